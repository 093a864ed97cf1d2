"""-m gpu: the continuous batcher's per-request logit processors and token masks (ContinuousBatcher.submit keywords,
set_token_mask; ftcf_batcher_submit_opts / ftcf_batcher_set_token_mask) on the tiny golden model, greedy unless said
otherwise.  Every expectation is exact by construction: a forced stream, a banned token replaced by the unconstrained run's
second choice, biases and penalties orders of magnitude above the raw logits."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import logit_processors_reference as lref
from tests.helpers import load_tiny

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


@pytest.fixture(scope="module")
def tiny():
    from tests import gpu_helpers as gh
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    cfg, w, z = load_tiny()
    return cfg, z, gh.make_op(cfg, w), gh


def batcher(op, **kw):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    return ContinuousBatcher(op, 4, 16, 64, 64, **kw)


def drain(cb, step=None):
    """{request_id: [event, ...]} of every iteration until the batcher is idle"""
    out, it = {}, 0
    while cb.busy():
        for e in (step or cb.step_ex)():
            out.setdefault(e[0], []).append(e)
        it += 1
        assert it < 200
    return out


def tokens(events):
    return [e[1] for e in events]


def ended_normally(events, n_new, end_id):
    flags = [e[2] for e in events]
    return flags == [False] * (len(events) - 1) + [True] and (len(events) == n_new or events[-1][1] == end_id)


@pytest.fixture(scope="module")
def plain(tiny):
    """the unconstrained streams every test compares with: z["prompt"] and z["prompt_b"], 8 tokens, through submit alone,
    with the top 20 pairs of every step"""
    cfg, z, op, gh = tiny
    runs = {}
    for name in ("prompt", "prompt_b"):
        cb = batcher(op)
        rid = cb.submit(z[name].tolist(), 8)
        runs[name] = drain(cb, lambda: cb.step(top_logprobs=20))[rid]
    return runs


def test_default_and_zero_options_are_todays_submit(tiny):
    from fastertransformer4codefuse_amd import capi
    cfg, z, op, gh = tiny
    p = z["prompt"].tolist()
    ids = np.asarray(p, dtype=np.int32)
    cb = batcher(op)

    def through_submit_opts(opts):
        rid = C.c_long(0)
        capi.check(capi.lib().ftcf_batcher_submit_opts(cb._h, ids.ctypes.data_as(C.POINTER(C.c_int)), len(p), 8, 0, C.c_float(0.0),
                                                       C.c_float(1.0), C.c_float(1.0), C.c_ulonglong(0), None, 0,
                                                       C.byref(opts) if opts is not None else None, C.byref(rid)))
        return rid.value

    # one request at a time: the same admission and the same decode steps as the first, so the same bits
    submits = [lambda: cb.submit(p, 8),
               lambda: cb.submit(p, 8, logit_bias=None, bad_words=None, presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0),
               lambda: cb.submit(p, 8, logit_bias={}, bad_words=[]),
               lambda: through_submit_opts(None), lambda: through_submit_opts(capi.LogitOptions()),
               lambda: through_submit_opts(capi.LogitOptions(struct_size=C.sizeof(capi.LogitOptions)))]
    streams = []
    for submit in submits:
        rid = submit()
        streams.append([e[1:] for e in drain(cb)[rid]])
    assert len(streams[0]) == 8 or streams[0][-1][0] == cfg["end_id"]
    for k, s in enumerate(streams[1:]):
        assert s == streams[0], (k + 1, s, streams[0])  # tokens, finished flags and log-probabilities


def test_forced_stream_by_masks_set_from_the_callback(tiny):
    cfg, z, op, gh = tiny
    V, end = cfg["vocab_size"], cfg["end_id"]
    forced = [17, 300, 5, 511, 0, 42]
    cb = batcher(op)
    seen, errors = [], []
    rid = cb.submit(z["prompt"].tolist(), 12)
    other = cb.submit(z["prompt_b"].tolist(), 6)  # rides along unmasked
    allowed = np.zeros(V, dtype=bool)
    allowed[forced[0]] = True
    cb.set_token_mask(rid, allowed)  # while it waits: governs the first token (a bool array here, id lists below)

    def on_token(request_id, token, finished):
        try:
            if request_id != rid:
                return
            seen.append(token)
            if not finished:
                cb.set_token_mask(rid, [forced[len(seen)]] if len(seen) < len(forced) else None)
        except Exception as ex:  # (an exception cannot cross the C callback)
            errors.append(ex)

    cb.set_token_callback(on_token)
    ev = drain(cb)
    cb.set_token_callback(None)
    assert not errors, errors
    assert tokens(ev[rid])[:len(forced)] == forced and tokens(ev[rid]) == seen
    assert len(ev[rid]) > len(forced) and ended_normally(ev[rid], 12, end), "after the mask is cleared the request goes on and ends"
    assert all(math.isfinite(e[3]) for e in ev[rid])
    assert all(abs(e[3]) < 1e-6 for e in ev[rid][:len(forced)]), "one allowed token: probability 1"
    assert ended_normally(ev[other], 6, end)


def test_banned_token_and_banned_bigram_give_the_second_choice(tiny, plain):
    cfg, z, op, gh = tiny
    p, run = z["prompt"].tolist(), plain["prompt"]
    s = tokens(run)
    assert len(s) >= 4 and all(e[4][0] == e[1] for e in run)
    for step in (0, 2):  # the precondition: the second choice of that step is not a near tie with the third
        assert run[step][5][1] - run[step][5][2] > 1e-3, (step, run[step][5][:3])
    cb = batcher(op)
    ev = {}
    a = cb.submit(p, 8, bad_words=[[s[0]]])
    ev.update(drain(cb))  # (one at a time, as the unconstrained run: the same admission, the same decode steps)
    b = cb.submit(p, 8, bad_words=[[s[1], s[2]]])
    ev.update(drain(cb))
    assert tokens(ev[a])[0] == run[0][4][1], (tokens(ev[a]), s, run[0][4][:3])
    assert s[0] not in tokens(ev[a])
    assert tokens(ev[b])[:3] == [s[0], s[1], run[2][4][1]], (tokens(ev[b]), s, run[2][4][:3])


def test_min_new_tokens_holds_a_biased_end_token_back(tiny):
    cfg, z, op, gh = tiny
    end, p = cfg["end_id"], z["prompt"].tolist()
    cb = batcher(op)
    a = cb.submit(p, 8, logit_bias={end: 1000.0})
    b = cb.submit(p, 8, logit_bias={end: 1000.0}, min_new_tokens=3)
    ev = drain(cb)
    assert [(e[1], e[2]) for e in ev[a]] == [(end, True)]
    tb = tokens(ev[b])
    assert len(tb) == 4 and end not in tb[:3] and tb[3] == end and [e[2] for e in ev[b]] == [False, False, False, True]


def simulate(V, end, n, **opts):
    """greedy over logits that are the options alone (raw logits = 0): the stream and the smallest decision margin"""
    hist, margin = [], math.inf
    for _ in range(n):
        x, _ = lref.process_row(np.zeros(V, dtype=np.float32), hist, 0, end, **opts)
        order = np.argsort(-x, kind="stable")
        margin = min(margin, x[order[0]] - x[order[1]])
        hist.append(int(order[0]))
    return hist, margin


@pytest.mark.parametrize("variant", ["frequency", "presence"])
def test_penalties_over_generated_tokens_steer_a_biased_stream(tiny, variant):
    cfg, z, op, gh = tiny
    V, end, p = cfg["vocab_size"], cfg["end_id"], z["prompt"].tolist()
    a, b = 100, 200
    p = p + [a, a, b]  # the prompt already holds a and b: its occurrences must not count
    opts = dict(bias=[(a, 1000.0), (b, 600.0)], frequency=300.0) if variant == "frequency" else dict(
        bias=[(a, 1000.0), (b, 600.0)], presence=500.0)
    want, margin = simulate(V, end, 6, **opts)
    if variant == "frequency":
        assert want == [a, a, b, a, b, a]
    else:
        assert want == [a, b, a, a, a, a]
    raw = np.abs(gh.run_op(op, np.asarray([p], dtype=np.int32), [len(p)], 6, V)["logits"]).max()
    assert margin > 2 * raw, (margin, raw)  # every decision is the options', whatever the model adds
    cb = batcher(op)
    rid = cb.submit(p, 6, logit_bias=dict(opts["bias"]), frequency_penalty=opts.get("frequency", 0.0),
                    presence_penalty=opts.get("presence", 0.0))
    assert tokens(drain(cb)[rid]) == want


def test_sampled_tokens_and_top_logprobs_stay_inside_the_mask(tiny):
    cfg, z, op, gh = tiny
    five = [9, 77, 130, 258, 511]
    cb = batcher(op)
    rid = cb.submit(z["prompt_b"].tolist(), 10, top_k=50, temperature=1.3, seed=11)
    cb.set_token_mask(rid, five)
    ev = drain(cb, lambda: cb.step(top_logprobs=5))[rid]
    assert len(ev) == 10 and all(e[1] in five for e in ev), tokens(ev)
    for e in ev:
        assert sorted(e[4]) == five and all(math.isfinite(v) for v in e[5]), e
        assert abs(sum(math.exp(v) for v in e[5]) - 1.0) < 1e-4 and math.isfinite(e[3])


def test_requests_without_options_are_unchanged_in_a_mixed_batch(tiny, plain):
    cfg, z, op, gh = tiny
    V = cfg["vocab_size"]
    cb = batcher(op)
    a = cb.submit(z["prompt"].tolist(), 8)
    x = cb.submit(z["prompt"].tolist(), 8, logit_bias={7: 50.0}, frequency_penalty=20.0)
    b = cb.submit(z["prompt_b"].tolist(), 8)
    y = cb.submit(z["prompt_b"].tolist(), 8, bad_words=[[tokens(plain["prompt_b"])[0]]])
    cb.set_token_mask(y, np.arange(V) % 2 == 1)
    ev = drain(cb)
    assert tokens(ev[a]) == tokens(plain["prompt"]) and tokens(ev[b]) == tokens(plain["prompt_b"])
    assert tokens(ev[x]) != tokens(plain["prompt"]) and all(t % 2 == 1 for t in tokens(ev[y]))


def test_guard_ends_a_request_that_has_no_token_left(tiny, plain):
    cfg, z, op, gh = tiny
    end = cfg["end_id"]
    cb = batcher(op)
    rid = cb.submit(z["prompt"].tolist(), 8, bad_words=[[40]])
    cb.set_token_mask(rid, [40])
    late = cb.submit(z["prompt_b"].tolist(), 8, bad_words=[[41]])  # ... and one that runs into the guard at a decode step
    seen = []
    cb.set_token_callback(lambda r, t, f: (seen.append(t), cb.set_token_mask(late, [41])) if r == late and not seen else None)
    ev = drain(cb)
    cb.set_token_callback(None)
    assert [(e[1], e[2]) for e in ev[rid]] == [(end, True)]
    assert len(ev[late]) == 2 and (ev[late][1][1], ev[late][1][2]) == (end, True)
    nxt = cb.submit(z["prompt"].tolist(), 8)
    assert tokens(drain(cb)[nxt]) == tokens(plain["prompt"])


def test_first_token_of_a_prefix_hit_goes_through_the_hook(tiny):
    cfg, z, op, gh = tiny
    p = np.random.RandomState(3).randint(3, cfg["vocab_size"], size=20).tolist()
    cb = batcher(op, prefix_cache=True)
    for _ in range(2):  # the second admission reuses the first one's page
        rid = cb.submit(p, 3, logit_bias={123: 1000.0}, bad_words=[[p[-1], 123]])
        cb.set_token_mask(rid, [123, 321])
        assert tokens(drain(cb)[rid])[0] == 321
    assert cb.prefix_stats()["hit_tokens"] == 16


def test_refusals_leave_the_batcher_usable(tiny, plain):
    from fastertransformer4codefuse_amd.capi import FtcfError
    cfg, z, op, gh = tiny
    V, p = cfg["vocab_size"], z["prompt"].tolist()
    cb = batcher(op)
    for kw in (dict(logit_bias=[(5, 1.0), (5, 2.0)]), dict(logit_bias={V: 1.0}), dict(bad_words=[[V]]), dict(logit_bias={-1: 1.0})):
        with pytest.raises((ValueError, FtcfError)):
            cb.submit(p, 4, **kw)
    with pytest.raises(TypeError):
        cb.submit_beam(p, 4, 2, logit_bias={5: 1.0})
    assert cb.status()["waiting"] == 0
    rid = cb.submit(p, 8)
    beam = cb.submit_beam(z["prompt_b"].tolist(), 3, 2)
    with pytest.raises(FtcfError):
        cb.set_token_mask(rid, [])  # no token allowed
    with pytest.raises(FtcfError):
        cb.set_token_mask(rid, np.zeros(V, dtype=bool))
    with pytest.raises(FtcfError):
        cb.set_token_mask(beam, [5])  # a waiting beam request
    with pytest.raises(FtcfError):
        cb.set_token_mask(10 ** 6, [5])  # nobody's id
    words = (C.c_uint * 3)(1, 1, 1)
    assert capi_set_mask(cb, rid, words, 3) == -1  # a wrong n_words
    ev = {}
    for e in cb.step_ex() + cb.step_ex():
        ev.setdefault(e[0], []).append(e)
    if cb.busy() and beam not in ev:
        with pytest.raises(FtcfError):
            cb.set_token_mask(beam, [5])  # a running beam request
    for k, v in drain(cb).items():
        ev.setdefault(k, []).extend(v)
    assert tokens(ev[rid]) == tokens(plain["prompt"]) and tokens(ev[beam]) == [-1]
    with pytest.raises(FtcfError):
        cb.set_token_mask(rid, [5])  # finished


def capi_set_mask(cb, rid, words, n):
    from fastertransformer4codefuse_amd import capi
    return capi.lib().ftcf_batcher_set_token_mask(cb._h, C.c_long(rid), words, n)
