"""-m gpu: ContinuousBatcher.step(top_logprobs=N) / ftcf_batcher_step_top -- in a mixed run in which requests arrive over time
every event carries the N best (id, log-probability) pairs of its step, the ones the engine alone returns for that request
(GptNeoXOp.forward top_logprobs).  The batcher's decode attention is paged, the engine's dense: values agree within the bound
of tests/test_gpu_batcher_log_probs.py (2e-3 + 2e-3 relative), ids are exact wherever the engine's neighbouring values are
further apart than twice that; a beam request's event carries (-1, NaN) pairs; plain step() calls in between are unchanged."""
import math

import numpy as np
import pytest

from tests.helpers import load_tiny

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
TOL = 2e-3
N = 5


@pytest.fixture(scope="module")
def tiny():
    from tests import gpu_helpers as gh
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    cfg, w, z = load_tiny()
    return cfg, w, z, gh.make_op(cfg, w)


def alone(op, prompt, n_new, V, **kw):
    """the engine alone: tokens up to the end / the last, output_log_probs, top ids [n, N], top values [n, N]"""
    from tests.test_gpu_top_logprobs_engine import run
    p = np.asarray(prompt, dtype=np.int32)
    r = run(op, p[None, :], [len(p)], n_new, V, N=N, debug=False, **kw)
    n = int(r["sequence_lengths"][0]) - len(p)
    return r["output_ids"][0, len(p):len(p) + n].tolist(), r["output_log_probs"][0, :n], r["top_ids"][0, :n], r["top_values"][0, :n]


def check_pairs(got_ids, got_lps, want_ids, want_lps, what):
    bound = lambda v: TOL + TOL * abs(float(v))
    want_ids, want_lps = want_ids.tolist(), want_lps.tolist()
    assert len(set(got_ids)) == N and all(math.isfinite(v) for v in got_lps), (what, got_ids, got_lps)
    for j in range(N):
        assert abs(got_lps[j] - want_lps[j]) <= bound(want_lps[j]), (what, j, got_lps, want_lps)
        if got_ids[j] != want_ids[j]:  # only a near tie may reorder (or bring the N + 1-th in at the end)
            k = want_ids.index(got_ids[j]) if got_ids[j] in want_ids else N - 1
            assert abs(want_lps[k] - want_lps[j]) <= 2 * bound(want_lps[j]), (what, j, got_ids, want_ids, want_lps)


def test_events_of_a_mixed_run_carry_the_engines_pairs(tiny):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z, op = tiny
    V = cfg["vocab_size"]
    rng = np.random.RandomState(7)
    greedy = [(z["prompt"].tolist(), 8, {}), (z["prompt_b"].tolist(), 6, {}), (rng.randint(3, V, size=5).tolist(), 7, {}),
              (rng.randint(3, V, size=20).tolist(), 5, {})]
    sampled = [(rng.randint(3, V, size=9).tolist(), 6, dict(top_k=4, temperature=0.8, seed=21))]
    reqs = greedy + sampled
    cb = ContinuousBatcher(op, 4, 16, 64, 64)
    ids, got = {}, {}

    def take(events, with_pairs):
        for e in events:
            assert len(e) == (6 if with_pairs else 3)
            got.setdefault(ids[e[0]], []).append(e)

    for k in (0, 1):
        ids[cb.submit(reqs[k][0], reqs[k][1], **reqs[k][2])] = k
    take(cb.step(top_logprobs=N), True)
    take(cb.step(top_logprobs=N), True)
    for k in (2, 4):  # arrive while the first two decode
        ids[cb.submit(reqs[k][0], reqs[k][1], **reqs[k][2])] = k
    take(cb.step(top_logprobs=N), True)
    plain_at = {k: len(v) for k, v in got.items()}
    take(cb.step(), False)  # a plain call in between: the same tokens, no pairs, nothing left behind
    ids[cb.submit(reqs[3][0], reqs[3][1], **reqs[3][2])] = 3
    it = 0
    while cb.busy():
        take(cb.step(top_logprobs=N), True)
        it += 1
        assert it < 200
    assert sorted(got) == [0, 1, 2, 3, 4]
    for k, (p, n, kw) in enumerate(reqs):
        ekw = dict(top_k=kw.get("top_k", 1), temperature=kw.get("temperature"), random_seed=kw.get("seed"))
        toks, lps, tids, tvals = alone(op, p, n, V, **ekw)
        assert [e[1] for e in got[k]] == toks, (k, [e[1] for e in got[k]], toks)
        assert [e[2] for e in got[k]] == [False] * (len(toks) - 1) + [True]
        for i, e in enumerate(got[k]):
            if len(e) == 3:
                assert i == plain_at[k]
                continue
            assert abs(e[3] - lps[i]) <= TOL + TOL * abs(lps[i])
            check_pairs(e[4], e[5], tids[i], tvals[i], (k, i))
            if "top_k" not in kw:
                assert e[4][0] == e[1], "a greedy request's first pair is its token"
            assert e[1] in e[4]  # top_k 4 <= N


def test_beam_event_carries_the_nan_pattern(tiny):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z, op = tiny
    cb = ContinuousBatcher(op, 4, 16, 64, 64)
    rb = cb.submit_beam(z["prompt"].tolist(), 4, 2)
    rg = cb.submit(z["prompt_b"].tolist(), 4)
    evs = []
    while cb.busy():
        evs += cb.step(top_logprobs=3)
    beam = [e for e in evs if e[0] == rb]
    assert len(beam) == 1 and beam[0][1] == -1 and beam[0][4] == [-1, -1, -1] and all(math.isnan(v) for v in beam[0][5])
    mine = [e for e in evs if e[0] == rg]
    assert len(mine) == 4 and all(e[4][0] == e[1] and all(math.isfinite(v) for v in e[5]) for e in mine)


def test_bad_top_n_is_refused(tiny):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    from fastertransformer4codefuse_amd import capi
    import ctypes as C
    cfg, w, z, op = tiny
    cb = ContinuousBatcher(op, 2, 16, 32, 64)
    n = C.c_int(0)
    ids, lps = (C.c_int * (4 * 21))(), (C.c_float * (4 * 21))()
    for top_n, a, b in ((21, ids, lps), (0, ids, lps), (5, None, lps)):
        assert capi.lib().ftcf_batcher_step_top(cb._h, cb._ids, cb._tok, cb._fin, cb._lp, top_n, a, b, 4, C.byref(n)) == -1
    assert cb.step() == []
