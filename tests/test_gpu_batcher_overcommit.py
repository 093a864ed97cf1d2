"""-m gpu: the continuous batcher with overcommit (ftcf_batcher_create_opts): requests take pages as they grow,
the latest arrival is swapped out to host pages when the pool runs dry and resumes later, in any slot, on fresh pages.

Swapping is a bit-exact copy, so the batcher's contract is unchanged and the checks ask for equality: on the tiny model every
stream is what the CPU oracle generates for the request alone (prompts chosen on the oracle for a top-2 margin of more than
1e-2 of max|logit| along the whole greedy trajectory and no end token), on the random models what the same requests produce
on a batcher whose pool is large enough that nobody is preempted.  Every test ends with all pages back and the swap space empty."""
import numpy as np
import pytest

from tests.helpers import load_tiny, random_model
from tests.test_gpu_batcher import MID, _beam_alone, _oracle_alone

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
MID128 = dict(head_num=8, size_per_head=128, inter_size=4096, num_layer=2, vocab_size=2048, rotary_dim=32, start_id=0, end_id=2)


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


@pytest.fixture(scope="module")
def tiny(gh):
    from oracle import oracle as orc
    from tests.helpers import weight_list_to_layers
    cfg, w, z = load_tiny()
    layers, glob = weight_list_to_layers(cfg, w)
    return dict(cfg=cfg, z=z, V=cfg["vocab_size"], end_id=cfg["end_id"], op=gh.make_op(cfg, w),
                model=orc.Model(dict(cfg, fp16=1), layers, glob), refs={})


def _prompt(seed, n, V):
    return np.random.RandomState(1000 + seed).randint(3, V, size=n).tolist()


# (length, new tokens) -> seed of a prompt with a wide greedy margin on the tiny model (see the module docstring)
WIDE = {(10, 6): (56, 52, 35, 51), (9, 30): (54,), (14, 30): (14,), (11, 30): (44,), (19, 12): (2,), (13, 24): (30,)}


def _wide(tiny, n, new, k=0):
    """(prompt, new tokens, the oracle's stream for it alone)"""
    key = (n, new, k)
    if key not in tiny["refs"]:
        p = _prompt(WIDE[(n, new)][k], n, tiny["V"])
        ref = _oracle_alone(tiny["model"], p, new, tiny["end_id"], top_k=1)
        assert len(ref) == new  # (no end token: the request really grows to its full length)
        tiny["refs"][key] = (p, new, ref)
    return tiny["refs"][key]


def _drive(cb, arrivals, stepper=None, after_step=None, limit=3000):
    """arrivals: {iteration: [(key, submit(cb) -> request id), ...]} -> ({key: tokens}, [(key, token, finished, ...)], {id: key});
    after_step(iteration, {id: key}, the iteration's events) runs after every step()"""
    ids, got, events, it = {}, {}, [], 0
    pending = dict(arrivals)
    while pending or cb.busy():
        for key, submit in pending.pop(it, []):
            ids[submit(cb)] = key
        evs = [(ids[ev[0]],) + tuple(ev[1:]) for ev in (stepper(cb) if stepper else cb.step())]
        events += evs
        for ev in evs:
            if ev[1] >= 0:
                got.setdefault(ev[0], []).append(ev[1])
        if after_step:
            after_step(it, ids, evs)  # (evs: this iteration's events)
        it += 1
        assert it < limit
    return got, events, ids


def _greedy(prompt, new):
    return lambda cb: cb.submit(prompt, new)


def _all_back(cb, free0):
    st, px, pe = cb.status(), cb.prefix_stats(), cb.preempt_stats()
    assert st == {"waiting": 0, "running": 0, "free_pages": free0 - px["cached_pages"]}, (st, px)
    assert pe["swap_pages_used"] == 0 and pe["swapped_requests"] == 0, pe
    return pe


def test_more_requests_run_at_once(tiny):
    """four prompts of 10 tokens that declare 40 new ones in a pool of 12 pages of 8: reservation runs one of them, overcommit
    all four; the clients cancel after 6 tokens and nobody was ever preempted"""
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    reqs = [_wide(tiny, 10, 6, k) for k in range(4)]
    geometry = dict(max_batch=4, page_tokens=8, num_pages=12, max_seq_len=64)
    plain = ContinuousBatcher(tiny["op"], **geometry)
    assert plain.preempt_stats() == dict.fromkeys(("enabled", "swapped_requests", "swap_pages_used", "swap_pages_total", "preemptions",
                                                   "resumes", "pages_out", "pages_in"), 0)
    rids = [plain.submit(p, 40) for p, _, _ in reqs]
    plain.step()
    assert plain.status()["running"] == 1 and plain.status()["waiting"] == 3
    for rid in rids:
        assert plain.cancel(rid)
    del plain
    cb = ContinuousBatcher(tiny["op"], overcommit=True, **geometry)
    free0 = cb.status()["free_pages"]
    assert cb.preempt_stats()["enabled"] == 1 and cb.preempt_stats()["swap_pages_total"] == 12
    rids = {cb.submit(p, 40): k for k, (p, _, _) in enumerate(reqs)}
    got = {k: [] for k in range(4)}
    first = True
    while cb.busy():
        for rid, tok, fin in cb.step():
            got[rids[rid]].append(tok)
            assert not fin
        if first:
            assert cb.status()["running"] == 4 and cb.status()["waiting"] == 0
            first = False
        for rid, k in rids.items():
            if len(got[k]) == 6:
                got[k].append(None)  # (cancelled: no further token may arrive)
                assert cb.cancel(rid)
    for k in range(4):
        assert got[k] == reqs[k][2] + [None], (k, got[k], reqs[k][2])
    assert _all_back(cb, free0)["preemptions"] == 0


FORCED = [("tiny", 0, 8, None, 10), ("tiny", 0, 32, "1", 5), ("tiny", 0, 32, "0", 5), ("mid", 1, 16, "1", 6), ("mid", 1, 16, "0", 6)]


@pytest.mark.parametrize("model,int8_mode,page_tokens,rows,num_pages", FORCED)
def test_forced_preemption_keeps_every_stream_exact(gh, tiny, monkeypatch, model, int8_mode, page_tokens, rows, num_pages):
    """three greedy requests of 9 / 14 / 11 prompt tokens and 30 new ones in a pool that holds their admissions (one or two pages
    each) but not their full lengths: requests are swapped out and resume, and every stream is exact -- on the per-GEMM launches
    and on the rows kernel's paged form (page_tokens 32 on the tiny model, 16 at size_per_head 128)"""
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    if rows is not None:
        monkeypatch.setenv("FTCF_BATCHER_ROWS", rows)
    if model == "tiny":
        op = tiny["op"]
        reqs = [_wide(tiny, 9, 30), _wide(tiny, 14, 30), _wide(tiny, 11, 30)]
    else:
        op = gh.make_op(MID128, random_model(MID128, seed=5 + int8_mode, std=0.04), int8_mode=int8_mode)
        rng = np.random.RandomState(77)
        reqs = [(rng.randint(3, MID128["vocab_size"], size=n).tolist(), 30, None) for n in (9, 14, 11)]
    arrivals = {0: [(k, _greedy(p, new)) for k, (p, new, _) in enumerate(reqs)]}
    if model != "tiny":  # the reference: the same requests where nothing is preempted (reservation, a pool for all of them)
        big = ContinuousBatcher(op, max_batch=3, page_tokens=page_tokens, num_pages=48, max_seq_len=64)
        ref, _, _ = _drive(big, arrivals)
        del big
        reqs = [(p, new, ref[k]) for k, (p, new, _) in enumerate(reqs)]
    cb = ContinuousBatcher(op, max_batch=3, page_tokens=page_tokens, num_pages=num_pages, max_seq_len=64, overcommit=True)
    free0 = cb.status()["free_pages"]
    seen = {}

    def after_step(it, ids, evs):
        if it == 0:
            assert cb.status()["running"] == 3  # all three were admitted on the pages of their prompts
        if it == 3 and rows is not None:
            assert op.stats()["decode_path"] == (3 if rows == "1" else 2)  # the layers of the last decode step
        seen["swapped"] = max(seen.get("swapped", 0), cb.preempt_stats()["swapped_requests"])
        assert cb.status()["waiting"] == cb.preempt_stats()["swapped_requests"]  # (swapped-out requests count as waiting)

    got, events, _ = _drive(cb, arrivals, after_step=after_step)
    for k, (_, new, ref) in enumerate(reqs):
        assert got[k] == ref, (k, got[k], ref)
    pe = _all_back(cb, free0)
    assert pe["preemptions"] > 0 and pe["resumes"] == pe["preemptions"] and pe["pages_in"] == pe["pages_out"] > 0, pe
    assert seen["swapped"] > 0
    assert sorted(k for k, _, fin in events if fin) == [0, 1, 2]


def test_no_event_is_lost_doubled_or_made_by_a_resume(tiny):
    """the event stream and the callback order of preempted requests: every token once, in order, one `finished` per request, the
    callback called for exactly the events step() returns, in their order -- and nothing at a resume"""
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    reqs = [_wide(tiny, 9, 30), _wide(tiny, 14, 30), _wide(tiny, 11, 30)]
    cb = ContinuousBatcher(tiny["op"], max_batch=3, page_tokens=8, num_pages=10, max_seq_len=64, overcommit=True)
    free0 = cb.status()["free_pages"]
    called, rises, seen = [], [], {"resumes": 0}
    cb.set_token_callback(lambda rid, tok, fin: called.append((rid, tok, fin)))

    def after_step(it, ids, evs):
        # who emitted = who ran in the step's decode (or was admitted); after it some finished and `rise` requests resumed: a
        # resumed request is running now and has emitted nothing
        rise = cb.preempt_stats()["resumes"] - seen["resumes"]
        seen["resumes"] += rise
        emitters, finished = {e[0] for e in evs}, sum(1 for e in evs if e[2])
        assert len(emitters) == len(evs) and len(emitters) == cb.status()["running"] - rise + finished, (it, evs, rise, cb.status())
        rises.append(rise)

    got, events, ids = _drive(cb, {0: [(k, _greedy(p, new)) for k, (p, new, _) in enumerate(reqs)]}, after_step=after_step)
    cb.set_token_callback(None)
    assert [(ids[rid], tok, fin) for rid, tok, fin in called] == events
    for k, (_, new, ref) in enumerate(reqs):
        mine = [(tok, fin) for key, tok, fin in events if key == k]
        assert mine == [(t, i == new - 1) for i, t in enumerate(ref)], (k, mine)
    pe = _all_back(cb, free0)
    assert pe["preemptions"] > 0 and sum(rises) == pe["resumes"] and max(rises) > 0 and len(events) == sum(new for _, new, _ in reqs)


def _sampled_run(cb, V, prompts, stop, stepper):
    """A short greedy request (slot 0), a long greedy one (slot 1), then the sampled request with every per-request state there is
    (slot 2, the latest arrival: the victim); its token mask arrives from the callback after its fifth token"""
    rng = np.random.RandomState(3)
    allowed = np.unique(np.concatenate([rng.randint(3, V, size=V // 2), np.arange(3, 40)]))
    box = {}

    def on_token(rid, tok, fin):
        if rid == box.get("rid"):
            box["n"] = box.get("n", 0) + 1
            if box["n"] == 5:
                cb.set_token_mask(rid, allowed)

    def sampled(cb):
        box["rid"] = cb.submit(prompts[2], 30, top_k=8, top_p=0.9, temperature=0.7, seed=1234, repetition_penalty=1.3,
                               stop_words=[stop] if stop else None, presence_penalty=0.4, frequency_penalty=0.2,
                               logit_bias={5: 1.5, 17: -2.0, 40: float("-inf")}, min_new_tokens=8)
        return box["rid"]

    trace = []  # per iteration: requests swapped out after it, resumes so far, who emitted, who finished

    def after_step(it, ids, evs):
        pe = cb.preempt_stats()
        trace.append((pe["swapped_requests"], pe["resumes"], {e[0] for e in evs}, {e[0] for e in evs if e[2]}))

    cb.set_token_callback(on_token)
    got, events, _ = _drive(cb, {0: [(0, _greedy(prompts[0], 14)), (1, _greedy(prompts[1], 40)), (2, sampled)]}, stepper=stepper,
                            after_step=after_step)
    cb.set_token_callback(None)
    return got, [ev for ev in events if ev[0] == 2], trace


def _check_the_sampled_request_was_the_victim(trace):
    """whenever a request is swapped out it is the sampled one (it emits nothing, the long greedy one goes on); it had its mask by
    then (five tokens), went on after its last resume, and at its first resume the short request had left slot 0"""
    out = [i for i, (swapped, _, _, _) in enumerate(trace) if swapped > 0]
    assert out and all(trace[i][0] == 1 and 2 not in trace[i][2] and 1 in trace[i][2] for i in out), [trace[i] for i in out]
    assert sum(1 for t in trace[:out[0]] if 2 in t[2]) >= 5
    assert any(2 in t[2] for t in trace[out[-1] + 1:])
    first_resume = next(i for i, t in enumerate(trace) if t[1] > 0)
    assert any(0 in t[3] for t in trace[:first_resume + 1]), "the short request still held slot 0 when the victim resumed"


def test_the_whole_state_of_a_sampled_request_survives_the_swap(gh):
    """top-k / top-p / temperature with a seed, repetition, presence and frequency penalties, logit bias, min_new_tokens, a
    two-token stop sequence and a token mask set from the callback: the victim's tokens, log-probabilities and top alternatives
    are those of the run in which it never left (the draw counter, the cumulative log-probability, the history and the
    processors' rows all went to host and came back -- into slot 0, which the short request has freed by then)"""
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    V = MID["vocab_size"]
    op = gh.make_op(MID, random_model(MID, seed=17), int8_mode=0)
    rng = np.random.RandomState(41)
    prompts = [rng.randint(3, V, size=n).tolist() for n in (6, 10, 12)]

    def make(small):
        if small:
            return ContinuousBatcher(op, max_batch=3, page_tokens=8, num_pages=7, max_seq_len=64, overcommit=True)
        return ContinuousBatcher(op, max_batch=3, page_tokens=8, num_pages=40, max_seq_len=64)

    free_run, _, _ = _sampled_run(make(False), V, prompts, None, lambda cb: cb.step_ex())
    s = free_run[2]
    assert len(s) == 30
    k = next(i for i in range(18, 28) if all(s[j:j + 2] != s[i:i + 2] for j in range(i)))  # a pair that has not occurred before
    stop = s[k:k + 2]
    for stepper in (lambda cb: cb.step_ex(), lambda cb: cb.step(top_logprobs=3)):
        big, small = make(False), make(True)
        free0 = small.status()["free_pages"]
        ref_got, ref_ev, _ = _sampled_run(big, V, prompts, stop, stepper)
        got, ev, trace = _sampled_run(small, V, prompts, stop, stepper)
        _check_the_sampled_request_was_the_victim(trace)
        assert ref_got[2] == s[:k + 2]  # the stop sequence ends it
        assert got == ref_got, (got, ref_got)
        assert [e[1:3] for e in ev] == [e[1:3] for e in ref_ev]
        np.testing.assert_allclose([e[3] for e in ev], [e[3] for e in ref_ev], rtol=1e-5)
        if len(ev[0]) > 4:
            assert [e[4] for e in ev] == [e[4] for e in ref_ev]
            np.testing.assert_allclose([e[5] for e in ev], [e[5] for e in ref_ev], rtol=1e-5)
        pe = _all_back(small, free0)
        assert pe["preemptions"] > 0 and pe["resumes"] == pe["preemptions"], pe
        assert big.preempt_stats()["preemptions"] == 0


def test_beam_groups_stay_put(gh, tiny):
    """a width-3 beam group keeps its budget and its pages while the ordinary requests beside it are swapped out and back: its
    hypotheses are the engine's own, the ordinary streams are exact"""
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    z, V, op = tiny["z"], tiny["V"], tiny["op"]
    reqs = [_wide(tiny, 9, 30), _wide(tiny, 14, 30), _wide(tiny, 11, 30)]
    bp, b_new, K = z["prompt"].tolist(), 30, 3
    b_ref = _beam_alone(gh, op, bp, b_new, V, K)
    # the group's budget (3 x 6 pages) and the 10 pages the three ordinary requests fight for
    cb = ContinuousBatcher(op, max_batch=6, page_tokens=8, num_pages=28, max_seq_len=64, overcommit=True)
    free0 = cb.status()["free_pages"]
    arrivals = {0: [("beam", lambda cb: cb.submit_beam(bp, b_new, K))], 1: [(k, _greedy(p, new)) for k, (p, new, _) in enumerate(reqs)]}
    got, events, ids = _drive(cb, arrivals)
    for k, (_, new, ref) in enumerate(reqs):
        assert got[k] == ref, (k, got[k], ref)
    assert [e for e in events if e[0] == "beam"] == [("beam", -1, True)]
    bid = next(rid for rid, key in ids.items() if key == "beam")
    out, lens, cum = cb.beam_result(bid)
    assert np.array_equal(out, b_ref[0]) and np.array_equal(lens, b_ref[1]), (out, b_ref[0])
    np.testing.assert_allclose(cum, b_ref[2], rtol=2e-3, atol=2e-3)
    pe = _all_back(cb, free0)
    assert pe["preemptions"] > 0 and pe["resumes"] == pe["preemptions"], pe


def test_cached_pages_are_evicted_before_anybody_is_preempted(tiny):
    """with the prefix cache: cached pages nobody holds make room first (evictions rise, nobody is preempted yet), then
    requests are swapped out; the latest arrival -- admitted on two cached pages of an earlier prompt -- is among them and
    resumes exactly, on private pages"""
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    a, b = _wide(tiny, 9, 30), _wide(tiny, 14, 30)
    x, y = _wide(tiny, 19, 12), _wide(tiny, 13, 24)
    cb = ContinuousBatcher(tiny["op"], max_batch=3, page_tokens=8, num_pages=10, max_seq_len=64, prefix_cache=True, overcommit=True)
    free0 = cb.status()["free_pages"]
    got, _, _ = _drive(cb, {0: [("x", _greedy(x[0], x[1])), ("y", _greedy(y[0], y[1]))]})
    assert got["x"] == x[2] and got["y"] == y[2]
    assert cb.prefix_stats()["cached_pages"] == 3 and cb.prefix_stats()["evictable_pages"] == 3  # 2 + 1 full prompt blocks
    assert cb.preempt_stats()["preemptions"] == 0
    track = []

    def after_step(it, ids, evs):
        track.append((cb.prefix_stats()["evictions"], cb.preempt_stats()["preemptions"]))

    got, _, _ = _drive(cb, {0: [("a", _greedy(a[0], a[1])), ("b", _greedy(b[0], b[1])), ("x2", _greedy(x[0], x[1]))]}, after_step=after_step)
    assert got["a"] == a[2] and got["b"] == b[2] and got["x2"] == x[2], got
    assert cb.prefix_stats()["hit_tokens"] == 16  # x2 was admitted on the two cached blocks of x
    assert any(ev > 0 and pre == 0 for ev, pre in track), track  # eviction came first ...
    assert track[-1][0] > 0 and track[-1][1] > 0, track         # ... then preemption
    pe = _all_back(cb, free0)
    assert pe["resumes"] == pe["preemptions"] and pe["pages_in"] == pe["pages_out"]


def test_growth_inside_a_chunked_admission(tiny, monkeypatch):
    """FTCF_BATCHER_PREFILL_CHUNK=8: a 19-token prompt arrives while two slots decode across a page boundary; the decode steps
    between its chunks take the pages the running slots need, later somebody is preempted, and all three streams are exact"""
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    monkeypatch.setenv("FTCF_BATCHER_PREFILL_CHUNK", "8")
    a, b, c = _wide(tiny, 9, 30), _wide(tiny, 14, 30), _wide(tiny, 19, 12)
    cb = ContinuousBatcher(tiny["op"], max_batch=3, page_tokens=8, num_pages=10, max_seq_len=64, overcommit=True)
    free0 = cb.status()["free_pages"]
    free = {}

    def after_step(it, ids, evs):
        free[it] = cb.status()["free_pages"]

    # iteration 7 ends with the 9-token request at 16 tokens: the first decode step between the chunks takes its third page
    got, events, _ = _drive(cb, {0: [(0, _greedy(a[0], a[1])), (1, _greedy(b[0], b[1]))], 7: [(2, _greedy(c[0], c[1]))]}, after_step=after_step)
    assert got[0] == a[2] and got[1] == b[2] and got[2] == c[2], got
    assert free[6] - free[7] == 3 + 1  # the admission's three pages and the page a decode step inside it took
    at = [i for i, e in enumerate(events) if e[0] == 2][0]  # (7 decode steps of two slots came before iteration 7's admission)
    assert (at - 2 * 7) // 2 >= 2 and [e[0] for e in events[:at]] == [0, 1] * (at // 2)  # >= 2 decode steps ran inside the admission
    pe = _all_back(cb, free0)
    assert pe["preemptions"] > 0 and pe["resumes"] == pe["preemptions"], pe


def test_cancelling_a_swapped_out_request_returns_its_host_pages(tiny):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    reqs = [_wide(tiny, 9, 30), _wide(tiny, 14, 30), _wide(tiny, 11, 30)]
    cb = ContinuousBatcher(tiny["op"], max_batch=3, page_tokens=8, num_pages=10, max_seq_len=64, overcommit=True)
    free0 = cb.status()["free_pages"]
    rids = [cb.submit(p, new) for p, new, _ in reqs]
    got = {rid: [] for rid in rids}
    cancelled = None
    while cb.busy():
        for rid, tok, fin in cb.step():
            got[rid].append(tok)
        pe = cb.preempt_stats()
        if cancelled is None and pe["swapped_requests"] > 0:
            running = cb.status()["running"]
            assert pe["swap_pages_used"] > 0 and pe["swapped_requests"] == 1
            cancelled = rids[2]  # (the latest arrival is the victim)
            assert cb.cancel(cancelled)
            assert cb.preempt_stats()["swap_pages_used"] == 0 and cb.preempt_stats()["swapped_requests"] == 0
            assert cb.status()["running"] == running and cb.status()["waiting"] == 0
            assert not cb.cancel(cancelled)
            with pytest.raises(RuntimeError):
                cb.set_token_mask(cancelled, [3, 4])
    assert cancelled is not None
    assert got[rids[0]] == reqs[0][2] and got[rids[1]] == reqs[1][2]
    assert got[cancelled] == reqs[2][2][:len(got[cancelled])] and len(got[cancelled]) < 30
    _all_back(cb, free0)


def test_a_full_swap_space_fails_the_step_and_the_batcher_goes_on(tiny):
    """swap_pages=1 and victims of four pages (the slot that fails is the first to grow in its step; the other order is
    test_a_slot_that_grew_in_the_step_that_failed_keeps_its_page): step() raises "swap space exhausted" before the step enqueues anything, as often as it
    is called; after one request has been cancelled the other one drains, exact"""
    from fastertransformer4codefuse_amd import capi
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    a, b = _wide(tiny, 9, 30), _wide(tiny, 14, 30)
    cb = ContinuousBatcher(tiny["op"], max_batch=2, page_tokens=8, num_pages=8, max_seq_len=64, overcommit=True, swap_pages=1)
    free0 = cb.status()["free_pages"]
    assert cb.preempt_stats()["swap_pages_total"] == 1
    ra, rb = cb.submit(a[0], a[1]), cb.submit(b[0], b[1])
    got, failed, it = {ra: [], rb: []}, 0, 0
    while cb.busy():
        try:
            for rid, tok, fin in cb.step():
                got[rid].append(tok)
        except capi.FtcfError as e:
            assert e.code == -2 and "swap space exhausted" in str(e)
            failed += 1
            before = (cb.status(), cb.preempt_stats(), {k: len(v) for k, v in got.items()})
            if failed == 1:
                continue  # (call again: the same answer, nothing has moved)
            assert failed == 2 and before[0]["running"] == 2 and before[1]["preemptions"] == 0
            assert cb.cancel(rb)
        it += 1
        assert it < 500
    assert failed == 2
    assert got[ra] == a[2] and got[rb] == b[2][:len(got[rb])] and 10 < len(got[rb]) < 30
    _all_back(cb, free0)


def test_a_slot_that_grew_in_the_step_that_failed_keeps_its_page(tiny):
    """Two requests cross a page boundary in the SAME step with one page free and swap_pages=1: the lower slot takes the page,
    the upper one finds no victim that fits (both hold three pages) and step() fails.  The page the lower slot took must be in the
    device's page table all the same -- the slot will not grow again for eight tokens, and a row that still ended in its padding
    would send them to page 0, the request's own first page.  After the other request is cancelled the survivor's stream is exact."""
    from fastertransformer4codefuse_amd import capi
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    a, b = _wide(tiny, 11, 30), _wide(tiny, 19, 12)  # 11 and 19 tokens: both reach a multiple of 8 after five decode steps
    cb = ContinuousBatcher(tiny["op"], max_batch=2, page_tokens=8, num_pages=6, max_seq_len=64, overcommit=True, swap_pages=1)
    free0 = cb.status()["free_pages"]
    ra, rb = cb.submit(a[0], a[1]), cb.submit(b[0], b[1])
    got, failed, it = {ra: [], rb: []}, 0, 0
    while cb.busy():
        try:
            for rid, tok, fin in cb.step():
                got[rid].append(tok)
            if it == 0:
                assert cb.status() == {"waiting": 0, "running": 2, "free_pages": 1}  # 2 + 3 pages taken
        except capi.FtcfError as e:
            assert e.code == -2 and "swap space exhausted" in str(e)
            failed += 1
            assert failed == 1 and len(got[ra]) == 6 and len(got[rb]) == 6  # the sixth decode step: 16 and 24 tokens cached
            assert cb.status() == {"waiting": 0, "running": 2, "free_pages": 0}  # the lower slot has grown, nobody has left
            assert cb.cancel(rb)
        it += 1
        assert it < 500
    assert failed == 1
    assert got[ra] == a[2], (got[ra], a[2])
    assert got[rb] == b[2][:6]
    pe = _all_back(cb, free0)
    assert pe["preemptions"] == 0


def test_overcommit_is_refused_under_tensor_parallelism(gh):
    """every rank would have to swap the same requests: not built, and an error at creation rather than a silent reservation"""
    import threading
    from fastertransformer4codefuse_amd import capi
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    from fastertransformer4codefuse_amd.gptneox_op import LocalTensorParallelGroup
    from tests.helpers import shard_weights
    cfg, w, _ = load_tiny()
    group, refused, err = LocalTensorParallelGroup(), [False, False], []

    def worker(r):
        try:
            op = gh.make_op(cfg, shard_weights(cfg, w, 2, r), tp=2, rank=r, comm=group)
            with pytest.raises(capi.FtcfError, match="tensor_para_size 1"):
                ContinuousBatcher(op, max_batch=2, page_tokens=8, num_pages=16, max_seq_len=64, overcommit=True)
            assert ContinuousBatcher(op, max_batch=2, page_tokens=8, num_pages=16, max_seq_len=64).preempt_stats()["enabled"] == 0
            refused[r] = True
        except BaseException as e:  # noqa: B902 (reported by the main thread)
            err.append(e)

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not err, err
    assert refused == [True, True]
