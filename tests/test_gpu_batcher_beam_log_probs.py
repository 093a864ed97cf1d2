"""-m gpu: per-token log-probabilities of beam requests inside the continuous batcher (submit_beam(token_log_probs=True) /
ftcf_batcher_submit_beam_opts / ftcf_batcher_beam_result_ex): the values are the engine's own for the request alone
(GptNeoXOp.beam_log_probs), next to greedy neighbours, through the chunked admission, with beams that end early; the edges."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library)

from tests.helpers import load_tiny, random_model
from tests.test_gpu_batcher import MID
from tests.test_gpu_beam_log_probs import assert_telescopes, bits

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
TOL = dict(rtol=2e-3, atol=2e-3)  # (test_beam_requests_share_the_batcher_with_greedy_ones: the cumulative scores of these shapes)


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


def beam_alone(gh, op, prompt, n_new, V, K, **kw):
    """What the engine returns for this prompt by itself: (output_ids, sequence_lengths, cum_log_probs, log_probs [K, n_new])."""
    r = gh.run_op_beam(op, np.asarray(prompt, np.int32)[None, :], [len(prompt)], n_new, V, K, **kw)
    return r["output_ids"][0], r["sequence_lengths"][0], r["cum_log_probs"].reshape(-1), op.beam_log_probs().cpu().numpy()[0]


def check_result(res, ref, K, n_new, n_prompt):
    assert len(res) == 4
    out, lens, cum, lp = res
    assert lp.shape == (K, n_new) and lp.dtype == np.float32
    assert np.array_equal(out, ref[0]), (out, ref[0])  # the tokens first: the values belong to them
    assert np.array_equal(lens, ref[1])
    print("max |batcher - engine|", float(np.abs(lp - ref[3]).max()))
    np.testing.assert_allclose(lp, ref[3], **TOL)
    assert (bits(lp)[ref[3] == 0] == 0).all(), "0 where the engine's are"
    if (lens == n_prompt + n_new).all():  # no beam ended early: the values sum to the batcher's own score
        assert_telescopes(lp, cum)
    return lp


@pytest.mark.parametrize("page_tokens", [8, 16])
def test_beam_requests_return_their_token_log_probs_next_to_greedy_ones(gh, page_tokens):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z = load_tiny()
    V = cfg["vocab_size"]
    op = gh.make_op(cfg, w)
    rng = np.random.RandomState(5)
    greedy = [(z["prompt"].tolist(), 10), (rng.randint(3, V, size=11).tolist(), 7)]
    beams = [(z["prompt"].tolist(), 9, 3, {}), (z["prompt_b"][:6].tolist(), 12, 4, dict(beam_search_diversity_rate=[-0.4]))]
    refs = [beam_alone(gh, op, p, n, V, K, **kw) for p, n, K, kw in beams]
    cb = ContinuousBatcher(op, max_batch=6, page_tokens=page_tokens, num_pages=200 // page_tokens + 8, max_seq_len=48)
    free0 = cb.status()["free_pages"]
    arrivals = {0: [("g", 0), ("b", 0)], 1: [("g", 1)], 3: [("b", 1)]}
    bids, done, it = {}, set(), 0
    while arrivals or cb.busy():
        for kind, i in arrivals.pop(it, []):
            if kind == "g":
                cb.submit(*greedy[i])
            else:
                p, n, K, kw = beams[i]
                bids[cb.submit_beam(p, n, K, float(kw.get("beam_search_diversity_rate", [0.0])[0]), token_log_probs=True)] = i
        done |= {rid for rid, tok, fin in cb.step() if rid in bids}
        it += 1
        assert it < 2000
    assert done == set(bids)
    for rid, i in bids.items():
        p, n, K, _ = beams[i]
        check_result(cb.beam_result(rid), refs[i], K, n, len(p))
        assert cb.beam_result(rid) is None  # fetched once
    assert cb.status() == {"waiting": 0, "running": 0, "free_pages": free0}


def test_a_chunked_admission_carries_the_first_steps_values(gh, monkeypatch):
    """(the set-up of test_a_beam_request_with_a_long_prompt_is_admitted_in_chunks) the first generated position is the row the
    group takes over from the engine's own first beam step"""
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    monkeypatch.setenv("FTCF_BATCHER_PREFILL_CHUNK", "8")
    cfg, w, z = load_tiny()
    V = cfg["vocab_size"]
    op = gh.make_op(cfg, w)
    rng = np.random.RandomState(23)
    greedy, g_new = z["prompt_b"].tolist(), 14
    bp, b_new, K = rng.randint(3, V, size=21).tolist(), 7, 3
    ref = beam_alone(gh, op, bp, b_new, V, K)
    cb = ContinuousBatcher(op, max_batch=4, page_tokens=8, num_pages=40, max_seq_len=48)
    gid = cb.submit(greedy, g_new)
    per_step, bid, it = [], None, 0
    while it == 0 or cb.busy():
        if it == 1:
            bid = cb.submit_beam(bp, b_new, K, 0.0, 0.0, 1.0, 1.0, token_log_probs=True)
        per_step.append([rid == gid for rid, _, _ in cb.step()])
        it += 1
        assert it < 500
    assert per_step[1] == [True, True, True], "the prompt was admitted in chunks of 8, 8, 5"
    lp = check_result(cb.beam_result(bid), ref, K, b_new, len(bp))
    assert (lp[:, 0] != 0).all()
    np.testing.assert_allclose(lp[:, 0], ref[3][:, 0], **TOL)


def test_values_behind_the_end_token_are_zero_inside_the_batcher(gh):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg = dict(MID)
    w = random_model(cfg, seed=21)
    V = cfg["vocab_size"]
    prompt = np.random.RandomState(9).randint(3, V, size=19).tolist()
    K, n_new = 4, 16
    free = gh.run_op_beam(gh.make_op(cfg, w), np.asarray(prompt, np.int32)[None, :], [len(prompt)], n_new, V, K)
    cfg2 = dict(cfg, end_id=int(free["output_ids"][0, 0, len(prompt) + 5]))  # a token the best hypothesis emits mid-way
    op = gh.make_op(cfg2, w)
    ref = beam_alone(gh, op, prompt, n_new, V, K)
    assert (ref[1] < len(prompt) + n_new).any(), "the case really finishes beams early"
    cb = ContinuousBatcher(op, max_batch=6, page_tokens=8, num_pages=60, max_seq_len=64)
    rid = cb.submit_beam(prompt, n_new, K, token_log_probs=True)
    it = 0
    while cb.busy():
        cb.step()
        it += 1
        assert it < 500
    lp = check_result(cb.beam_result(rid), ref, K, n_new, len(prompt))
    seen = 0
    for k in range(K):
        ends = np.flatnonzero(ref[0][k, len(prompt):len(prompt) + n_new] == cfg2["end_id"])
        if ends.size:
            seen += 1
            assert lp[k, ends[0]] != 0, "the end token itself was read from a cell"
            assert (bits(lp[k, ends[0] + 1:]) == 0).all(), (k, lp[k])
    assert seen > 0


def test_the_edges_of_the_batchers_interface(gh):
    from fastertransformer4codefuse_amd import capi
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z = load_tiny()
    op = gh.make_op(cfg, w)
    L = capi.lib()
    prompt, n_new, K = z["prompt"].tolist(), 6, 3
    ids = np.ascontiguousarray(prompt, dtype=np.int32)

    def drain(cb):
        it = 0
        while cb.busy():
            cb.step()
            it += 1
            assert it < 500

    def fetch(cb, rid, with_lp):
        k, t = C.c_int(0), C.c_int(0)
        total = len(prompt) + n_new
        out, lens, cum = np.zeros((K, total), np.int32), np.zeros(K, np.int32), np.zeros(K, np.float32)
        lp = np.zeros((K, n_new), np.float32)
        rc = L.ftcf_batcher_beam_result_ex(cb._h, rid, out.ctypes.data, lens.ctypes.data, cum.ctypes.data, lp.ctypes.data if with_lp else None,
                                           out.size, C.byref(k), C.byref(t))
        return rc, (out, lens, cum, lp), (k.value, t.value)

    cb = ContinuousBatcher(op, max_batch=4, page_tokens=8, num_pages=40, max_seq_len=48)
    # without the flag: a 3-tuple, and the array is refused (the result stays parked for the plain fetch)
    plain = cb.submit_beam(prompt, n_new, K)
    drain(cb)
    rc, _, _ = fetch(cb, plain, True)
    assert rc == -1 and b"token_log_probs" in L.ftcf_last_error()  # FTCF_ERR_INVALID_ARG
    ref = cb.beam_result(plain)
    assert len(ref) == 3
    # a wrong struct_size is refused and nothing is queued
    o = capi.BeamOptions(struct_size=C.sizeof(capi.BeamOptions) - 4, beam_width=K, temperature=1.0, repetition_penalty=1.0)
    rid = C.c_long(-7)
    assert L.ftcf_batcher_submit_beam_opts(cb._h, ids.ctypes.data, ids.size, n_new, C.byref(o), C.byref(rid)) == -1
    assert b"struct_size" in L.ftcf_last_error() and rid.value == -7 and not cb.busy()
    # flag 0: submit_beam_ex
    o.struct_size = C.sizeof(capi.BeamOptions)
    capi.check(L.ftcf_batcher_submit_beam_opts(cb._h, ids.ctypes.data, ids.size, n_new, C.byref(o), C.byref(rid)))
    drain(cb)
    rc, got, (k, t) = fetch(cb, rid.value, False)  # (NULL is allowed)
    assert rc == 0 and (k, t) == (K, len(prompt) + n_new)
    for a, b in zip(got[:3], ref):
        assert a.tobytes() == b.tobytes()
    # flag 1 through the C entry points: the values of the Python path
    o.token_log_probs = 1
    capi.check(L.ftcf_batcher_submit_beam_opts(cb._h, ids.ctypes.data, ids.size, n_new, C.byref(o), C.byref(rid)))
    drain(cb)
    rc, got, _ = fetch(cb, rid.value, True)
    assert rc == 0 and got[0].tobytes() == ref[0].tobytes()
    py = cb.submit_beam(prompt, n_new, K, token_log_probs=True)
    drain(cb)
    res = cb.beam_result(py)
    assert len(res) == 4 and res[3].tobytes() == got[3].tobytes() and (res[3] != 0).any()
