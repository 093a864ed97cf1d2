"""-m gpu: top_logprobs through GptNeoXOp.forward on the tiny golden model -- greedy and top_k = 4 with temperature and
repetition penalty, one row and three ragged rows of which one ends early, against a float64 log-softmax of the debug_logits
taps processed as tests/top_logprobs_reference.py processes a row (fp32 stores of the temperature product and of the penalty,
then float64); tokens, cum_log_probs and output_log_probs are those of the request without it; the captured token loop returns
the bits of the eager one; the refusals; a speculative request runs unspeculated; both ranks of a TP = 2 local group return
the same pairs."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import decode_reference as ref
from tests import top_logprobs_reference as tlp
from tests.decode_cases import LP_TOL
from tests.helpers import load_tiny, shard_weights

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
OUT = 8


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


def run(op, ids, lens, out, V, N=0, debug=True, beam=1, olp=True, cum=1, **kw):
    import torch
    ids_t = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).cuda()
    lens_t = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).cuda()
    B = ids_t.shape[0]
    dbg = torch.zeros((out, B * beam, V), dtype=torch.float32, device="cuda") if debug else None
    t = lambda v, dt: None if v is None else torch.tensor(v if isinstance(v, (list, tuple)) else [v], dtype=dt)
    outs = op.forward(ids_t, lens_t, out, beam, t(kw.get("top_k"), torch.int32), None, None, t(kw.get("temperature"), torch.float32),
                      None, t(kw.get("repetition_penalty"), torch.float32), t(kw.get("random_seed"), torch.int64), None, None, cum, None,
                      _debug_logits=dbg, return_output_log_probs=olp or None, speculative_tokens=kw.get("speculative_tokens"),
                      top_logprobs=N or None)
    torch.cuda.synchronize()
    assert len(outs) == 2 + cum + (1 if olp else 0) + (2 if N else 0)
    res = dict(output_ids=outs[0][:, 0, :].cpu().numpy(), sequence_lengths=outs[1][:, 0].cpu().numpy())
    if cum:
        res["cum_log_probs"] = outs[2][:, 0].cpu().numpy()
    if olp:
        res["output_log_probs"] = outs[2 + cum][:, 0, :].cpu().numpy()
    if N:  # appended after the other optional outputs
        assert tuple(outs[-2].shape) == (B, beam, out, N) and outs[-2].dtype == torch.int32 and outs[-1].dtype == torch.float32
        res["top_ids"], res["top_values"] = outs[-2][:, 0].cpu().numpy(), outs[-1][:, 0].cpu().numpy()
    if debug:
        res["logits"] = dbg.cpu().numpy()
    return res


def batch(cfg, z, B):
    ids = np.full((B, 16), cfg["end_id"], dtype=np.int32)
    ids[0] = z["prompt"]
    lens = [16]
    if B > 1:
        ids[1, :11] = z["prompt_b"]
        ids[2, :7] = np.random.RandomState(5).randint(3, cfg["vocab_size"], size=7)
        lens += [11, 7]
    return ids, np.array(lens, dtype=np.int32)


def processed(logits, history, temperature, repetition_penalty):
    """one row of debug_logits as k_decode_prep leaves it (tests/decode_reference.py sampling_step, step 1)"""
    l = logits.astype(np.float64)
    if temperature is not None:
        l = ref.stored(l * ref.stored(1.0 / ref.stored(np.float32(temperature) + ref.stored(1e-6))))
    if repetition_penalty is not None:
        pen = float(np.float32(repetition_penalty))
        before = l.copy()
        for t in set(history):
            l[t] = ref.stored(before[t] * pen) if before[t] < 0.0 else ref.stored(before[t] / pen)
    return l


SAMPLING = {"greedy": dict(top_k=1), "top_k4": dict(top_k=4, temperature=0.7, repetition_penalty=1.2, random_seed=3)}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("sampling", sorted(SAMPLING))
def test_pairs_match_the_float64_log_softmax_of_the_taps(gh, sampling, B, monkeypatch):
    kw, N = SAMPLING[sampling], 5
    cfg, w, z = load_tiny()
    V = cfg["vocab_size"]
    ids, lens = batch(cfg, z, B)
    free = run(gh.make_op(cfg, w), ids, lens, OUT, V, **kw)
    cfg = dict(cfg, end_id=int(free["output_ids"][0, 16 + 2]))  # row 0's third token ends it
    op = gh.make_op(cfg, w)
    base = run(op, ids, lens, OUT, V, **kw)
    r = run(op, ids, lens, OUT, V, N=N, **kw)
    # tokens are those of the request without it; its log-probabilities are those of the general decode form, which a request
    # with top_logprobs takes (the one-launch greedy / top-k steps add the slices' soft-max statistics in another order: a last bit)
    for key in ("output_ids", "sequence_lengths"):
        assert r[key].tobytes() == base[key].tobytes(), key
    for key in ("cum_log_probs", "output_log_probs"):
        np.testing.assert_allclose(r[key], base[key], err_msg=key, **LP_TOL)
    monkeypatch.setenv("FTCF_GREEDY_FUSED", "0")
    monkeypatch.setenv("FTCF_TOPK_FUSED", "0")
    general = run(op, ids, lens, OUT, V, **kw)
    monkeypatch.delenv("FTCF_GREEDY_FUSED")
    monkeypatch.delenv("FTCF_TOPK_FUSED")
    for key in ("output_ids", "sequence_lengths", "cum_log_probs", "output_log_probs"):
        assert r[key].tobytes() == general[key].tobytes(), key
    assert op.stats()["decode_steps"] >= 1
    n_gen = r["sequence_lengths"] - 16
    assert 1 <= n_gen[0] <= 3, "row 0 ends early"
    for b in range(B):
        toks = r["output_ids"][b, lens[b]:lens[b] + n_gen[b]].tolist()
        for i in range(OUT):
            gi, gl = r["top_ids"][b, i], r["top_values"][b, i]
            if i >= n_gen[b]:  # the row had finished before the step
                assert (gi == -1).all() and (gl == 0.0).all() and not np.signbit(gl).any(), (b, i, gi, gl)
                continue
            hist = ids[b, :lens[b]].tolist() + toks[:i]
            want = tlp.top_n(processed(r["logits"][i, b], hist, kw.get("temperature"), kw.get("repetition_penalty")), N)
            print(sampling, B, "row", b, "step", i, gi.tolist(), want["ids"].tolist(), gl.tolist())
            np.testing.assert_array_equal(gi, want["ids"], err_msg=f"row {b} step {i}")
            np.testing.assert_allclose(gl, want["log_probs"], err_msg=f"row {b} step {i}", **LP_TOL)
            if kw["top_k"] == 1:
                assert gi[0] == toks[i]
            assert toks[i] in gi.tolist()  # top_k <= N
            np.testing.assert_allclose(gl[gi.tolist().index(toks[i])], r["output_log_probs"][b, i], **LP_TOL)
    # the captured token loop (no debug tap) indexes the buffers by the device-side step: the same bits
    g = run(op, ids, lens, OUT, V, N=N, debug=False, **kw)
    assert g["output_ids"].tobytes() == r["output_ids"].tobytes()
    assert g["top_ids"].tobytes() == r["top_ids"].tobytes() and g["top_values"].tobytes() == r["top_values"].tobytes()


def test_refusals(gh):
    import torch
    from fastertransformer4codefuse_amd import capi
    cfg, w, z = load_tiny()
    V = cfg["vocab_size"]
    op = gh.make_op(cfg, w)
    ids, lens = batch(cfg, z, 1)
    with pytest.raises(capi.FtcfError, match="top_logprobs is not supported with beam_width"):
        run(op, ids, lens, 4, V, N=5, debug=False, beam=2, olp=False)
    with pytest.raises(capi.FtcfError, match="top_logprobs"):
        run(op, ids, lens, 4, V, N=21, debug=False, top_k=1)
    # a NULL buffer, through the C ABI
    ids_t, lens_t = torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda()
    out_t, seq_t = torch.zeros((1, 1, 20), dtype=torch.int32, device="cuda"), torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    top = torch.zeros((1, 1, 4, 5), dtype=torch.int32, device="cuda")
    a = capi.ForwardArgs()
    a.input_ids, a.input_lengths, a.output_ids, a.sequence_lengths = ids_t.data_ptr(), lens_t.data_ptr(), out_t.data_ptr(), seq_t.data_ptr()
    a.batch_size, a.max_input_len, a.output_len, a.beam_width = 1, 16, 4, 1
    a.top_logprobs, a.top_logprob_ids = 5, top.data_ptr()
    assert capi.lib().ftcf_gptneox_forward(op._h, C.byref(a)) == -1
    assert b"top_logprob" in capi.lib().ftcf_last_error()
    r = run(op, ids, lens, 4, V, N=1, debug=False, top_k=1)  # the engine goes on
    assert r["top_ids"][0, :, 0].tolist() == r["output_ids"][0, 16:20].tolist()


def test_a_speculative_request_runs_unspeculated(gh):
    cfg, w, z = load_tiny()
    V = cfg["vocab_size"]
    op = gh.make_op(cfg, w)
    ids, lens = batch(cfg, z, 1)
    lean = dict(debug=False, olp=False, cum=0, top_k=1)
    run(op, ids, lens, OUT, V, speculative_tokens=4, **lean)
    assert op.stats()["spec_active"] == 1, "the request without top_logprobs speculates"
    plain = run(op, ids, lens, OUT, V, N=5, **lean)
    spec = run(op, ids, lens, OUT, V, N=5, speculative_tokens=4, **lean)
    assert op.stats()["spec_active"] == 0 and op.stats()["spec_steps"] == 0
    for key in ("output_ids", "top_ids", "top_values"):
        assert spec[key].tobytes() == plain[key].tobytes(), key


def test_both_ranks_of_a_local_group_return_the_same_pairs(gh):
    from fastertransformer4codefuse_amd.gptneox_op import LocalTensorParallelGroup
    cfg, w, z = load_tiny()
    V = cfg["vocab_size"]
    ids, lens = batch(cfg, z, 3)
    tp, N = 2, 5
    one = run(gh.make_op(cfg, w), ids, lens, OUT, V, N=N, debug=False, top_k=1)
    group = LocalTensorParallelGroup()
    res, err = [None] * tp, []

    def worker(r):
        try:
            op = gh.make_op(cfg, shard_weights(cfg, w, tp, r), tp=tp, rank=r, comm=group)
            res[r] = run(op, ids, lens, OUT, V, N=N, debug=False, top_k=1)
        except BaseException as e:  # noqa: BLE001
            err.append((r, e))

    ths = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(tp)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=300)
    assert not err, err
    assert all(x is not None for x in res)
    for key in ("output_ids", "top_ids", "top_values"):
        assert res[1][key].tobytes() == res[0][key].tobytes(), key
    assert res[0]["output_ids"].tolist() == one["output_ids"].tolist()
    assert (res[0]["top_ids"][:, :, 0] == one["top_ids"][:, :, 0]).all()  # the emitted tokens
    # (the sharded GEMMs and the all-reduce round differently from TP 1: the bound of tests/test_gpu_log_probs.py)
    np.testing.assert_allclose(np.sort(res[0]["top_values"], axis=-1), np.sort(one["top_values"], axis=-1), atol=5e-3, rtol=1e-2)
