"""-m gpu: per-token log-probabilities of the engine behind GptNeoXOp.forward -- output_log_probs of the generated tokens
(GptNeoX.cc:418, 967-987; stored where the sampling kernels add to cum_log_probs) and context_log_probs of the prompt tokens
(ParallelGpt.cc:403-470, the fused LM-head kernel here) -- on every decode path, with tensor parallelism, and the refusals."""
import threading

import numpy as np
import pytest

from tests.helpers import load_tiny, random_model, shard_weights

pytestmark = pytest.mark.gpu

MID = dict(head_num=8, size_per_head=128, inter_size=4096, num_layer=2, vocab_size=2048, rotary_dim=32, start_id=0, end_id=2)


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


def run(op, ids, lens, out, V, debug=True, olp=True, clp=False, cum=1, beam=1, **kw):
    """op.forward with the new outputs; returns a dict of numpy arrays (row 0 of the beam axis)."""
    import torch
    ids_t = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).cuda()
    lens_t = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).cuda()
    B = ids_t.shape[0]
    dbg = torch.zeros((out, B * beam, V), dtype=torch.float32, device="cuda") if debug else None
    t = lambda v, dt: None if v is None else torch.tensor(v if isinstance(v, (list, tuple)) else [v], dtype=dt)
    outs = op.forward(ids_t, lens_t, out, beam, t(kw.get("top_k"), torch.int32), t(kw.get("top_p"), torch.float32), None,
                      t(kw.get("temperature"), torch.float32), None, t(kw.get("repetition_penalty"), torch.float32),
                      t(kw.get("random_seed"), torch.int64), None, None, cum, None, _debug_logits=dbg,
                      return_output_log_probs=olp or None, return_context_log_probs=clp or None)
    torch.cuda.synchronize()
    res = {"n_outputs": len(outs), "output_ids": outs[0][:, 0, :].cpu().numpy(), "sequence_lengths": outs[1][:, 0].cpu().numpy()}
    i = 2
    if cum:
        res["cum_log_probs"] = outs[i][:, 0].cpu().numpy()
        i += 1
    if olp:
        res["output_log_probs"] = outs[i][:, 0, :].cpu().numpy()
        i += 1
    if clp:
        res["context_log_probs"] = outs[i].cpu().numpy()
    if debug:
        res["logits"] = dbg.cpu().numpy()
    return res


def seq_sum(v):
    s = np.float32(0.0)
    for x in v:
        s = np.float32(s + np.float32(x))
    return s


def log_softmax64(x):
    x = x.astype(np.float64)
    m = x.max()
    return x - m - np.log(np.exp(x - m).sum())


def check_output_log_probs(r, ref, lens, out, temperature=None, unpenalised=True):
    """r: the run with output_log_probs; ref: the same request with return_cum_log_probs = 1 only."""
    assert r["output_ids"].tolist() == ref["output_ids"].tolist()
    assert r["sequence_lengths"].tolist() == ref["sequence_lengths"].tolist()
    B = len(lens)
    S = r["output_ids"].shape[1] - out
    for b in range(B):
        lp = r["output_log_probs"][b]
        assert seq_sum(lp).tobytes() == np.float32(r["cum_log_probs"][b]).tobytes(), (b, seq_sum(lp), r["cum_log_probs"][b])
        assert r["cum_log_probs"][b].tobytes() == ref["cum_log_probs"][b].tobytes()
        n_gen = int(r["sequence_lengths"][b]) - S  # (sequence_lengths counts from max_input_len, GptNeoX.cc:1090-1181)
        assert 1 <= n_gen <= out
        assert np.all(lp[n_gen:] == 0.0), (b, n_gen, lp)  # steps after the row finished
        assert np.all(lp[:n_gen] <= 0.0)
        if unpenalised and "logits" in r:
            T = 1.0 if temperature is None else temperature
            # generated token i sits at output position lens[b] + i (invokeGatherTree removes the padding) and was produced by
            # the loop's step i, whose logits are debug_logits[i]
            for i in range(n_gen):
                tok = int(r["output_ids"][b, lens[b] + i])
                want = log_softmax64(r["logits"][i, b] / T)[tok]
                assert abs(lp[i] - want) <= 1e-4, (b, i, lp[i], want)


def _batch(cfg, B, S, seed):
    rng = np.random.RandomState(seed)
    lens = rng.randint(max(1, S // 2), S + 1, size=B).astype(np.int32)
    lens[0] = S
    ids = np.full((B, S), cfg["end_id"], dtype=np.int32)
    for b in range(B):
        ids[b, :lens[b]] = rng.randint(3, cfg["vocab_size"], size=lens[b])
    return ids, lens


CASES = {
    # name: (model, B, kwargs, env, expected decode_path, unpenalised, temperature)
    "persist1_lm_head_greedy": ("tiny", 1, dict(top_k=1), {}, 1, True, None),
    "persist2_lm_head_greedy": ("tiny", 2, dict(top_k=1), {}, 1, True, None),
    "persist1_k_sample": ("tiny", 1, dict(top_k=1), {"FTCF_GREEDY_FUSED": "0"}, 1, True, None),
    "rows3_greedy_decode": ("mid", 3, dict(top_k=1), {}, 3, True, None),
    "rows16_greedy_decode": ("mid", 16, dict(top_k=1), {}, 3, True, None),
    "general5": ("mid", 5, dict(top_k=1), {"FTCF_ROWS": "0"}, 2, True, None),
    "launches1": ("tiny", 1, dict(top_k=1), {"FTCF_PERSIST": "0"}, 0, True, None),
    "topk50_decode": ("mid", 4, dict(top_k=50, random_seed=11), {}, 3, True, None),
    "topp": ("mid", 3, dict(top_p=0.9, random_seed=5), {}, 3, True, None),
    "topk_temperature": ("tiny", 2, dict(top_k=4, temperature=0.7, random_seed=3), {}, 1, True, 0.7),
    "topp_temperature": ("mid", 5, dict(top_p=0.8, temperature=1.3, random_seed=9), {"FTCF_ROWS": "0"}, 2, True, 1.3),
    "repetition": ("mid", 3, dict(top_k=1, repetition_penalty=1.3), {}, 3, False, None),
}


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_output_log_probs_on_every_decode_path(gh, monkeypatch, case, graph):
    """Sequential fp32 sum == cum_log_probs bit for bit, tokens == the return_cum_log_probs = 1 run, values == float64
    log_softmax(logits / T)[token] where nothing but the temperature touched the logits.  `graph`: no debug tap, so the token
    step is captured once and replayed (the buffer is indexed by the device-side step)."""
    model, B, kw, env, path, unpenalised, T = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if model == "tiny":
        cfg, w, z = load_tiny()
        ids = np.full((B, 16), cfg["end_id"], dtype=np.int32)
        ids[0] = z["prompt"]
        lens = np.array([16, 11][:B], dtype=np.int32)
        if B > 1:
            ids[1, :11] = z["prompt_b"]
    else:
        cfg = MID
        w = random_model(cfg, seed=B, std=0.04)
        ids, lens = _batch(cfg, B, 21, seed=B)
    out = 10
    V = cfg["vocab_size"]
    op = gh.make_op(cfg, w)
    ref = run(op, ids, lens, out, V, debug=not graph, olp=False, **kw)
    r = run(op, ids, lens, out, V, debug=not graph, olp=True, **kw)
    assert op.stats()["decode_path"] == path
    check_output_log_probs(r, ref, lens, out, temperature=T, unpenalised=unpenalised and not graph)
    if graph:  # the captured form holds the same values as the eager one
        e = run(op, ids, lens, out, V, debug=True, olp=True, **kw)
        assert e["output_ids"].tolist() == r["output_ids"].tolist()
        np.testing.assert_array_equal(e["output_log_probs"], r["output_log_probs"])
    # without cum_log_probs the tokens are still those of the return_cum_log_probs = 1 request
    r2 = run(op, ids, lens, out, V, debug=False, olp=True, cum=0, **kw)
    assert r2["output_ids"].tolist() == ref["output_ids"].tolist()
    np.testing.assert_array_equal(r2["output_log_probs"], r["output_log_probs"])


def test_rows_that_finish_early_hold_zero(gh):
    cfg, w, z = load_tiny()
    ids = np.full((2, 16), cfg["end_id"], dtype=np.int32)
    ids[0] = z["prompt"]
    ids[1, :11] = z["prompt_b"]
    lens = np.array([16, 11], dtype=np.int32)
    free = run(gh.make_op(cfg, w), ids, lens, 8, cfg["vocab_size"], top_k=1)
    end = int(free["output_ids"][0, 16 + 2])  # row 0's third token becomes the end id
    cfg2 = dict(cfg, end_id=end)
    r = run(gh.make_op(cfg2, w), ids, lens, 8, cfg["vocab_size"], top_k=1)
    assert int(r["sequence_lengths"][0]) == 16 + 3
    assert np.all(r["output_log_probs"][0, 3:] == 0.0) and np.all(r["output_log_probs"][0, :3] < 0.0)
    np.testing.assert_array_equal(r["output_log_probs"][0, :3], free["output_log_probs"][0, :3])
    assert seq_sum(r["output_log_probs"][0]).tobytes() == np.float32(r["cum_log_probs"][0]).tobytes()


def test_context_log_probs_match_hf_golden(gh):
    """tests/golden/tiny_gptneox_fp32.npz: HF's fp32 logits of prompt + hf_tokens -- log P(hf_tokens[i]) is context position
    len(prompt) + i.  Bound: the fp16 engine's logit distance from HF (4e-3 of max|logit|, tests/test_gpu_engine.py) on the
    target logit and on the log-sum-exp."""
    cfg, w, z = load_tiny()
    op = gh.make_op(cfg, w)
    V = cfg["vocab_size"]
    for prompt, toks, hfl in ((z["prompt"], z["hf_tokens"], z["hf_logits"]), (z["prompt_1"], z["hf_tokens_1"], z["hf_logits_1"])):
        seq = np.concatenate([prompt, toks]).astype(np.int32)[None, :]
        r = run(op, seq, [seq.shape[1]], 2, V, olp=False, clp=True, top_k=1)
        c = r["context_log_probs"][0]
        P = len(prompt)
        want = np.array([log_softmax64(hfl[i])[int(toks[i])] for i in range(len(toks))])
        tol = 2 * 4e-3 * np.abs(hfl).max()
        np.testing.assert_allclose(c[P:P + len(toks)], want, atol=tol, rtol=0)
        assert c[0] == 0.0
        assert np.all(c[1:] < 0.0)


def test_context_log_probs_padding_and_ragged_rows(gh):
    """Ragged rows equal each row run alone (tokens exact, values within rounding); padding and position 0 hold 0; a one-token
    prompt gives zeros."""
    cfg = MID
    w = random_model(cfg, seed=1, std=0.04)
    V = cfg["vocab_size"]
    op = gh.make_op(cfg, w)
    ids, lens = _batch(cfg, 4, 23, seed=4)
    r = run(op, ids, lens, 6, V, olp=True, clp=True, top_k=1)
    for b in range(4):
        c = r["context_log_probs"][b]
        assert c[0] == 0.0 and np.all(c[lens[b]:] == 0.0) and np.all(c[1:lens[b]] < 0.0)
        a = run(op, ids[b:b + 1, :lens[b]], lens[b:b + 1], 6, V, olp=True, clp=True, top_k=1)
        assert a["output_ids"][0, :lens[b] + 6].tolist() == r["output_ids"][b, :lens[b] + 6].tolist()
        # (one row runs the persistent decode kernel, the batch the rows kernel: fp16 rounding of different GEMM orders)
        np.testing.assert_allclose(a["context_log_probs"][0], c[:lens[b]], atol=2e-3, rtol=2e-3)
        np.testing.assert_allclose(a["output_log_probs"][0], r["output_log_probs"][b], atol=2e-3, rtol=2e-2)
    one = run(op, ids[:2, :1], np.array([1, 1], dtype=np.int32), 4, V, olp=False, clp=True, top_k=1)
    assert np.all(one["context_log_probs"] == 0.0)


def test_context_log_probs_of_a_continuation_match_its_output_log_probs(gh):
    """Prefill vs decode: scoring prompt + the greedy continuation gives the continuation's output_log_probs."""
    cfg, w, z = load_tiny()
    V = cfg["vocab_size"]
    op = gh.make_op(cfg, w)
    g = run(op, z["prompt"][None, :], [16], 8, V, top_k=1)
    seq = g["output_ids"][:, :24]
    c = run(op, seq, [24], 1, V, olp=False, clp=True, top_k=1)
    np.testing.assert_allclose(c["context_log_probs"][0, 16:24], g["output_log_probs"][0], atol=5e-3, rtol=0)


def test_beams_refuse_output_log_probs_and_score_the_prompt_once(gh):
    from fastertransformer4codefuse_amd.capi import FtcfError
    cfg, w, z = load_tiny()
    V = cfg["vocab_size"]
    op = gh.make_op(cfg, w)
    ids = np.full((2, 16), cfg["end_id"], dtype=np.int32)
    ids[0] = z["prompt"]
    ids[1, :11] = z["prompt_b"]
    lens = np.array([16, 11], dtype=np.int32)
    with pytest.raises(FtcfError):
        run(op, ids, lens, 4, V, debug=False, olp=True, beam=3)
    b1 = run(op, ids, lens, 4, V, debug=False, olp=False, clp=True, top_k=1)
    b3 = run(op, ids, lens, 4, V, debug=False, olp=False, clp=True, beam=3)
    np.testing.assert_allclose(b3["context_log_probs"], b1["context_log_probs"], atol=1e-5, rtol=0)


def test_fp32_engine_refuses_context_log_probs(gh):
    import torch
    from fastertransformer4codefuse_amd.capi import FtcfError
    cfg, w, z = load_tiny()
    op = gh.make_op(cfg, w, dtype=torch.float32)
    with pytest.raises(FtcfError):
        run(op, z["prompt"][None, :], [16], 4, cfg["vocab_size"], debug=False, olp=False, clp=True, top_k=1)
    r = run(op, z["prompt"][None, :], [16], 4, cfg["vocab_size"], olp=True, top_k=1)  # output_log_probs work there
    check_output_log_probs(r, run(op, z["prompt"][None, :], [16], 4, cfg["vocab_size"], olp=False, top_k=1), [16], 4)


def test_defaults_return_what_they_returned(gh):
    cfg, w, z = load_tiny()
    op = gh.make_op(cfg, w)
    V = cfg["vocab_size"]
    a = run(op, z["prompt"][None, :], [16], 8, V, debug=False, olp=False, cum=0, top_k=1)
    assert a["n_outputs"] == 2
    b = run(op, z["prompt"][None, :], [16], 8, V, debug=False, olp=False, cum=1, top_k=1)
    assert b["n_outputs"] == 3
    c = run(op, z["prompt"][None, :], [16], 8, V, debug=False, olp=True, clp=True, cum=1, top_k=1)
    assert c["n_outputs"] == 5
    assert a["output_ids"].tolist() == b["output_ids"].tolist() == c["output_ids"].tolist()
    assert b["cum_log_probs"].tobytes() == c["cum_log_probs"].tobytes()


@pytest.mark.parametrize("tp", [2, 4])
def test_tensor_parallel_ranks_are_identical_and_match_tp1(gh, tp):
    """Local-group ranks (one process, one device, tests/test_gpu_tp_local.py): every rank scores the whole vocabulary
    from the all-reduced hidden rows with the replicated head -- identical bits on every rank, TP 1 within rounding."""
    from fastertransformer4codefuse_amd.gptneox_op import LocalTensorParallelGroup
    cfg, w, z = load_tiny()
    V = cfg["vocab_size"]
    ids = np.full((2, 16), cfg["end_id"], dtype=np.int32)
    ids[0] = z["prompt"]
    ids[1, :11] = z["prompt_b"]
    lens = np.array([16, 11], dtype=np.int32)
    for rows in (1, 2):
        one = run(gh.make_op(cfg, w), ids[:rows], lens[:rows], 8, V, debug=False, clp=True, top_k=1)
        group = LocalTensorParallelGroup()
        res, err = [None] * tp, []

        def worker(r):
            try:
                op = gh.make_op(cfg, shard_weights(cfg, w, tp, r), tp=tp, rank=r, comm=group)
                res[r] = run(op, ids[:rows], lens[:rows], 8, V, debug=False, clp=True, top_k=1)
            except BaseException as e:  # noqa: BLE001
                err.append((r, e))

        ths = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(tp)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(timeout=300)
        assert not err, err
        assert all(x is not None for x in res)
        for r in range(1, tp):
            assert res[r]["output_ids"].tolist() == res[0]["output_ids"].tolist()
            assert res[r]["output_log_probs"].tobytes() == res[0]["output_log_probs"].tobytes()
            assert res[r]["context_log_probs"].tobytes() == res[0]["context_log_probs"].tobytes()
        assert res[0]["output_ids"].tolist() == one["output_ids"].tolist()
        # (the sharded GEMMs and the all-reduce round differently from TP 1: relative to the value, as the engine tests' logits)
        np.testing.assert_allclose(res[0]["output_log_probs"], one["output_log_probs"], atol=5e-3, rtol=1e-2)
        np.testing.assert_allclose(res[0]["context_log_probs"], one["context_log_probs"], atol=5e-3, rtol=2e-3)
        for b in range(rows):
            assert seq_sum(res[0]["output_log_probs"][b]).tobytes() == np.float32(res[0]["cum_log_probs"][b]).tobytes()
