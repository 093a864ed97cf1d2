"""Helpers for the -m gpu parity tests: build engine inputs from the reference weight-list contract."""
import ctypes as C

import numpy as np
import torch

from fastertransformer4codefuse_amd import capi
from fastertransformer4codefuse_amd.gptneox_op import GptNeoXOp, symmetric_quantize_last_axis_of_batched_matrix_int8


def dev(a, dtype=torch.float16):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def make_op(cfg, w, int8_mode=0, tp=1, rank=0, comm=None, use_gptj_residual=True, dtype=torch.float16, op_class=None):
    """cfg: dict like tests.helpers ; w: reference-order list of float32 numpy arrays -- the full TP=1 layout, or with
    tp > 1 the shard of `rank` (tests.helpers.shard_weights)."""
    L = cfg["num_layer"]
    H = cfg["head_num"] * cfg["size_per_head"]
    I = cfg["inter_size"]
    shapes = {2: (H, 3 * H // tp), 4: (H // tp, H), 6: (H, I // tp), 8: (I // tp, H)}
    weights, int8_w, scales = [], [None] * (4 * L), [None] * (4 * L)
    for g in range(12):
        for l in range(L):
            a = w[g * L + l]
            if g in shapes and a.size:
                a = a.reshape(shapes[g])
                if int8_mode:
                    q, s = symmetric_quantize_last_axis_of_batched_matrix_int8(torch.from_numpy(a).half().contiguous())
                    qi = {2: 0, 4: 1, 6: 2, 8: 3}[g]
                    int8_w[qi * L + l] = q.cuda()
                    scales[qi * L + l] = s.cuda()
                    weights.append(torch.empty(0, dtype=dtype, device="cuda"))
                    continue
            weights.append(dev(a, dtype) if a.size else torch.empty(0, dtype=dtype, device="cuda"))
    V = cfg["vocab_size"]
    weights += [dev(w[12 * L].reshape(V, H), dtype), dev(w[12 * L + 1], dtype), dev(w[12 * L + 2], dtype),
                dev(w[12 * L + 3].reshape(V, H), dtype)]
    if not int8_mode:
        int8_w, scales = [], []
    # (op_class: the compiled libth_gptneox.GptNeoXOp instead of the ctypes one -- tests/test_gpu_th_modules.py)
    op = (op_class or GptNeoXOp)(comm, rank, cfg["head_num"], cfg["size_per_head"], I, L, V, cfg["rotary_dim"], cfg.get("start_id", 0),
                   cfg["end_id"], tp, 1, int8_mode, 1024, use_gptj_residual, weights, int8_w, scales)
    return op


def run_op(op, input_ids, input_lengths, out_len, V, return_logits=True, **kw):
    ids = torch.from_numpy(np.ascontiguousarray(input_ids, dtype=np.int32)).cuda()
    lens = torch.from_numpy(np.ascontiguousarray(input_lengths, dtype=np.int32)).cuda()
    B = ids.shape[0]
    dbg = torch.zeros((out_len, B, V), dtype=torch.float32, device="cuda") if return_logits else None
    t = lambda v, dt: None if v is None else torch.tensor(v if isinstance(v, (list, tuple)) else [v], dtype=dt)
    outs = op.forward(ids, lens, out_len, 1, t(kw.get("top_k"), torch.int32), t(kw.get("top_p"), torch.float32), None,
                      t(kw.get("temperature"), torch.float32), None, t(kw.get("repetition_penalty"), torch.float32),
                      t(kw.get("random_seed"), torch.int64),
                      None if kw.get("stop_words") is None else torch.from_numpy(
                          np.ascontiguousarray(kw["stop_words"], dtype=np.int32)).cuda(),
                      None if kw.get("optional_last_tokens") is None else torch.from_numpy(
                          np.ascontiguousarray(kw["optional_last_tokens"], dtype=np.int32)).cuda(),
                      kw.get("return_cum_log_probs", 1), kw.get("callback"), _debug_logits=dbg)
    torch.cuda.synchronize()
    res = {"output_ids": outs[0][:, 0, :].cpu().numpy(), "sequence_lengths": outs[1][:, 0].cpu().numpy()}
    if len(outs) > 2:
        res["cum_log_probs"] = outs[2][:, 0].cpu().numpy()
    if return_logits:
        res["logits"] = dbg.cpu().numpy()
    return res


def run_op_beam(op, input_ids, input_lengths, out_len, V, K, return_logits=False, **kw):
    """Beam search through GptNeoXOp.forward: output_ids [B, K, total], sequence_lengths / cum_log_probs [B, K]."""
    ids = torch.from_numpy(np.ascontiguousarray(input_ids, dtype=np.int32)).cuda()
    lens = torch.from_numpy(np.ascontiguousarray(input_lengths, dtype=np.int32)).cuda()
    B = ids.shape[0]
    dbg = torch.zeros((out_len, B * K, V), dtype=torch.float32, device="cuda") if return_logits else None
    t = lambda v, dt: None if v is None else torch.tensor(v if isinstance(v, (list, tuple)) else [v], dtype=dt)
    outs = op.forward(ids, lens, out_len, K, None, None, t(kw.get("beam_search_diversity_rate"), torch.float32),
                      t(kw.get("temperature"), torch.float32), t(kw.get("len_penalty"), torch.float32),
                      t(kw.get("repetition_penalty"), torch.float32), None,
                      None if kw.get("stop_words") is None else torch.from_numpy(
                          np.ascontiguousarray(kw["stop_words"], dtype=np.int32)).cuda(),
                      None if kw.get("optional_last_tokens") is None else torch.from_numpy(
                          np.ascontiguousarray(kw["optional_last_tokens"], dtype=np.int32)).cuda(),
                      1, kw.get("callback"), _debug_logits=dbg)
    torch.cuda.synchronize()
    res = {"output_ids": outs[0].cpu().numpy(), "sequence_lengths": outs[1].cpu().numpy(),
           "cum_log_probs": outs[2].cpu().numpy()}
    if return_logits:
        res["logits"] = dbg.cpu().numpy()
    return res


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------
# Tensor-parallel shards of a model in bench.synth_weights' int8 form ((args, weights, int8_w, scales)), shared by the
# full-size tests.  The int8 matrices are the engine's tiled images ([N/16][K/64][1 KiB] tiles): a column range is a range of
# the first axis, a k range a range of the second.
# ---------------------------------------------------------------------------------------------------------------------
def _run(op, ids, out, V, lens=None):
    B, S = ids.shape
    if lens is None:
        lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    dbg = torch.zeros((out, B, V), dtype=torch.float32, device="cuda")
    o = op.forward(ids, lens, out, 1, torch.tensor([1], dtype=torch.int32), _debug_logits=dbg)
    torch.cuda.synchronize()
    return o[0][:, 0].cpu().numpy(), dbg.cpu().numpy()


def _shard(full, tp, r):
    a, weights, int8_w, scales = full
    L, H, I = a.layers, a.heads * a.head_dim, a.inter
    hl, il = H // tp, I // tp

    def cols(t, N, lo, hi):  # tiled [N/16][K/64][1 KiB]: a column range is a range of the first axis
        return t.view(N // 16, -1)[lo // 16:hi // 16]

    def rows(t, N, K, lo, hi):  # a k range is a range of the second axis
        return t.view(N // 16, K // 64, 1024)[:, lo // 64:hi // 64, :].contiguous().view(-1)

    w = list(weights)
    q8, sc = list(int8_w), list(scales)
    for l in range(L):
        w[3 * L + l] = torch.cat([weights[3 * L + l].view(3, H)[p, r * hl:(r + 1) * hl] for p in range(3)]).contiguous()
        w[7 * L + l] = weights[7 * L + l][r * il:(r + 1) * il].contiguous()
        w[9 * L + l] = (weights[9 * L + l].float() / tp).half()  # row-split GEMM biases are divided by TP (the converter)
        q8[0 * L + l] = torch.cat([cols(int8_w[l], 3 * H, p * H + r * hl, p * H + (r + 1) * hl) for p in range(3)]
                                  ).contiguous().view(-1)
        sc[0 * L + l] = torch.cat([scales[l].view(3, H)[p, r * hl:(r + 1) * hl] for p in range(3)]).contiguous()
        q8[1 * L + l] = rows(int8_w[L + l], H, H, r * hl, (r + 1) * hl)
        q8[2 * L + l] = cols(int8_w[2 * L + l], I, r * il, (r + 1) * il).contiguous().view(-1)
        sc[2 * L + l] = scales[2 * L + l][r * il:(r + 1) * il].contiguous()
        q8[3 * L + l] = rows(int8_w[3 * L + l], H, I, r * il, (r + 1) * il)
    return w, q8, sc


def _periodic(full, n):
    """`full` with an embedding table and an LM head that repeat with period V / n (copies of their first slice): every
    vocabulary slice of a TP = n (or n / 2, n / 4, ...) job is then the same, and a token and its copies embed alike."""
    a, weights, int8_w, scales = full
    L, V = a.layers, a.vocab
    w = list(weights)
    for i in (12 * L, 12 * L + 3):  # pre-decoder embedding table, LM head
        w[i] = weights[i].view(n, V // n, -1)[:1].expand(n, -1, -1).reshape(weights[i].shape).contiguous()
    return a, w, int8_w, scales


def _tile(shard, tp, r):
    """A TP = 1 model whose every rank-r' shard (r' < tp) equals `shard`, the rank-r shard of (a, *shard): every head group,
    FFN column block and vocabulary slice is a copy of rank r's.  Built on the tiled int8 images (no requantisation):
    column-split matrices (QKV per q / k / v plane, FFN1) and their scales and biases are repeated along the columns,
    row-split matrices (out-proj, FFN2) along K with their scales unchanged and their biases x tp (the shard holds bias / TP);
    the LM head repeats slice r and the embedding table its first slice (period V / tp).  What a TP = tp job whose ranks all
    hold `shard` computes, up to summation order -- with fake peers (FTCF_FAKE_TP) one rank computes exactly that."""
    a, weights, int8_w, scales = shard
    L, H, I, V = a.layers, a.heads * a.head_dim, a.inter, a.vocab
    hl, il, vl = H // tp, I // tp, V // tp
    w, q8, sc = list(weights), list(int8_w), list(scales)
    for l in range(L):
        w[3 * L + l] = weights[3 * L + l].view(3, 1, hl).expand(3, tp, hl).reshape(-1).contiguous()
        w[7 * L + l] = weights[7 * L + l].repeat(tp)
        w[9 * L + l] = (weights[9 * L + l].float() * tp).half()
        q8[0 * L + l] = int8_w[l].view(3, 1, hl // 16, -1).expand(3, tp, -1, -1).reshape(-1).contiguous()
        sc[0 * L + l] = scales[l].view(3, 1, hl).expand(3, tp, hl).reshape(-1).contiguous()
        q8[1 * L + l] = int8_w[L + l].view(H // 16, hl // 64, 1024).repeat(1, tp, 1).view(-1)
        q8[2 * L + l] = int8_w[2 * L + l].view(il // 16, -1).repeat(tp, 1).view(-1)
        sc[2 * L + l] = scales[2 * L + l].repeat(tp)
        q8[3 * L + l] = int8_w[3 * L + l].view(H // 16, il // 64, 1024).repeat(1, tp, 1).view(-1)
    emb, lm = weights[12 * L], weights[12 * L + 3]
    w[12 * L] = emb.view(tp, vl, H)[:1].expand(tp, -1, -1).reshape(emb.shape).contiguous()
    w[12 * L + 3] = lm.view(tp, vl, H)[r:r + 1].expand(tp, -1, -1).reshape(lm.shape).contiguous()
    return a, w, q8, sc


def _close(ref_t, ref_l, t, l, S, frac, what):
    scale = np.abs(ref_l).max()
    for b in range(ref_t.shape[0]):
        for s in range(ref_l.shape[0]):
            e = np.abs(l[s, b] - ref_l[s, b]).max() / scale
            assert e <= frac, (what, b, s, e)
            if t[b, S + s] != ref_t[b, S + s]:
                top2 = np.sort(ref_l[s, b])[-2:]
                assert top2[1] - top2[0] <= 2 * frac * scale, (what, b, s, "token flip without a near tie")
                break
