"""top_logprobs: what it costs.

1. --kernels B,N : REPS dynamic-decode steps (ftcf_dynamic_decode_step, general form, top_k = 1, return_cum_log_probs) on random
   logits at V = 100864 with top_logprobs = N.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_top_logprobs.py
   --kernels 1,5`: the trace's per-kernel averages are the durations of k_top_logprobs_slices / k_top_logprobs_merge next to
   k_decode_prep / k_topk_stage1 / k_sample / k_decode_finish of the same steps.
2. --request : a bs = 1 greedy request of the bench.py model (13B-shaped int8, synthetic weights) with return_cum_log_probs = 1
   and output_log_probs, without top_logprobs (the one-launch greedy step) and with N = 5 / N = 20 (the general four launches +
   the two new ones): milliseconds per decode step, legs alternated, tokens and cum_log_probs compared.

    python tools/bench_top_logprobs.py --request [--steps 64] [--rounds 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fastertransformer4codefuse_amd import capi  # noqa: E402


def run_kernels(B, N, reps, V=100864):
    g = torch.Generator(device="cuda").manual_seed(B * 100 + N)
    src = torch.randn(B, V, generator=g, device="cuda") * 2.0
    total, mil = 16, 4
    ids = torch.randint(3, V, (total, B), generator=g, device="cuda", dtype=torch.int32)
    lens = torch.full((B,), mil, dtype=torch.int32, device="cuda")
    top_ids = torch.empty((total - mil, B, N), dtype=torch.int32, device="cuda")
    top_lps = torch.empty((total - mil, B, N), dtype=torch.float32, device="cuda")
    olp = torch.empty((total - mil, B), dtype=torch.float32, device="cuda")
    k = np.ones(1, np.int32)
    for _ in range(reps):
        logits = src.clone()
        fin, slen = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.full((B,), mil + 1, dtype=torch.int32, device="cuda")
        cum, draws = torch.zeros(B, dtype=torch.float32, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda")
        a = capi.DynamicDecodeArgs()
        a.logits, a.output_ids, a.finished, a.seq_len = logits.data_ptr(), ids.data_ptr(), fin.data_ptr(), slen.data_ptr()
        a.cum_log_probs, a.output_log_probs, a.draw_counter = cum.data_ptr(), olp.data_ptr(), draws.data_ptr()
        a.input_lengths = lens.data_ptr()
        a.top_k, a.n_top_k = k.ctypes.data, 1
        a.B, a.V, a.step, a.max_input_len, a.total_len, a.end_id, a.return_cum_log_probs, a.finish = B, V, mil + 2, mil, total, 2, 1, 1
        a.top_logprobs, a.top_ids, a.top_log_probs = N, top_ids.data_ptr(), top_lps.data_ptr()
        capi.check(capi.lib().ftcf_dynamic_decode_step(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert int(top_ids[2, 0, 0]) == int(src[0].argmax())
    print(json.dumps(dict(kernels=dict(B=B, N=N, V=V, reps=reps))), flush=True)


def bench_request(steps, rounds, prompt_len):
    import bench
    from fastertransformer4codefuse_amd.gptneox_op import GptNeoXOp
    a = types.SimpleNamespace(layers=40, heads=40, head_dim=128, inter=20480, vocab=100864, dtype="int8")
    dev = torch.device("cuda", 0)
    weights, int8_w, scales = bench.synth_weights(a, 1, dev)
    op = GptNeoXOp(None, 0, a.heads, a.head_dim, a.inter, a.layers, a.vocab, 32, 0, 2, 1, 1, 1, 2048, True, weights, int8_w, scales)
    B, S, out_len = 1, prompt_len, steps + 16
    gi = torch.Generator().manual_seed(42)
    ids = torch.randint(3, a.vocab, (B, S), generator=gi, dtype=torch.int32).to(dev)
    lens = torch.full((B,), S, dtype=torch.int32, device=dev)
    out_ids = torch.empty((B, 1, S + out_len), dtype=torch.int32, device=dev)
    seq = torch.empty((B, 1), dtype=torch.int32, device=dev)
    cum = torch.empty((B, 1), dtype=torch.float32, device=dev)
    olp = torch.empty((B, 1, out_len), dtype=torch.float32, device=dev)
    tid = torch.empty((B, 1, out_len, 20), dtype=torch.int32, device=dev)
    tlp = torch.empty((B, 1, out_len, 20), dtype=torch.float32, device=dev)
    top_k = (C.c_int * 1)(1)
    minlen = (C.c_int * 1)(out_len)
    L = capi.lib()

    def leg(N):
        fa = capi.ForwardArgs()
        fa.input_ids, fa.input_lengths = ids.data_ptr(), lens.data_ptr()
        fa.batch_size, fa.max_input_len, fa.output_len, fa.beam_width = B, S, out_len, 1
        fa.top_k, fa.n_top_k = C.cast(top_k, C.c_void_p), 1
        fa.min_length, fa.n_min_length = C.cast(minlen, C.c_void_p), 1
        fa.return_cum_log_probs = 1
        fa.output_ids, fa.sequence_lengths, fa.cum_log_probs = out_ids.data_ptr(), seq.data_ptr(), cum.data_ptr()
        fa.output_log_probs = olp.data_ptr()
        if N:
            fa.top_logprobs, fa.top_logprob_ids, fa.top_logprob_values = N, tid.data_ptr(), tlp.data_ptr()
        capi.check(L.ftcf_gptneox_begin(op._h, C.byref(fa)))
        capi.check(L.ftcf_gptneox_step(op._h, 16, None))  # warm-up steps (graph capture)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        capi.check(L.ftcf_gptneox_step(op._h, steps, None))
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        capi.check(L.ftcf_gptneox_finish(op._h))
        torch.cuda.synchronize()
        first = tid.view(-1)[:B * out_len * N].view(B, out_len, N)[0, :, 0].cpu().clone() if N else None  # (the buffer is [B, 1, out_len, N])
        return ms, out_ids.cpu().clone(), cum.cpu().clone(), first

    leg(0)
    legs = (0, 5, 20)
    res = {N: [] for N in legs}
    last = {}
    for _ in range(rounds):
        for N in legs:
            ms, toks, c, first = leg(N)
            res[N].append(round(ms, 4))
            last[N] = (toks, c, first)
    same = all(torch.equal(last[0][0], last[N][0]) for N in (5, 20))
    # (the general form adds the slices' soft-max statistics in another order than the one-launch greedy step: last bits)
    cum_diff = max(float((last[0][1] - last[N][1]).abs().max()) for N in (5, 20))
    greedy = all(torch.equal(last[N][2], last[N][0][0, 0, S:S + out_len]) for N in (5, 20))  # pair 0 is the emitted token
    med = {N: sorted(v)[len(v) // 2] for N, v in res.items()}
    summ = dict(ms_per_step={str(N): v for N, v in res.items()}, median={str(N): m for N, m in med.items()},
                overhead_pct={str(N): round((med[N] / med[0] - 1) * 100, 2) for N in (5, 20)},
                tokens_identical=bool(same), cum_log_probs_max_abs_diff=cum_diff, cum_log_probs=float(last[0][1][0, 0]),
                first_pair_is_the_token=bool(greedy), decode_path=op.stats()["decode_path"])
    print(json.dumps(summ), flush=True)
    return summ


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--kernels", default=None, help="B,N: run REPS decode steps with top_logprobs = N on B rows (for rocprofv3)")
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--request", action="store_true")
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--prompt-len", type=int, default=128)
    a = p.parse_args()
    capi.require_gpu()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    if a.kernels:
        B, N = (int(x) for x in a.kernels.split(","))
        run_kernels(B, N, a.reps)
    if a.request:
        bench_request(a.steps, a.rounds, a.prompt_len)


if __name__ == "__main__":
    main()
