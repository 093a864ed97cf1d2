"""Per-token log-probabilities: what they cost.

1. The fused LM head -> log-prob kernel (ftcf_lm_head_log_probs, csrc/kernels_logprob.hip) on the 13B head (100864 x 5120
   fp16) for m prompt rows: microseconds per call (HIP events over repeated calls), the fraction of the 2.5 PFLOP/s dense fp16
   peak, and the fraction of 8 TB/s for one read of the head.
2. A bs = 1 greedy request of the bench.py model (13B-shaped int8, synthetic weights) with return_cum_log_probs = 1, with and
   without output_log_probs: milliseconds per decode step, legs alternated.

    python tools/bench_logprobs.py [--rows 64,256,1024,2048] [--steps 64] [--rounds 3] [--no-request]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fastertransformer4codefuse_amd import capi  # noqa: E402

PEAK_FLOPS = 2.5e15
PEAK_BYTES = 8e12


def bench_kernel(rows, reps=20):
    n, k = 100864, 5120
    g = torch.Generator(device="cuda").manual_seed(1)
    W = (torch.randn(n, k, generator=g, device="cuda") * 0.02).half()
    res = []
    for m in rows:
        A = torch.randn(m, k, generator=g, device="cuda").half()
        t = torch.randint(0, n, (m,), generator=g, device="cuda", dtype=torch.int32)
        lp = torch.empty(m, dtype=torch.float32, device="cuda")
        call = lambda: capi.check(capi.lib().ftcf_lm_head_log_probs(capi.vp(A), capi.vp(W), capi.vp(t), capi.vp(lp), C.c_void_p(None),
                                                                    m, n, k, C.c_void_p(None)))
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        flops = 2.0 * m * n * k
        byts = 2.0 * n * k + 2.0 * m * k
        res.append(dict(m=m, us=round(us, 1), tflops=round(flops / us * 1e-6, 1), frac_peak_flops=round(flops / (us * 1e-6) / PEAK_FLOPS, 3),
                        frac_8tbs=round(byts / (us * 1e-6) / PEAK_BYTES, 3)))
        print(json.dumps(res[-1]), flush=True)
    del W
    torch.cuda.empty_cache()
    return res


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
    top_k = (C.c_int * 1)(1)
    minlen = (C.c_int * 1)(out_len)
    L = capi.lib()

    def leg(with_olp):
        fa = capi.ForwardArgs()
        fa.input_ids, fa.input_lengths = ids.data_ptr(), lens.data_ptr()
        fa.batch_size, fa.max_input_len, fa.output_len, fa.beam_width = B, S, out_len, 1
        fa.top_k, fa.n_top_k = C.cast(top_k, C.c_void_p), 1
        fa.min_length, fa.n_min_length = C.cast(minlen, C.c_void_p), 1
        fa.return_cum_log_probs = 1
        fa.output_ids, fa.sequence_lengths, fa.cum_log_probs = out_ids.data_ptr(), seq.data_ptr(), cum.data_ptr()
        if with_olp:
            fa.output_log_probs = olp.data_ptr()
        capi.check(L.ftcf_gptneox_begin(op._h, C.byref(fa)))
        capi.check(L.ftcf_gptneox_step(op._h, 16, None))  # warm-up steps (graph capture)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        capi.check(L.ftcf_gptneox_step(op._h, steps, None))
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        capi.check(L.ftcf_gptneox_finish(op._h))
        return ms, out_ids.cpu().clone(), cum.cpu().clone()

    leg(False)
    res = {"off": [], "on": []}
    for _ in range(rounds):
        for name in ("off", "on"):
            ms, toks, c = leg(name == "on")
            res[name].append(round(ms, 4))
            res[name + "_tokens"], res[name + "_cum"] = toks, c
    same = bool(torch.equal(res["off_tokens"], res["on_tokens"]) and torch.equal(res["off_cum"], res["on_cum"]))
    summ = dict(ms_per_step_off=res["off"], ms_per_step_on=res["on"], best_off=min(res["off"]), best_on=min(res["on"]),
                overhead_pct=round((min(res["on"]) / min(res["off"]) - 1) * 100, 2), tokens_and_cum_identical=same,
                decode_path=op.stats()["decode_path"])
    print(json.dumps(summ), flush=True)
    return summ


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="64,256,1024,2048")
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--prompt-len", type=int, default=128)
    p.add_argument("--no-request", action="store_true")
    a = p.parse_args()
    capi.require_gpu()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    bench_kernel([int(x) for x in a.rows.split(",") if x])
    if not a.no_request:
        bench_request(a.steps, a.rounds, a.prompt_len)


if __name__ == "__main__":
    main()
