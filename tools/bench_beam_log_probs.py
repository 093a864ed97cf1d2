"""Per-token log-probabilities of beam hypotheses: what they cost.

1. --step : ftcf_beam_search_step on random logits at V = 100864, K = 4 and K = 16 (one batch entry), with step_log_probs NULL and
   set.  Every call starts from the same saved state; the legs alternate call by call in one process; the figure is the median
   wall time of a call (upload of the runtime arguments, the two launches, the stream synchronisation).  The change is K stores
   in k_beam_batch: no difference beyond the spread is expected.
2. --getter : GptNeoXOp.beam_log_probs() after a K = 4 request of 1024 prompt tokens + 512 new ones on a small synthetic model
   (the walk does not depend on the model): milliseconds per call, the cost a caller pays once per request.

    python tools/bench_beam_log_probs.py --step --getter
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


def bench_step(K, reps, V=100864):
    g = torch.Generator(device="cuda").manual_seed(K)
    logits = torch.randn(K, V, generator=g, device="cuda") * 2.0
    S, total = 4, 16
    ids = torch.randint(3, V, (total, K), generator=g, device="cuda", dtype=torch.int32)
    par = torch.zeros((total, K), dtype=torch.int32, device="cuda")
    indir = torch.zeros((2, K, total), dtype=torch.int32, device="cuda")
    in_len = torch.full((K,), S, dtype=torch.int32, device="cuda")
    fin = torch.zeros(K, dtype=torch.uint8, device="cuda")
    seq = torch.full((K,), S + 1, dtype=torch.int32, device="cuda")
    cum0 = -torch.arange(K, dtype=torch.float32, device="cuda")
    cum = cum0.clone()
    lp = torch.zeros((total, K), dtype=torch.float32, device="cuda")
    a = capi.BeamSearchArgs()
    a.logits, a.output_ids, a.parent_ids, a.cache_indir = logits.data_ptr(), ids.data_ptr(), par.data_ptr(), indir.data_ptr()
    a.finished, a.seq_len, a.cum_log_probs, a.input_lengths = fin.data_ptr(), seq.data_ptr(), cum.data_ptr(), in_len.data_ptr()
    a.B, a.K, a.V, a.step, a.max_input_len, a.total_len, a.s_max, a.end_id = 1, K, V, S + 2, S, total, total, 2
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    us = {0: [], 1: []}
    after = {}
    for r in range(-10, reps):  # (10 warm-up rounds)
        for leg in (0, 1):
            a.step_log_probs = lp.data_ptr() if leg else None
            cum.copy_(cum0)
            fin.zero_()
            seq.fill_(S + 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            capi.check(capi.lib().ftcf_beam_search_step(C.byref(a), stream))
            dt = (time.perf_counter() - t0) * 1e6
            if r >= 0:
                us[leg].append(dt)
            after[leg] = (cum.cpu().clone(), ids[S + 2].cpu().clone())
    assert torch.equal(after[0][0], after[1][0]) and torch.equal(after[0][1], after[1][1])
    med = {leg: float(np.median(v)) for leg, v in us.items()}
    spread = {leg: [float(np.percentile(v, 25)), float(np.percentile(v, 75))] for leg, v in us.items()}
    out = dict(step=dict(K=K, V=V, reps=reps, median_us=dict(null=round(med[0], 2), set=round(med[1], 2)),
                         quartiles_us=dict(null=[round(x, 2) for x in spread[0]], set=[round(x, 2) for x in spread[1]]),
                         difference_pct=round((med[1] / med[0] - 1) * 100, 2)))
    print(json.dumps(out), flush=True)
    return out


def bench_getter(reps, K=4, S=1024, out_len=512):
    import bench
    from fastertransformer4codefuse_amd.gptneox_op import GptNeoXOp
    a = types.SimpleNamespace(layers=2, heads=8, head_dim=64, inter=2048, vocab=2048, dtype="fp16")
    dev = torch.device("cuda", 0)
    weights, int8_w, scales = bench.synth_weights(a, 1, dev)
    op = GptNeoXOp(None, 0, a.heads, a.head_dim, a.inter, a.layers, a.vocab, 16, 0, 2, 1, 1, 0, 2048, True, weights, int8_w, scales)
    ids = torch.randint(3, a.vocab, (1, S), generator=torch.Generator().manual_seed(42), dtype=torch.int32).to(dev)
    lens = torch.full((1,), S, dtype=torch.int32, device=dev)
    outs = op.forward(ids, lens, out_len, K, return_cum_log_probs=1)
    torch.cuda.synchronize()
    ms = []
    for r in range(-3, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lp = op.beam_log_probs()
        dt = (time.perf_counter() - t0) * 1e3
        if r >= 0:
            ms.append(dt)
    err = float((lp.double().sum(-1) - outs[2].double()).abs().max())
    out = dict(getter=dict(K=K, prompt=S, new=out_len, reps=reps, median_ms=round(float(np.median(ms)), 4),
                           min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), full_length=bool((outs[1] == S + out_len).all()),
                           sum_minus_cum_log_probs_max_abs=err))
    print(json.dumps(out), flush=True)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--step", action="store_true")
    p.add_argument("--getter", action="store_true")
    p.add_argument("--reps", type=int, default=200)
    a = p.parse_args()
    capi.require_gpu()
    print("device:", torch.cuda.get_device_name(0), flush=True)
    if a.step:
        for K in (4, 16):
            bench_step(K, a.reps)
    if a.getter:
        bench_getter(max(a.reps // 10, 5))


if __name__ == "__main__":
    main()
