"""Per-request logit processors: what they cost.

1. The workload of tools/bench_batcher.py (13B-shaped int8 model, 32 requests of 256-in / 64..128-out over 16 slots), once plain and
   once with EVERY request carrying an allowed-token mask (half the vocabulary), 300 logit-bias pairs, both penalties and a
   64-entry bad-word list; the two legs alternate for --rounds rounds: milliseconds per batcher iteration of each leg.
2. The stage itself (ftcf_logit_process: two launches) on 16 rows of V = 100864 logits with the same options and a 384-token
   history, timed with device events over --reps calls that rotate over 8 logits buffers (51 MB: the stage never meets the
   buffer it has just written), against the same loop over rows without options (the launches alone): microseconds per call.

    python tools/bench_logit_processors.py [--rounds 3] [--out profiles/logit_processors_bench.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from fastertransformer4codefuse_amd import capi  # noqa: E402
from fastertransformer4codefuse_amd.batcher import ContinuousBatcher  # noqa: E402
from fastertransformer4codefuse_amd.gptneox_op import GptNeoXOp  # noqa: E402

V, END_ID = 100864, 2


def request_options(rng):
    """the options of one request: 300 bias pairs, both penalties, 64 bad words (32 single tokens, 32 bigrams), half the vocabulary
    allowed (the end token neither allowed nor biased: both legs generate the same number of tokens)"""
    ids = rng.choice(np.arange(3, V), size=300 + 96, replace=False)
    bias = {int(t): float(v) for t, v in zip(ids[:300], rng.randn(300) * 2)}
    w = ids[300:].tolist()
    words = [[t] for t in w[:32]] + [[w[32 + 2 * i], w[33 + 2 * i]] for i in range(32)]
    allowed = rng.rand(V) < 0.5
    allowed[END_ID] = False
    return dict(logit_bias=bias, bad_words=words, presence_penalty=0.5, frequency_penalty=0.2), allowed


def bench_batcher_legs(a):
    m = argparse.Namespace(layers=a.layers, heads=40, head_dim=128, inter=20480, vocab=V, rotary=32, dtype="int8")
    weights, int8_w, scales = bench.synth_weights(m, 1, torch.device("cuda", 0))
    op = GptNeoXOp(None, 0, m.heads, m.head_dim, m.inter, m.layers, m.vocab, m.rotary, 0, END_ID, 1, 1, 1, 2048, True, weights, int8_w, scales)
    per_seq = (a.prompt_len + a.new + a.page - 1) // a.page
    cb = ContinuousBatcher(op, a.slots, a.page, per_seq * a.slots, a.prompt_len + a.new)
    rng = np.random.RandomState(0)
    reqs = [(rng.randint(3, V, size=a.prompt_len).tolist(), int(rng.randint(a.new // 2, a.new + 1))) for _ in range(a.requests)]
    opts = [request_options(rng) for _ in reqs]

    def leg(processed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for (p, n), (kw, allowed) in zip(reqs, opts):
            rid = cb.submit(p, n, **(kw if processed else {}))
            if processed:
                cb.set_token_mask(rid, allowed)
        toks, iters = 0, 0
        while cb.busy():
            toks += len(cb.step())
            iters += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dict(generated_tokens=toks, iterations=iters, seconds=round(dt, 3), tokens_per_sec=round(toks / dt, 1),
                    ms_per_iteration=round(dt / iters * 1e3, 3))

    for processed in (False, True):  # warm-up: every kernel shape of both legs
        rid = cb.submit(reqs[0][0], 4, **(opts[0][0] if processed else {}))
        if processed:
            cb.set_token_mask(rid, opts[0][1])
        cb.run_all()
    runs = {"plain": [], "processed": []}
    for _ in range(a.rounds):
        for name in ("plain", "processed"):
            runs[name].append(leg(name == "processed"))
    med = {k: sorted(r["ms_per_iteration"] for r in v)[len(v) // 2] for k, v in runs.items()}
    return dict(workload=f"13B-shaped int8 (L={a.layers}), {a.requests} requests x {a.prompt_len}-in / {a.new // 2}..{a.new}-out, {a.slots} slots, "
                         f"{a.page}-token pages; processed: every request with a mask, 300 bias pairs, presence + frequency penalty, 64 bad words",
                runs=runs, median_ms_per_iteration=med, processed_minus_plain_us_per_iteration=round((med["processed"] - med["plain"]) * 1e3, 1),
                processed_over_plain_pct=round((med["processed"] / med["plain"] - 1) * 100, 2))


def bench_stage(a, B=16, T=384, gen_start=256, nbuf=8):
    rng = np.random.RandomState(1)
    g = torch.Generator(device="cuda").manual_seed(1)
    bufs = [torch.randn(B, V, generator=g, device="cuda") * 3 for _ in range(nbuf)]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    hist = dev(rng.randint(3, V, size=(T + 2, B)).astype(np.int32))  # time-major, as the batcher's
    bias_ids, bias_vals = np.zeros((B, 1024), np.int32), np.zeros((B, 1024), np.float32)
    bad = np.zeros((B, 2, 256), np.int32)
    mask = np.zeros((B, (V + 31) // 32), np.uint32)
    for b in range(B):
        kw, allowed = request_options(rng)
        bias_ids[b, :300], bias_vals[b, :300] = list(kw["logit_bias"]), list(kw["logit_bias"].values())
        flat = [t for w in kw["bad_words"] for t in w]
        bad[b, 0, :len(flat)] = flat
        bad[b, 1] = -1
        bad[b, 1, :len(kw["bad_words"])] = np.cumsum([len(w) for w in kw["bad_words"]])
        mask[b] = np.packbits(allowed, bitorder="little").view(np.uint32)
    t = dict(hist_len=dev(np.full(B, T, np.int32)), gen_start=dev(np.full(B, gen_start, np.int32)), pres=dev(np.full(B, 0.5, np.float32)),
             freq=dev(np.full(B, 0.2, np.float32)), n_bias=dev(np.full(B, 300, np.int32)), bias_ids=dev(bias_ids), bias_vals=dev(bias_vals),
             bad=dev(bad), mask=dev(mask.view(np.int32)), on=dev(np.ones(B, np.uint8)), off=dev(np.zeros(B, np.uint8)))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def args(buf, enabled):
        x = capi.LogitProcessArgs()
        x.struct_size, x.batch_size, x.vocab_size, x.end_id, x.logits = C.sizeof(x), B, V, END_ID, buf.data_ptr()
        x.row_on = (t["on"] if enabled else t["off"]).data_ptr()
        x.hist, x.stride_t, x.stride_b, x.hist_len, x.gen_start = hist.data_ptr(), B, 1, t["hist_len"].data_ptr(), t["gen_start"].data_ptr()
        x.presence_penalty, x.frequency_penalty, x.n_bias = t["pres"].data_ptr(), t["freq"].data_ptr(), t["n_bias"].data_ptr()
        x.bias_ids, x.bias_values, x.bias_stride = t["bias_ids"].data_ptr(), t["bias_vals"].data_ptr(), 1024
        x.bad_words, x.bad_words_len, x.mask = t["bad"].data_ptr(), 256, t["mask"].data_ptr()
        return x

    def timed(enabled):
        calls = [args(buf, enabled) for buf in bufs]
        for x in calls:
            capi.check(capi.lib().ftcf_logit_process(C.byref(x), stream))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(a.reps):
            capi.check(capi.lib().ftcf_logit_process(C.byref(calls[i % nbuf]), stream))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps

    res = {"processed": [], "launches_only": []}
    for _ in range(a.rounds):
        res["launches_only"].append(round(timed(False), 2))
        res["processed"].append(round(timed(True), 2))
    return dict(shape=f"{B} rows x V = {V}, {T}-token history ({T - gen_start} generated), the options of the processed leg on every row, "
                      f"{nbuf} logits buffers in rotation, {a.reps} calls per figure", us_per_call=res,
                median_us={k: sorted(v)[len(v) // 2] for k, v in res.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--prompt-len", type=int, default=256)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--page", type=int, default=64)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logit_processors_bench.txt"))
    a = ap.parse_args()
    capi.require_gpu()
    lines = ["device: " + torch.cuda.get_device_name(0),
             "stage: " + json.dumps(bench_stage(a)),
             "batcher: " + json.dumps(bench_batcher_legs(a))]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/bench_logit_processors.py\n" + text)


if __name__ == "__main__":
    main()
