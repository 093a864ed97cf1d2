"""Weight-only int8 quantiser at load time: host (ftcf_symmetric_quantize_int8, csrc/host_quant.cc) against device
(ftcf_symmetric_quantize_int8_device, csrc/kernels_quant.hip), same machine, same run.

1. The four GEMM matrices of a CodeFuse-13B layer (fp16): host seconds per call at the thread count the machine gives (min and max of 3); device
   kernel time from HIP events over repeated calls (rotating through buffer sets larger than the last-level cache, so the
   figure is not cache-warm) with the bytes/s it implies, counting K * N * (2 * sizeof(T) + 1) (the two
   reads of the weight and the int8 write) against 8 TB/s; device time including the upload from pageable host memory (host clock
   around upload + kernels + synchronise).  The device result is compared with the host's, byte for byte.
2. GptNeoXWeights.load of a 13B-shaped checkpoint of --layers layers (random fp16 files written to --dir), int8_mode = 1, with
   and without quantize_on_device: wall seconds, and the per-layer part scaled to 40 layers.

    python tools/bench_quantize.py [--layers 2] [--reps 20] [--dir /tmp/ftcf_bench_quantize] [--out FILE] [--no-load]
"""
import argparse
import ctypes as C
import os
import shutil
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fastertransformer4codefuse_amd import capi, harness  # noqa: E402
from fastertransformer4codefuse_amd.gptneox_op import (  # noqa: E402
    symmetric_quantize_last_axis_of_batched_matrix_int8 as host_quant,
    symmetric_quantize_last_axis_of_batched_matrix_int8_device as dev_quant)

PEAK_BYTES = 8e12
H, HEADS, INTER = 5120, 40, 20480
SHAPES = [("qkv", H, 3 * H), ("out", H, H), ("ffn1", H, INTER), ("ffn2", INTER, H)]
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def bench_matrices(reps):
    L = capi.lib()
    say(f"host threads: OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '(unset)')}, torch.get_num_threads()={torch.get_num_threads()}")
    say(f"device: {torch.cuda.get_device_name(0)}")
    say("matrix   K x N (fp16)    host s/call (min of 3; max)   device kernels us   GB/s   of 8 TB/s   device incl. upload s   host / (device incl. upload)   identical")
    tot_host = tot_dev = tot_up = 0.0
    for name, K, N in SHAPES:
        w = (torch.randn(K, N, generator=torch.Generator().manual_seed(K + N)) * 0.02).half()
        host_quant(w[:64].contiguous())  # (thread pool start-up is not the quantiser)
        host_runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            hq, hs = host_quant(w)
            host_runs.append(time.perf_counter() - t0)
        host_s = min(host_runs)
        # kernels only: HIP events around `reps` calls that rotate through `sets` resident weight / output sets, so many that
        # their footprint (K * N * 3 bytes each) is three times the 256 MiB last-level cache: no call finds its lines cached
        sets = max(2, -(-768 * 2 ** 20 // (K * N * 3)))
        wd = [w.cuda() for _ in range(sets)]
        q = [torch.empty((K, N), dtype=torch.int8, device="cuda") for _ in range(sets)]
        s = torch.empty(N, dtype=torch.float16, device="cuda")
        ws_bytes = int(L.ftcf_symmetric_quantize_int8_device_workspace(C.c_size_t(1), C.c_size_t(N)))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        call = lambda i: capi.check(L.ftcf_symmetric_quantize_int8_device(
            capi.vp(wd[i % sets]), capi.FP16, C.c_size_t(1), C.c_size_t(K), C.c_size_t(N), capi.vp(q[i % sets]), capi.vp(s),
            capi.vp(ws), C.c_size_t(ws_bytes), C.c_void_p(stream)))
        for i in range(sets):
            call(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            call(i)
        e1.record()
        torch.cuda.synchronize()
        dev_s = e0.elapsed_time(e1) * 1e-3 / reps
        same = all(torch.equal(x.cpu(), hq) for x in q) and torch.equal(s.cpu().view(torch.int16), hs.view(torch.int16))
        del wd, q, s, ws
        # upload from pageable memory + kernels, as the load path runs it (best of 3)
        up_s = 1e9
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dq, ds = dev_quant(w)
            torch.cuda.synchronize()
            up_s = min(up_s, time.perf_counter() - t0)
            del dq, ds
        nbytes = K * N * (2 * 2 + 1)
        say(f"{name:5s} {K:6d} x {N:<6d}   {host_s:10.3f} ({max(host_runs):.3f})          {dev_s * 1e6:14.1f}   {nbytes / dev_s / 1e9:7.0f}   {nbytes / dev_s / PEAK_BYTES:8.1%}"
            f"   {up_s:18.4f}   {host_s / up_s:20.1f}x   {'yes' if same else 'NO'}")
        tot_host, tot_dev, tot_up = tot_host + host_s, tot_dev + dev_s, tot_up + up_s
    say(f"one layer (4 matrices): host {tot_host:.3f} s, device kernels {tot_dev * 1e3:.3f} ms, device incl. upload {tot_up:.3f} s;"
        f" x 40 layers: host {40 * tot_host:.1f} s, device incl. upload {40 * tot_up:.1f} s")


def write_checkpoint(d, layers, vocab):
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(0)

    def put(name, *shape):
        (rng.standard_normal(shape, dtype=np.float32) * 0.02).astype(np.float16).tofile(os.path.join(d, name + ".bin"))

    for l in range(layers):
        p = f"model.layers.{l}."
        for n in ("input_layernorm.bias", "input_layernorm.weight", "post_attention_layernorm.bias", "post_attention_layernorm.weight",
                  "mlp.attention.bias.sum"):
            put(p + n, H)
        put(p + "attention.query_key_value.weight.0", H, 3 * H)
        put(p + "attention.query_key_value.bias.0", 3 * H)
        put(p + "attention.dense.weight.0", H, H)
        put(p + "mlp.dense_h_to_4h.weight.0", H, INTER)
        put(p + "mlp.dense_h_to_4h.bias.0", INTER)
        put(p + "mlp.dense_4h_to_h.weight.0", INTER, H)
    put("model.wte", vocab, H)
    put("model.final_layernorm.weight", H)
    put("model.final_layernorm.bias", H)
    put("model.lm_head.weight", vocab, H)


def bench_load(d, layers, vocab=1024):
    write_checkpoint(d, layers, vocab)
    say()
    say(f"GptNeoXWeights.load, 13B-shaped checkpoint of {layers} layers (fp16 files, vocabulary {vocab}), int8_mode = 1; page cache warm")
    res = {}
    for on_device in (False, True, False, True):  # alternated; the first pair also warms the page cache
        w = harness.GptNeoXWeights(HEADS, H // HEADS, layers, vocab, 1024, 1, 1, True, int8_mode=1, inference_data_type="fp16",
                                   weights_data_type=np.float16, inter_size=INTER, quantize_on_device=on_device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert w.load(d, 0, 0)
        w._map_int8(lambda t: t.cuda())  # (what GptNeoX.cuda() does next: the host path uploads its int8 tensors here)
        torch.cuda.synchronize()
        res.setdefault(on_device, []).append(time.perf_counter() - t0)
        del w
    for on_device in (False, True):
        best = min(res[on_device])
        say(f"  quantize_on_device={on_device!s:5s}: {best:8.3f} s (runs: {', '.join('%.3f' % t for t in res[on_device])})"
            f" -> {best / layers:.3f} s per layer, {best / layers * 40:.1f} s for 40 layers")
    say(f"  host / device: {min(res[False]) / min(res[True]):.2f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dir", default="/tmp/ftcf_bench_quantize")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--no-load", action="store_true")
    a = ap.parse_args()
    capi.require_gpu()
    bench_matrices(a.reps)
    if not a.no_load:
        try:
            bench_load(a.dir, a.layers)
        finally:
            shutil.rmtree(a.dir, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
