"""Overcommit of the continuous batcher (ftcf_batcher_create_opts): what it buys and what a swap costs.

13B-shaped int8 model, 16 slots, 64-token pages.  64 requests of 256 prompt tokens declare max_new_tokens = 1024; the client
cancels each after 64..128 tokens (seeded).

A. The pool holds 16 x (256 + 128) tokens.  Reservation against overcommit, the two legs alternating in one process for
   --rounds rounds: generated tokens/s, mean running slots per iteration, median time to first token.
B. The same with half the pool, so that requests are preempted: the same figures, the preemptions and pages moved, and the
   milliseconds an iteration with a swap-out / a swap-in takes beyond the median iteration without one.
L. B with half as many requests that run for 256..512 tokens (one round): a request of this workload grows by at most one page
   after admission, which the admission watermark already sets aside, so B itself preempts nobody; these do.
C. The copy itself, for the pages of one 384-token victim (6 pages of every layer of both pools): k_pages_pack + one linear
   hipMemcpyAsync per chunk (what the batcher does) against one hipMemcpy2DAsync per page and pool (pitch = the layer stride)
   against ONE contiguous hipMemcpyAsync of the same byte count -- the link's own rate -- all into the same pinned region.

    python tools/bench_overcommit.py [--rounds 2] [--legs ABCL] [--out profiles/overcommit_bench.txt]
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


def serve(cb, reqs, declared):
    """submit everything at once, cancel each request after its own number of tokens; figures of the run"""
    stamps, count, steps = {}, {}, []
    cb.set_token_callback(lambda rid, tok, fin: stamps.setdefault(rid, time.perf_counter()))
    pe0 = cb.preempt_stats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sub = {}
    for p, n in reqs:
        rid = cb.submit(p, declared)
        sub[rid] = (time.perf_counter(), n)
    toks, running = 0, []
    while cb.busy():
        before = cb.preempt_stats()
        t = time.perf_counter()
        events = cb.step()
        dt = time.perf_counter() - t
        after = cb.preempt_stats()
        steps.append((dt, after["preemptions"] - before["preemptions"], after["resumes"] - before["resumes"],
                      after["pages_out"] - before["pages_out"], after["pages_in"] - before["pages_in"]))
        running.append(cb.status()["running"])
        for rid, tok, fin in events:
            toks += 1
            count[rid] = count.get(rid, 0) + 1
            if count[rid] == sub[rid][1] and not fin:
                cb.cancel(rid)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    cb.set_token_callback(None)
    ttft = sorted((stamps[r] - ts) * 1e3 for r, (ts, _) in sub.items())
    pe = cb.preempt_stats()
    res = dict(generated_tokens=toks, seconds=round(dt, 3), tokens_per_sec=round(toks / dt, 1), iterations=len(steps),
               mean_running_slots=round(float(np.mean(running)), 2), ttft_ms_median=round(ttft[len(ttft) // 2], 1),
               ttft_ms_max=round(ttft[-1], 1))
    if pe["enabled"]:
        plain = sorted(s[0] for s in steps if s[1] == 0 and s[2] == 0)
        base = plain[len(plain) // 2] if plain else 0.0
        outs = [(s[0] - base) * 1e3 / s[1] for s in steps if s[1] > 0 and s[2] == 0]
        ins = [(s[0] - base) * 1e3 / s[2] for s in steps if s[2] > 0 and s[1] == 0]
        res.update(preemptions=pe["preemptions"] - pe0["preemptions"], resumes=pe["resumes"] - pe0["resumes"],
                   pages_out=pe["pages_out"] - pe0["pages_out"], pages_in=pe["pages_in"] - pe0["pages_in"],
                   median_iteration_ms=round(base * 1e3, 3),
                   ms_per_swap_out=round(float(np.median(outs)), 2) if outs else None,
                   ms_per_swap_in=round(float(np.median(ins)), 2) if ins else None)
    return res


def legs_ab(a, op, halve, new=None, requests=None, rounds=None):
    pages = a.slots * (a.prompt_len + a.new) // a.page // (2 if halve else 1)
    new, requests, rounds = new or a.new, requests or a.requests, rounds or a.rounds
    rng = np.random.RandomState(0)
    reqs = [(rng.randint(3, V, size=a.prompt_len).tolist(), int(rng.randint(new // 2, new + 1))) for _ in range(requests)]
    geometry = dict(max_batch=a.slots, page_tokens=a.page, num_pages=pages, max_seq_len=a.prompt_len + a.declared)
    runs = {"reservation": [], "overcommit": []}
    cbs = {"reservation": ContinuousBatcher(op, **geometry), "overcommit": ContinuousBatcher(op, overcommit=True, **geometry)}
    for cb in cbs.values():  # warm-up: every kernel shape
        cb.submit(reqs[0][0], 4)
        cb.run_all()
    for _ in range(rounds):
        for name, cb in cbs.items():
            runs[name].append(serve(cb, reqs, a.declared))
    med = {k: sorted(r["tokens_per_sec"] for r in v)[len(v) // 2] for k, v in runs.items()}
    return dict(workload=f"13B-shaped int8 (L={a.layers}), {requests} requests x {a.prompt_len}-in, max_new_tokens {a.declared}, cancelled "
                         f"after {new // 2}..{new} tokens, {a.slots} slots, {pages} pages of {a.page} tokens",
                runs=runs, median_tokens_per_sec=med, overcommit_over_reservation=round(med["overcommit"] / med["reservation"], 3))


def leg_c(a, n_pages=6, pool_pages=24, reps=5):
    try:
        hip = C.CDLL("libamdhip64.so")  # (the runtime torch and libftcf have loaded)
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    L, nh, P, dh = a.layers, 40, a.page, 128
    page_elems = nh * P * dh
    layer_elems = pool_pages * page_elems
    kpool = torch.randn(L * layer_elems, device="cuda", dtype=torch.float16)
    vpool = torch.randn(L * layer_elems, device="cuda", dtype=torch.float16)
    total = n_pages * 2 * L * page_elems * 2  # bytes
    stage_pages = max(1, (64 << 20) // (2 * L * page_elems * 2))
    stage = torch.empty(stage_pages * 2 * L * page_elems, device="cuda", dtype=torch.float16)
    src = torch.empty(total // 2, device="cuda", dtype=torch.float16)
    host = torch.empty(total // 2, dtype=torch.float16).pin_memory()
    pages = torch.tensor([5, 0, 3, 17, 9, 22][:n_pages], dtype=torch.int32, device="cuda")
    plist = pages.cpu().tolist()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    D2H, chunk_bytes = 2, 2 * L * page_elems * 2
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]

    def packed():
        for c0 in range(0, n_pages, stage_pages):
            nc = min(stage_pages, n_pages - c0)
            capi.check(capi.lib().ftcf_pages_pack(capi.vp(stage), capi.vp(kpool), capi.vp(vpool), C.c_void_p(pages.data_ptr() + 4 * c0), nc, L,
                                                  nh, dh, P, C.c_size_t(layer_elems), stream))
            assert hip.hipMemcpyAsync(host.data_ptr() + c0 * chunk_bytes, stage.data_ptr(), nc * chunk_bytes, D2H, stream) == 0

    def per_page_2d():
        for j, pg in enumerate(plist):
            for k, pool in enumerate((kpool, vpool)):
                assert hip.hipMemcpy2DAsync(host.data_ptr() + (2 * j + k) * L * page_elems * 2, page_elems * 2,
                                            pool.data_ptr() + pg * page_elems * 2, layer_elems * 2, page_elems * 2, L, D2H, stream) == 0

    def contiguous():
        assert hip.hipMemcpyAsync(host.data_ptr(), src.data_ptr(), total, D2H, stream) == 0

    out = {}
    for name, fn in (("pack_plus_linear_copy", packed), ("memcpy2d_per_page_and_pool", per_page_2d), ("contiguous_memcpy", contiguous)):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out[name] = dict(ms=round(float(np.median(ts)) * 1e3, 2), GB_per_s=round(total / float(np.median(ts)) / 1e9, 1))
    out["bytes"] = total
    out["pack_over_contiguous"] = round(out["pack_plus_linear_copy"]["ms"] / out["contiguous_memcpy"]["ms"], 3)
    out["shape"] = f"{n_pages} pages x 2 pools x {L} layers x {page_elems * 2} B, device -> one pinned region, staging {stage_pages} page(s)"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--prompt-len", type=int, default=256)
    ap.add_argument("--new", type=int, default=128, help="the clients cancel after new / 2 .. new tokens")
    ap.add_argument("--declared", type=int, default=1024, help="max_new_tokens of every request")
    ap.add_argument("--page", type=int, default=64)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--legs", default="ABCL")
    ap.add_argument("--long-new", type=int, default=512, help="leg L: the clients cancel after long_new / 2 .. long_new tokens")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overcommit_bench.txt"))
    a = ap.parse_args()
    capi.require_gpu()
    lines = ["device: " + torch.cuda.get_device_name(0)]
    if "C" in a.legs:
        lines.append("C copy: " + json.dumps(leg_c(a)))
        print(lines[-1], flush=True)
    if set("ABL") & set(a.legs):
        m = argparse.Namespace(layers=a.layers, heads=40, head_dim=128, inter=20480, vocab=V, rotary=32, dtype="int8")
        weights, int8_w, scales = bench.synth_weights(m, 1, torch.device("cuda", 0))
        op = GptNeoXOp(None, 0, m.heads, m.head_dim, m.inter, m.layers, m.vocab, m.rotary, 0, END_ID, 1, 1, 1, 2048, True, weights, int8_w, scales)
        for leg, halve in (("A", False), ("B", True)):
            if leg in a.legs:
                lines.append(f"{leg} {'half pool' if halve else 'full pool'}: " + json.dumps(legs_ab(a, op, halve)))
                print(lines[-1], flush=True)
        if "L" in a.legs:  # B with outputs that outgrow the watermark of one page per running request: requests ARE preempted
            lines.append("L half pool, long outputs: " + json.dumps(legs_ab(a, op, True, new=a.long_new, requests=a.requests // 2, rounds=1)))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/bench_overcommit.py\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
