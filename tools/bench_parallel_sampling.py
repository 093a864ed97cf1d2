"""n samples of one prompt: K plain submissions against one submit_n (ftcf_batcher_submit_n).

The model of tools/bench_batcher.py (13B-shaped, synthetic int8 weights), one 1024-token prompt, 64 new tokens per sample, top-k
sampling with seeds seed + i, K in {4, 8, 16} samples over 16 slots and 64-token pages.  Leg A submits the prompt K times (one
ragged prompt phase of K rows, K copies of the prompt's pages); leg B submits it once with n = K (one prompt phase of one row, the
prompt's 16 full pages held once).  The legs alternate in one process for --rounds rounds.  Per leg:
  * first_tokens_ms: from the submission to the last sample's first-token event;
  * pages_in_use: pool pages held right after the admission -- leg B must hold exactly shared + K * own (checked, not measured);
  * tokens_per_sec over the whole run (submission to the last token).

    python tools/bench_parallel_sampling.py [--rounds 3] [--out profiles/parallel_sampling_bench.txt]
"""
import argparse
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


def run_leg(cb, a, prompt, K, fork, num_pages):
    kw = dict(top_k=8, temperature=0.9)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if fork:
        ids = cb.submit_n(prompt, a.new, K, seed=a.seed, **kw)
    else:
        ids = [cb.submit(prompt, a.new, seed=a.seed + i, **kw) for i in range(K)]
    seen, toks, iters, first_ms, pages = set(), 0, 0, None, None
    while cb.busy():
        evs = cb.step()
        toks += len(evs)
        iters += 1
        seen.update(e[0] for e in evs)
        if first_ms is None and len(seen) == K:
            first_ms = (time.perf_counter() - t0) * 1e3
            pages = num_pages - cb.status()["free_pages"]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert sorted(seen) == sorted(ids)
    return dict(first_tokens_ms=round(first_ms, 2), pages_in_use=pages, generated_tokens=toks, iterations=iters, seconds=round(dt, 3),
                tokens_per_sec=round(toks / dt, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--prompt-len", type=int, default=1024)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--page", type=int, default=64)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--samples", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parallel_sampling_bench.txt"))
    a = ap.parse_args()
    capi.require_gpu()
    m = argparse.Namespace(layers=a.layers, heads=40, head_dim=128, inter=20480, vocab=V, rotary=32, dtype="int8")
    weights, int8_w, scales = bench.synth_weights(m, 1, torch.device("cuda", 0))
    op = GptNeoXOp(None, 0, m.heads, m.head_dim, m.inter, m.layers, m.vocab, m.rotary, 0, END_ID, 1, 1, 1, 2048, True, weights, int8_w, scales)
    per_seq = (a.prompt_len + a.new + a.page - 1) // a.page
    shared = a.prompt_len // a.page
    own = per_seq - shared
    num_pages = per_seq * a.slots
    cb = ContinuousBatcher(op, a.slots, a.page, num_pages, a.prompt_len + a.new)
    prompt = np.random.RandomState(0).randint(3, V, size=a.prompt_len).tolist()
    for fork in (False, True):  # warm-up: every kernel shape of both legs
        run_leg(cb, argparse.Namespace(new=4, seed=a.seed), prompt, 2, fork, num_pages)
    lines = ["device: " + torch.cuda.get_device_name(0),
             f"workload: 13B-shaped int8 (L={a.layers}), one {a.prompt_len}-token prompt, {a.new} new tokens per sample, top_k 8, "
             f"{a.slots} slots, {a.page}-token pages ({num_pages} in the pool); a sample at full length: {per_seq} pages = {shared} full "
             f"prompt pages + {own} of its own"]
    for K in a.samples:
        runs = {"plain": [], "submit_n": []}
        for _ in range(a.rounds):
            for name in ("plain", "submit_n"):
                runs[name].append(run_leg(cb, a, prompt, K, name == "submit_n", num_pages))
        for r in runs["plain"]:
            assert r["pages_in_use"] == K * per_seq, r
        for r in runs["submit_n"]:
            assert r["pages_in_use"] == shared + K * own, r  # (the accounting, not a measurement)
        med = {k: {f: sorted(r[f] for r in v)[len(v) // 2] for f in ("first_tokens_ms", "tokens_per_sec", "pages_in_use")}
               for k, v in runs.items()}
        fs = cb.fork_stats()
        lines.append(f"K={K}: " + json.dumps(dict(median=med, runs=runs, fork_stats=fs)))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("tools/bench_parallel_sampling.py\n" + text)


if __name__ == "__main__":
    main()
