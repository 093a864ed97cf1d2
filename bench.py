#!/usr/bin/env python3
"""Headline benchmark: decode tokens/s of a CodeFuse-13B-shaped GPT-NeoX (weight-only int8 by default), bs=1,
1024-token prompt + 512 generated tokens, tensor parallel over --gpus ranks (one process per GPU, RCCL).

  python bench.py --gpus 1 --steps 504 --warmup 8            # N = 1
  python bench.py --gpus 1 --steps 504 --warmup 8 --full     # + end-to-end request, roofline, CPU baseline
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A "step" is one decoded token (one pass of the per-token hot path: L decoder layers + LM head + dynamic decode).
The request is ALWAYS the headline one -- a 1024-token prompt prefilled through the real context path (KV cache resident
in HBM) and --output-len (512) generated tokens -- whatever --steps / --warmup say: the K timed steps (preceded by W
untimed ones) are a window of that request centred on output token 256, i.e. on the mean KV length 1280 of the whole
request (K + W >= 512: the whole request is the window; K + W > --output-len lengthens the request to K + W tokens, so K is
always the number of timed steps).  The steps before and after the window run untimed.  That is all a plain run does
besides one short warm-up request; --full adds the legs that the headline figure does not need: one complete
ftcf_gptneox_forward of the same request (end-to-end latency), a profiled run of the window's KV lengths (roofline, with a
rocprofv3 PMC child process at N = 1) and the whole-model CPU baseline.  --dump-outputs DIR writes what the measured
request returned to its caller (output ids, sequence lengths, cumulative log-probs) as DIR/<name>.npy; the inputs are
seeded, so two builds run with the same arguments can be compared output for output.  return_cum_log_probs = 1 as in the
reference harness (codefuse_example.py:745).  Weights are synthetic (random int8 + fp16 scales of CodeFuse-13B's shape,
generated on the device); there is no network for checkpoints.  Rank 0 prints ONE JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=504, help="timed decode steps (>= 1)")
    p.add_argument("--warmup", type=int, default=8)
    p.add_argument("--dtype", default="int8", choices=["int8", "fp16"])
    p.add_argument("--prompt-len", type=int, default=1024)
    p.add_argument("--output-len", type=int, default=512)
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--layers", type=int, default=40)
    p.add_argument("--heads", type=int, default=40)
    p.add_argument("--head-dim", type=int, default=128)
    p.add_argument("--inter", type=int, default=20480)
    p.add_argument("--vocab", type=int, default=100864)
    p.add_argument("--rotary", type=int, default=32)
    p.add_argument("--top-k", type=int, default=1, help="sampling top_k (1 = greedy, the headline; the reference harness "
                                                         "defaults to 50)")
    p.add_argument("--top-p", type=float, default=0.0, help="sampling top_p (with --top-k 0: the top-p layer)")
    p.add_argument("--full", action="store_true",
                   help="also run the end-to-end request, the profiled roofline run and the CPU baseline (the four options "
                        "below trim a --full run; a plain run does none of these)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-e2e", action="store_true")
    p.add_argument("--profile-steps", type=int, default=48)
    p.add_argument("--no-pmc", action="store_true",
                   help="do not measure the layer kernel's HBM traffic with a `rocprofv3 --pmc` pass of a child process (N = 1)")
    p.add_argument("--fake-tp", type=int, default=0,
                   help="timing aid: run rank 0's shard of a TP=N model in ONE process over a 1-rank communicator "
                        "(no peers: outputs are meaningless, the JSON line is marked invalid)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the measured request's outputs (what the caller receives) as DIR/<name>.npy (rank 0)")
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0:
        p.error("--steps must be >= 1 and --warmup >= 0")
    if not a.full:
        a.no_cpu_baseline = a.no_e2e = a.no_pmc = True
        a.profile_steps = 0
    return a


def synth_weights(a, tp, dev):
    """CodeFuse-13B-shaped synthetic shard in the reference's weight-list order."""
    L, H, I, V = a.layers, a.heads * a.head_dim, a.inter, a.vocab
    hl, il = H // tp, I // tp
    g = torch.Generator(device=dev).manual_seed(1234)
    h16 = dict(dtype=torch.float16, device=dev)

    def rn(*shape, std=0.02, mean=0.0):
        return (torch.randn(*shape, generator=g, device=dev) * std + mean).to(torch.float16)

    groups = [[] for _ in range(12)]
    int8_w = [[] for _ in range(4)]
    scales = [[] for _ in range(4)]
    shapes = [(H, 3 * hl), (hl, H), (H, il), (il, H)]
    empty = torch.empty(0, **h16)
    for _ in range(L):
        groups[0].append(rn(H))
        groups[1].append(rn(H, mean=1.0))
        groups[3].append(rn(3 * hl))
        groups[5].append(empty)
        groups[7].append(rn(il))
        groups[9].append(rn(H))
        groups[10].append(rn(H))
        groups[11].append(rn(H, mean=1.0))
        for i, (K, N) in enumerate(shapes):
            gi = (2, 4, 6, 8)[i]
            if a.dtype == "int8":
                # the tile layout is a permutation of the matrix: uniform random bytes ARE a uniform random int8 matrix
                q = torch.randint(1, 256, (K, N), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
                int8_w[i].append(q.view(torch.int8))
                scales[i].append((torch.rand(N, generator=g, device=dev) * 2e-4 + 1e-4).to(torch.float16))
                groups[gi].append(empty)
            else:
                groups[gi].append(rn(K, N))
    weights = [t for grp in groups for t in grp]
    weights += [rn(V, H), rn(H, mean=1.0), rn(H), rn(V, H)]
    return weights, [t for grp in int8_w for t in grp], [t for grp in scales for t in grp]


def bytes_per_token(a, tp, t_mean):
    L, H, I, V = a.layers, a.heads * a.head_dim, a.inter, a.vocab
    w = 1 if a.dtype == "int8" else 2
    return (L * (4 * H * H + 2 * H * I) * w + V * H * 2 + 2 * L * t_mean * H * 2 * a.batch) / tp


def cpu_baseline(a, budget_s=25.0, max_steps=8):
    """Oracle (CPU restatement, kind "port") on the FULL model: all L layers of CodeFuse-13B-shaped weight-only int8
    (13.1 GB of int8 weights in host RAM, every layer its own random matrices), KV caches pre-filled to the prompt
    length with synthetic rows, then whole decode steps -- L decoder layers + final LayerNorm + the V x H LM head +
    greedy arg-max -- on all host cores: one warm-up step, then up to `max_steps` timed steps or `budget_s` seconds,
    whichever comes first (workload B)."""
    from oracle import oracle as orc
    Lc = a.layers
    H, I, nh, dh, V = a.heads * a.head_dim, a.inter, a.heads, a.head_dim, a.vocab
    rng = np.random.default_rng(0)
    int8 = a.dtype == "int8"

    def rand_q(K, N):  # uniform int8 in [-127, 127] at memory speed
        q = np.frombuffer(rng.bytes(K * N), dtype=np.int8).reshape(K, N).copy()
        q[q == -128] = 0
        return q

    layers = []
    ones, zeros = np.ones(H, np.float32), np.zeros(H, np.float32)
    for _ in range(Lc):
        lay = dict(ln1_g=ones, ln1_b=zeros, ln2_g=ones, ln2_b=zeros, qkv_b=np.zeros(3 * H, np.float32),
                   ffn1_b=np.zeros(I, np.float32), ffn2_b=zeros)
        for name, (K, N) in dict(qkv=(H, 3 * H), out=(H, H), ffn1=(H, I), ffn2=(I, H)).items():
            if int8:
                lay[name + "_q"] = rand_q(K, N)
                lay[name + "_s"] = np.full(N, 2e-4, np.float32)
            else:
                lay[name + "_w"] = rand_q(K, N).astype(np.float32) * np.float32(2e-4)
        layers.append(lay)
    head = rand_q(V, H).astype(np.float32) * np.float32(1e-3)
    glob = dict(wte=head, final_ln_g=ones, final_ln_b=zeros, lm_head=head)
    cfg = dict(head_num=nh, size_per_head=dh, inter_size=I, num_layer=Lc, vocab_size=V, rotary_dim=a.rotary, end_id=2,
               int8_mode=1 if int8 else 0, fp16=1)
    m = orc.Model(cfg, layers, glob)
    t = a.prompt_len
    s_max = t + max_steps + 2
    kc = rng.standard_normal((Lc, 1, nh, s_max, dh), dtype=np.float32) * np.float32(0.5)
    vc = rng.standard_normal((Lc, 1, nh, s_max, dh), dtype=np.float32) * np.float32(0.5)
    zero1, mask = np.zeros(1, np.int32), np.zeros((1, s_max), np.uint8)
    fin = np.zeros(1, np.uint8)

    def one_step(tok, pos):
        x = head[tok:tok + 1]  # embedding row (wte)
        y = m.decoder_step(x, kc, vc, np.array([pos], np.int32), zero1, mask, fin, pos + 1)
        logits = orc.lm_head(orc.layernorm(y, ones, zeros), head)
        return int(np.argmax(logits[0]))

    tok = one_step(3, t)  # warm-up (page faults, thread pool)
    t0 = time.time()
    reps = 0
    while reps < max_steps and (reps == 0 or time.time() - t0 < budget_s):
        tok = one_step(tok, t + 1 + reps)
        reps += 1
    dt = (time.time() - t0) / reps
    return {"value": 1.0 / dt, "unit": "tokens/s", "cores": int(orc.lib().orc_num_threads()), "kind": "port",
            "sample": f"{reps} whole decode steps (all {Lc} layers of the {'int8' if int8 else 'fp16'} model + final LN + "
                      f"{V}x{H} LM head + arg-max) at KV length {t + 1}..{t + reps}, bs=1, after one warm-up step; "
                      f"oracle/ftcf_oracle.c", "s_per_step": dt}


def live_traffic(a):
    """HBM bytes of one k_decode_persistent launch from the PMC counters, measured by THIS invocation: a child process runs the very
    same request (all 512 tokens: the launches' mean KV length is the request's) under `rocprofv3 --pmc FETCH_SIZE --kernel-trace`
    -- its own pass, no other trace domain, as MI355X_MICROARCH.md's HBM section prescribes -- and the per-dispatch counter is
    averaged over the launches that ran the layers (the two table-building launches over no layers are short).  FETCH_SIZE counts
    KiB and is half the bytes on gfx950 (the guide's correction): bytes = value * 1024 * 2.  Returns (bytes, launches, avg us) or
    None (no rocprofv3, a nested profiler, a failed pass)."""
    import glob
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe) or any(k.startswith("ROCPROF") or k.startswith("ROCP_") for k in os.environ):
        return None
    tmp = tempfile.mkdtemp(prefix="ftcf_pmc_", dir="/tmp")
    cmd = [exe, "--pmc", "FETCH_SIZE", "--kernel-trace", "-d", tmp, "-o", "p", "--", sys.executable, os.path.abspath(__file__),
           "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-e2e", "--no-cpu-baseline", "--profile-steps", "0", "--no-pmc",
           "--dtype", a.dtype, "--prompt-len", str(a.prompt_len), "--output-len", str(a.output_len), "--batch", str(a.batch),
           "--layers", str(a.layers), "--heads", str(a.heads), "--head-dim", str(a.head_dim), "--inter", str(a.inter),
           "--vocab", str(a.vocab), "--rotary", str(a.rotary)]
    try:
        env = dict(os.environ, TMPDIR="/tmp")
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        subprocess.run(cmd, cwd="/tmp", env=env, timeout=180, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
        dbs = glob.glob(os.path.join(tmp, "**", "*results.db"), recursive=True)
        c = sqlite3.connect(dbs[0])
        tabs = [r[0] for r in c.execute("select name from sqlite_master where type='table'")]
        T = lambda pre: [t for t in tabs if t.startswith(pre)][0]  # noqa: E731
        disp, sym, pmc, info = T("rocpd_kernel_dispatch"), T("rocpd_info_kernel_symbol"), T("rocpd_pmc_event"), T("rocpd_info_pmc")
        scols = [r[1] for r in c.execute(f"pragma table_info({sym})")]
        name_col = "kernel_name" if "kernel_name" in scols else "display_name"
        q = (f"select count(*), avg(e.value), avg(d.end - d.start) from {pmc} e join {disp} d on e.event_id = d.event_id "
             f"join {sym} s on d.kernel_id = s.id join {info} i on e.pmc_id = i.id "
             f"where i.name = 'FETCH_SIZE' and s.{name_col} like '%k_decode_persistent%' and (d.end - d.start) > 200000")
        n, kb, dur = c.execute(q).fetchone()
        c.close()
        if not n or not kb:
            return None
        return float(kb) * 1024.0 * 2.0, int(n), float(dur) / 1e3
    except Exception:  # noqa: BLE001  (the bench line falls back to the committed pass and says so)
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    a = parse()
    # RCCL prints a version banner through C stdio on stdout (flushed at exit, i.e. after our line): keep fd 1 clean for
    # the ONE JSON line by sending everything else that writes to stdout to stderr
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    sys.stdout = os.fdopen(os.dup(2), "w")
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    import torch.distributed as dist
    group = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        group = dist.group.WORLD

    from fastertransformer4codefuse_amd import capi
    from fastertransformer4codefuse_amd.gptneox_op import GptNeoXOp
    tp = world
    if a.fake_tp > 1:
        assert world == 1
        tp = a.fake_tp
        os.environ["FTCF_FAKE_TP"] = "1"
        group = object()  # any non-None token: the op only hands it to init_tensor_parallel_comm
    H = a.heads * a.head_dim
    weights, int8_w, scales = synth_weights(a, tp, dev)
    end_id = 2
    op = GptNeoXOp(group, rank, a.heads, a.head_dim, a.inter, a.layers, a.vocab, a.rotary, 0, end_id, tp, 1,
                   1 if a.dtype == "int8" else 0, 2048, True, weights, int8_w, scales)
    B, S = a.batch, a.prompt_len
    out_len = max(a.output_len, a.steps + a.warmup)  # K timed steps + W warm-up steps always fit in the request
    # the timed window inside the request: K steps centred on output token out_len / 2 (KV length S + out_len / 2 = the
    # request's mean), W untimed steps right before it; the rest of the request runs untimed around the window
    steps, warmup = a.steps, a.warmup
    first = max(warmup, min(out_len - steps, out_len // 2 - steps // 2))  # output index of the first timed step
    pre, post = first - warmup, out_len - first - steps
    gi = torch.Generator().manual_seed(42)
    ids = torch.randint(3, a.vocab, (B, S), generator=gi, dtype=torch.int32).to(dev)
    lens = torch.full((B,), S, dtype=torch.int32, device=dev)
    total = S + out_len
    out_ids = torch.empty((B, 1, total), dtype=torch.int32, device=dev)
    seq = torch.empty((B, 1), dtype=torch.int32, device=dev)
    cum = torch.empty((B, 1), dtype=torch.float32, device=dev)
    top_k = np.array([a.top_k], np.int32)
    top_p = np.array([a.top_p], np.float32)
    minlen = np.array([out_len], np.int32)  # end_id cannot be sampled: all steps run

    def make_args(olen):
        fa = capi.ForwardArgs()
        fa.input_ids, fa.input_lengths = ids.data_ptr(), lens.data_ptr()
        fa.batch_size, fa.max_input_len, fa.output_len, fa.beam_width = B, S, olen, 1
        fa.top_k, fa.n_top_k = top_k.ctypes.data, 1
        if a.top_p > 0:
            fa.top_p, fa.n_top_p = top_p.ctypes.data, 1
        fa.min_length, fa.n_min_length = minlen.ctypes.data, 1
        fa.return_cum_log_probs = 1  # codefuse_example.py:745
        fa.output_ids, fa.sequence_lengths, fa.cum_log_probs = out_ids.data_ptr(), seq.data_ptr(), cum.data_ptr()
        return fa

    L = capi.lib()

    def barrier():
        if world > 1:
            dist.barrier()

    def run_steps(n):
        if n > 0:
            done = C.c_int(0)
            capi.check(L.ftcf_gptneox_step(op._h, n, C.byref(done)))
            assert done.value == n, f"only {done.value} of {n} steps ran"

    # A tensor-parallel decode that cannot complete its in-kernel exchange on this box (every spin is bounded) makes
    # finish() raise on EVERY rank and pins the engines to the RCCL path: the request is then simply run again.
    fallback_note = None

    def with_fallback(fn):
        nonlocal fallback_note
        try:
            return fn()
        except capi.FtcfError as e:
            if "gave up" not in str(e):
                raise
            fallback_note = str(e)
            return fn()

    # ---- untimed: one short request to warm every kernel / allocation ----
    fa = make_args(out_len)

    def warm_request():
        capi.check(L.ftcf_gptneox_begin(op._h, C.byref(fa)))
        capi.check(L.ftcf_gptneox_step(op._h, 2, None))
        capi.check(L.ftcf_gptneox_finish(op._h))

    with_fallback(warm_request)

    # ---- the measured request ----
    def measured_request():
        torch.cuda.synchronize()
        barrier()
        tp0 = time.perf_counter()
        capi.check(L.ftcf_gptneox_begin(op._h, C.byref(fa)))  # 1024-token prefill through the real context path
        torch.cuda.synchronize()
        pw = (time.perf_counter() - tp0) * 1e3
        run_steps(pre)
        run_steps(warmup)
        torch.cuda.synchronize()
        barrier()
        ta = time.perf_counter()
        run_steps(steps)
        torch.cuda.synchronize()
        barrier()
        tb = time.perf_counter()
        run_steps(post)
        capi.check(L.ftcf_gptneox_finish(op._h))
        return pw, ta, tb

    prefill_wall_ms, t0, t1 = with_fallback(measured_request)
    # what the measured request handed back (the requests below write the same buffers): ids as float64 (exact)
    outputs = {"output_ids": out_ids.cpu().numpy().astype(np.float64),
               "sequence_lengths": seq.cpu().numpy().astype(np.float64),
               "cum_log_probs": cum.cpu().numpy().astype(np.float32)}
    elapsed = torch.tensor([t1 - t0], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    elapsed = float(elapsed.item())
    st = op.stats()

    # ---- end-to-end latency of the whole request (prefill + out_len tokens), the reference README's metric ----
    e2e_ms = e2e_decode_tok_s = None
    if not a.no_e2e:
        torch.cuda.synchronize()
        barrier()
        t2 = time.perf_counter()
        capi.check(L.ftcf_gptneox_forward(op._h, C.byref(fa)))
        torch.cuda.synchronize()
        barrier()
        e2e_ms = (time.perf_counter() - t2) * 1e3
        se = op.stats()
        e2e_decode_tok_s = se["decode_steps"] * B / (se["decode_ms"] * 1e-3) if se["decode_ms"] > 0 else None

    # ---- roofline leg: HIP events around every weight-streaming launch of a short profiled run ----
    KIND_NAMES = {0: "k_ln_gemv_group (LN1 -> QKV weight stream)", 1: "k_gemv_chunked (out-proj + FFN2 weight stream)",
                  2: "k_lm_head", 3: "k_mmha_ln_gemv (attention || LN2 -> FFN1 weight stream)",
                  4: "k_decode_persistent (all layers of one token: weights + KV cache)",
                  5: "k_gemm_smallm_burst (batched decode: one weight matrix per launch, read once for all rows; the attention branch "
                     "and the FFN branch of a layer run on two streams, so a launch shares the HBM with its neighbour)"}
    roof = None
    if a.profile_steps > 0:
        # the profiled steps sit at the same place of the request as the timed window (same KV lengths)
        nprof = min(a.profile_steps, out_len)
        pfirst = max(0, min(out_len - nprof, out_len // 2 - nprof // 2))
        fa2 = make_args(out_len)
        capi.check(L.ftcf_gptneox_begin(op._h, C.byref(fa2)))
        run_steps(pfirst)
        op.set_profiling(True)
        run_steps(nprof)
        capi.check(L.ftcf_gptneox_finish(op._h))
        ps = op.stats()
        op.set_profiling(False)
        if ps["decode_path"] == 3:  # (the launches of kind 4 were the rows kernel's)
            KIND_NAMES[4] = "k_decode_rows (all layers of one token for 3..16 rows: weights + KV cache)"
        if ps["gemv_launches"] > 0:
            per_launch_bytes = ps["gemv_bytes"] / ps["gemv_launches"]
            avg_ms = ps["gemv_ms_sum"] / ps["gemv_launches"]
            achieved = per_launch_bytes / (avg_ms * 1e-3) / 1e9
            # HBM traffic of that kernel from the PMC pass recorded under profiles/ (collected in its own rocprofv3 run, as
            # the counters cannot ride along with this timing run); only quoted when it was measured on this very config
            traffic = traffic_source = None
            live = None
            if (world == 1 and a.fake_tp <= 1 and not a.no_pmc and ps["gemv_kind"] == 4 and a.batch == 1):
                live = live_traffic(a)
            try:
                import glob
                pm = json.load(open(sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_int8_tp1.json")))[-1]))
                c = pm["config"]
                if (ps["gemv_kind"] == 4 and a.fake_tp <= 1 and a.dtype == c["dtype"] and world == c["tensor_parallel"] and a.layers == c["layers"]
                        and H == c["hidden"] and a.inter == c["inter"] and a.batch == 1):
                    traffic = pm["traffic_bytes_per_launch"]
                    traffic_source = ("profiles/" + os.path.basename(sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_int8_tp1.json")))[-1])
                                      + ": FETCH_SIZE x 2 (gfx950 correction) from a separate `rocprofv3 --pmc` pass over this very "
                                        "command, NOT measured in this run")
            except (OSError, KeyError, ValueError, IndexError):
                pass
            if live is not None:
                traffic = live[0]
                traffic_source = (f"measured by this invocation: a child process ran the same request under `rocprofv3 --pmc FETCH_SIZE "
                                  f"--kernel-trace` (its own pass); FETCH_SIZE x 1024 x 2 (gfx950 correction) averaged over {live[1]} "
                                  f"launches of the kernel ({live[2]:.1f} us each under the counters)")
            roof = {"bound": "hbm", "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0,
                    "traffic": traffic, "traffic_source": traffic_source, "kernel": KIND_NAMES.get(ps["gemv_kind"], "?"), "bytes_per_launch": per_launch_bytes, "avg_launch_us": avg_ms * 1e3,
                    "launches": ps["gemv_launches"],
                    "measured_over": f"{nprof} profiled decode steps (output tokens {pfirst}..{pfirst + nprof - 1}), "
                                     "HIP events on the engine's stream around every launch of that kernel"}

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return
    if a.dump_outputs:
        os.makedirs(a.dump_outputs, exist_ok=True)
        for name, arr in outputs.items():
            np.save(os.path.join(a.dump_outputs, name + ".npy"), arr)
    tok_s = steps * B / elapsed
    t_mean = S + first + steps / 2.0  # mean KV length of the timed steps
    bpt = bytes_per_token(a, tp, t_mean)  # HBM bytes of ONE step (weights once, K/V rows of all B rows)
    res = {
        "metric": "decode_tokens_per_sec", "value": tok_s, "unit": "tokens/s", "n_gpus": world, "steps": steps,
        "warmup": warmup, "ms_per_step": elapsed / steps * 1e3, "higher_is_better": True, "scaling": "strong",
        # the reference's README quotes 75 tok/s (1xA100) / 98 tok/s (2xA100 TP=2) for int8, 48 / 77 fp16
        "vs_baseline": (tok_s / {("int8", 1): 75.0, ("int8", 2): 98.0, ("fp16", 1): 48.0, ("fp16", 2): 77.0}[(a.dtype, world)]
                        if (a.dtype, world) in (("int8", 1), ("int8", 2), ("fp16", 1), ("fp16", 2))
                        and a.layers == 40 and a.batch == 1 else None),
        "dtype": "f16", "data": "synthetic",
        "config": {"workload": f"CodeFuse-13B-shaped GPT-NeoX (L={a.layers},H={H},I={a.inter},V={a.vocab}) "
                               f"{'weight-only int8' if a.dtype == 'int8' else 'fp16'} TP={tp}, bs={B}, "
                               f"{S}-in/{out_len}-out {'greedy' if a.top_k == 1 else 'top-k ' + str(a.top_k)} decode", "weights": a.dtype, "tensor_parallel": tp,
                   "batch": B, "prompt_len": S, "output_len": out_len, "return_cum_log_probs": 1,
                   "timed_window": f"output tokens {first}..{first + steps - 1} of the {S}-in/{out_len}-out request "
                                   f"(KV length {S + first}..{S + first + steps - 1}, mean {t_mean:g}; request mean "
                                   f"{S + out_len / 2:g}); {pre} + {warmup} steps before and {post} after run untimed"},
        "prefill_ms": st["prefill_ms"], "prefill_wall_ms": prefill_wall_ms, "e2e_ms": e2e_ms,
        "e2e_decode_tokens_per_sec": e2e_decode_tok_s,  # all out_len tokens of the end-to-end run (HIP events)
        # context phase: 2*(4H^2+2HI)*L*S*B GEMM flops + 2*L*S^2*H*B causal attention flops, per GPU, vs the 2.5 PFLOP/s
        # dense fp16 MFMA peak (MI355X_MICROARCH.md)
        "prefill_tflops_per_gpu": ((2.0 * (4.0 * H * H + 2.0 * H * a.inter) * a.layers * S * B
                                    + 2.0 * a.layers * S * S * H * B) / tp) / (st["prefill_ms"] * 1e-3) / 1e12,
        "prefill_mfma_frac": ((2.0 * (4.0 * H * H + 2.0 * H * a.inter) * a.layers * S * B
                               + 2.0 * a.layers * S * S * H * B) / tp) / (st["prefill_ms"] * 1e-3) / 2.5e15,
        "hbm_bytes_per_step_per_gpu": bpt,
        # whole-step HBM roofline (8 TB/s), incl. KV + fp16 LM head: bytes of one step x steps per second
        "path_roofline_frac": bpt * (tok_s / B) / 8e12,
        "roofline": roof,
        # which decode path the timed steps took on rank 0 and how the per-layer all-reduce travelled (the driver's SCALE run
        # reads this to confirm that N ranks were up and whether the in-kernel xGMI exchange or the RCCL fallback ran)
        "tensor_parallel": {"ranks": world if a.fake_tp <= 1 else a.fake_tp, "backend": "rccl" if world > 1 else "none",
                            "decode_path": {0: "per-stage launches", 1: "persistent kernel", 2: "general path",
                                            3: "rows kernel (persistent layers for 3..16 rows)"}.get(
                                st["decode_path"], str(st["decode_path"])),
                            # (one- / two-row kernel: its out-proj / FFN2 stage -- DESIGN.md section 4b)
                            "persistent_p3_layout": ("own groups (one hop at the layer boundary)" if st.get("persist_layout") else
                                                     "K pieces merged by an owner") if st["decode_path"] == 1 else None,
                            "layer_allreduce": ("none" if tp == 1 else
                                                "in-kernel exchange windows (peer-mapped, xGMI stores)"
                                                if st["decode_path"] == 1 else "ncclAllReduce per layer"),
                            # prompt phase: FTCF_PREFILL_OVERLAP unset = decided from data on THIS node (engine.hip
                            # context_decoder_overlapped: one plain and one overlapped prompt phase are timed, the faster form stays)
                            "prefill_overlap": {"mode": os.environ.get("FTCF_PREFILL_OVERLAP", "off"),
                                                "ran_in_the_last_request": bool(st.get("prefill_overlap", 0)),
                                                "trial_ms_plain": st.get("prefill_ms_plain", 0.0),
                                                "trial_ms_overlapped": st.get("prefill_ms_overlapped", 0.0)},
                            # batched decode (4..32 rows): the layer's all-reduce on the side stream under the other micro-batch
                            # (engine.hip.h decoder_overlapped; auto = one plain and one overlapped request timed on THIS node)
                            "decode_overlap": {"mode": os.environ.get("FTCF_DECODE_OVERLAP", "off"),
                                               "ran_in_the_last_request": bool(st.get("decode_overlap", 0)),
                                               "trial_step_ms_plain": st.get("decode_step_ms_plain", 0.0),
                                               "trial_step_ms_overlapped": st.get("decode_step_ms_overlapped", 0.0)},
                            "prompt_phase_allreduces_through_windows": st.get("window_allreduces", 0),
                            "fallback": fallback_note},
    }
    if a.fake_tp > 1:
        res["invalid"] = f"--fake-tp {a.fake_tp}: one rank of a TP={a.fake_tp} job without its peers (timing aid only)"
        res["vs_baseline"] = None
    if world == 1 and not a.no_cpu_baseline and a.dtype != "int8":
        res["cpu_baseline"] = {"skipped": "the CPU leg holds the model as int8 + fp32 scales (13 GB); run --dtype int8"}
    elif world == 1 and not a.no_cpu_baseline:
        try:
            res["cpu_baseline"] = cpu_baseline(a)
        except Exception as e:  # the oracle is only a reported baseline
            res["cpu_baseline"] = {"error": repr(e)}
    os.write(real_stdout, (json.dumps(res) + "\n").encode())
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
