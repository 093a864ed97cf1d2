"""Speculative greedy decoding: what a verify pass costs and what it returns.

The bench.py model (13B-shaped int8, synthetic weights), one request of 1024 prompt tokens and 512 generated ones.  Synthetic
weights do not copy from their prompt, so acceptance is IMPOSED through draft_ids: a first plain run records the greedy
tokens, the speculative runs draft them with every p-th draft replaced by a different token (p = 0: none).  Per K in {2, 4, 8}
and acceptance setting: milliseconds per verify pass (the request's token-loop time minus its plain steps at the plain run's
rate, over its passes), tokens per pass, tokens/s, next to the plain run's; break-even tokens per pass = verify-pass time /
plain step time.  Plain and speculative runs alternate inside the one process, after a warm-up of each shape.

    python tools/bench_speculative.py [--prompt-len 1024] [--out-len 512] [--rounds 3] [--ks 2,4,8] [--every 0,4,2,1]

--scope adds the leg of the wider speculative scope (GptNeoXOp.set_speculative_scope(1)): the same workload as the harness sends
it -- return_cum_log_probs, a stop-word list that never matches and a no-op callback.  The passes of both legs close with
k_verify_slices + k_verify_close: the legs differ only in what the request carries.  Per round the plain run, the scope 0 run and
the scope 1 run follow each other in the one process; a row reports both legs' milliseconds per verify pass (best, and the
spread over the rounds) and tokens/s (profiles/speculative_scope_bench.txt).

--sampled adds the leg of speculative SAMPLING (GptNeoXOp.set_speculative_sampling(1)): the request as the harness sends it with its
top_k = 50, whose passes close with k_verify_topk_slices + k_verify_pick + k_verify_sample_close.  The drafts are the plain SAMPLED
run's tokens (same seed) with every p-th replaced.  Per round the plain greedy run, the greedy scope 1 run, the plain sampled run
and the speculative sampled run follow each other in the one process; a row reports, for the greedy and the sampled leg, the plain
milliseconds per token, milliseconds per verify pass (best and the spread) and tokens/s (profiles/speculative_sampled_bench.txt).
The difference between the two passes is the selection: per row the radix select of 32 slices' k best, a merge and a draw where
the greedy pass keeps an arg max -- what k_topk_decode costs over k_greedy_decode in the plain step.
"""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fastertransformer4codefuse_amd import capi  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--prompt-len", type=int, default=1024)
    p.add_argument("--out-len", type=int, default=512)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--ks", default="2,4,8")
    p.add_argument("--every", default="0,4,2,1", help="corrupt every p-th draft (0: none, 1: all)")
    p.add_argument("--scope", action="store_true", help="add the scope 1 leg (cum_log_probs + stop words + callback) next to scope 0")
    p.add_argument("--sampled", action="store_true", help="the top_k 50 request of the harness under speculative sampling, next to greedy scope 1")
    p.add_argument("--seed", type=int, default=7, help="random_seed of the sampled legs")
    a = p.parse_args()
    capi.require_gpu()
    import bench
    from fastertransformer4codefuse_amd.gptneox_op import GptNeoXOp
    m = types.SimpleNamespace(layers=40, heads=40, head_dim=128, inter=20480, vocab=100864, dtype="int8")
    dev = torch.device("cuda", 0)
    print("device:", torch.cuda.get_device_name(0), flush=True)
    weights, int8_w, scales = bench.synth_weights(m, 1, dev)
    op = GptNeoXOp(None, 0, m.heads, m.head_dim, m.inter, m.layers, m.vocab, 32, 0, 2, 1, 1, 1, 2048, True, weights, int8_w, scales)
    S, out_len = a.prompt_len, a.out_len
    ids = torch.randint(3, m.vocab, (1, S), generator=torch.Generator().manual_seed(42), dtype=torch.int32).to(dev)
    lens = torch.full((1,), S, dtype=torch.int32, device=dev)
    k1 = torch.tensor([1], dtype=torch.int32)

    def run(n_out=out_len, top_k=k1, **kw):
        o = op.forward(ids, lens, n_out, 1, top_k, **kw)
        torch.cuda.synchronize()
        return o[0][0, 0, S:].cpu().tolist(), int(o[1][0, 0].item()) - S, op.stats()

    gen, n_gen, st = run()
    gen = gen[:n_gen]
    print(json.dumps(dict(plain_tokens=n_gen, decode_path=st["decode_path"], note="tokens generated before the end token" if n_gen < out_len else "")),
          flush=True)
    wrong = lambda t: 3 + (t - 3 + 1) % (m.vocab - 3)

    def drafts(every):
        d = [(wrong(t) if every and i % every == every - 1 else t) for i, t in enumerate(gen)]
        return torch.tensor(d + [3] * (out_len - len(d)), dtype=torch.int32, device=dev)

    ks = [int(x) for x in a.ks.split(",") if x]
    every = [int(x) for x in a.every.split(",") if x]
    if a.scope:
        return scope_legs(a, op, run, drafts, gen, n_gen, ks, every, dev)
    if a.sampled:
        return sampled_legs(a, op, run, gen, n_gen, ks, every, dev, m.vocab)
    for K in ks:  # warm-up of each shape (arena, graph capture of the plain step, every kernel's code object)
        run(32)
        run(32, speculative_tokens=K, draft_ids=drafts(0)[:32].contiguous())
    rows = []
    for K in ks:
        for ev in every:
            d = drafts(ev)
            best = None
            for _ in range(a.rounds):
                _, n_p, sp = run()  # plain, then speculative: alternating
                toks, n_s, ss = run(speculative_tokens=K, draft_ids=d)
                plain_ms = sp["decode_ms"] / sp["decode_steps"]
                n_plain = ss["decode_steps"] - ss["spec_accepted"] - ss["spec_steps"]
                pass_ms = (ss["decode_ms"] - n_plain * plain_ms) / max(1, ss["spec_steps"])
                r = dict(K=K, corrupt_every=ev, plain_ms_per_token=round(plain_ms, 4), plain_tok_s=round(1e3 / plain_ms, 1),
                         spec_active=ss["spec_active"], passes=ss["spec_steps"], drafted=ss["spec_drafted"], accepted=ss["spec_accepted"],
                         tokens_per_pass=round((ss["spec_accepted"] + ss["spec_steps"]) / max(1, ss["spec_steps"]), 3),
                         ms_per_pass=round(pass_ms, 4), spec_tok_s=round(ss["decode_steps"] / ss["decode_ms"] * 1e3, 1),
                         break_even_tokens_per_pass=round(pass_ms / plain_ms, 3),
                         speedup=round((ss["decode_steps"] / ss["decode_ms"]) / (sp["decode_steps"] / sp["decode_ms"]), 3),
                         tokens_differ=sum(1 for x, y in zip(toks[:n_s], gen) if x != y) + abs(n_s - n_gen))
                if best is None or r["spec_tok_s"] > best["spec_tok_s"]:
                    best = r
            rows.append(best)
            print(json.dumps(best), flush=True)
    return rows


def scope_legs(a, op, run, drafts, gen, n_gen, ks, every, dev):
    """scope 0 (the bare request) next to scope 1 (the request the harness sends), alternating"""
    never = torch.tensor([[[2, 2], [2, -1]]], dtype=torch.int32, device=dev)  # one word, the end token twice: never completes
    wide = dict(return_cum_log_probs=1, stop_words_list=never, callback=lambda d: None)

    def leg(scope, plain_ms, **kw):
        op.set_speculative_scope(scope)
        toks, n_s, ss = run(**kw)
        n_plain = ss["decode_steps"] - ss["spec_accepted"] - ss["spec_steps"]
        pass_ms = (ss["decode_ms"] - n_plain * plain_ms) / max(1, ss["spec_steps"])
        return dict(spec_active=ss["spec_active"], passes=ss["spec_steps"], accepted=ss["spec_accepted"], ms_per_pass=pass_ms,
                    tok_s=ss["decode_steps"] / ss["decode_ms"] * 1e3,
                    tokens_differ=sum(1 for x, y in zip(toks[:n_s], gen) if x != y) + abs(n_s - n_gen))

    for K in ks:
        op.set_speculative_scope(1)
        run(32, speculative_tokens=K, draft_ids=drafts(0)[:32].contiguous(), **wide)
    rows = []
    for K in ks:
        for ev in every:
            d = drafts(ev)
            legs = {0: [], 1: []}
            plain = []
            for _ in range(a.rounds):
                op.set_speculative_scope(0)
                _, _, sp = run()
                plain_ms = sp["decode_ms"] / sp["decode_steps"]
                plain.append(plain_ms)
                legs[0].append(leg(0, plain_ms, speculative_tokens=K, draft_ids=d))
                legs[1].append(leg(1, plain_ms, speculative_tokens=K, draft_ids=d, **wide))
            row = dict(K=K, corrupt_every=ev, plain_ms_per_token=[round(min(plain), 4), round(max(plain), 4)])
            for sc in (0, 1):
                ms = [r["ms_per_pass"] for r in legs[sc]]
                row[f"scope{sc}"] = dict(spec_active=legs[sc][0]["spec_active"], passes=legs[sc][0]["passes"], accepted=legs[sc][0]["accepted"],
                                         ms_per_pass_min=round(min(ms), 4), ms_per_pass_max=round(max(ms), 4),
                                         tok_s_best=round(max(r["tok_s"] for r in legs[sc]), 1),
                                         tokens_differ=max(r["tokens_differ"] for r in legs[sc]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    op.set_speculative_scope(0)
    return rows


def sampled_legs(a, op, run, gen, n_gen, ks, every, dev, V):
    """the harness's request greedy at scope 1 next to the same request with its top_k = 50 under speculative sampling, alternating"""
    never = torch.tensor([[[2, 2], [2, -1]]], dtype=torch.int32, device=dev)  # one word, the end token twice: never completes
    wide = dict(return_cum_log_probs=1, stop_words_list=never, callback=lambda d: None)
    k50 = dict(top_k=torch.tensor([50], dtype=torch.int32), random_seed=torch.tensor([a.seed], dtype=torch.int64))
    out_len = a.out_len
    op.set_speculative_scope(1)
    op.set_speculative_sampling(1)
    s_gen, s_n, _ = run(**k50, **wide)
    s_gen = s_gen[:s_n]
    print(json.dumps(dict(sampled_plain_tokens=s_n, not_the_greedy_token=sum(1 for x, y in zip(s_gen, gen) if x != y))), flush=True)
    wrong = lambda t: 3 + (t - 3 + 1) % (V - 3)

    def drafts(tokens, ev):
        d = [(wrong(t) if ev and i % ev == ev - 1 else t) for i, t in enumerate(tokens)]
        return torch.tensor(d + [3] * (out_len - len(d)), dtype=torch.int32, device=dev)

    def leg(tokens, n_tokens, plain_ms, **kw):
        toks, n_s, ss = run(**kw)
        n_plain = ss["decode_steps"] - ss["spec_accepted"] - ss["spec_steps"]
        pass_ms = (ss["decode_ms"] - n_plain * plain_ms) / max(1, ss["spec_steps"])
        return dict(spec_active=ss["spec_active"], passes=ss["spec_steps"], accepted=ss["spec_accepted"], ms_per_pass=pass_ms,
                    tok_s=ss["decode_steps"] / ss["decode_ms"] * 1e3,
                    tokens_differ=sum(1 for x, y in zip(toks[:n_s], tokens) if x != y) + abs(n_s - n_tokens))

    for K in ks:  # warm-up of each shape
        run(32, speculative_tokens=K, draft_ids=drafts(gen, 0)[:32].contiguous(), **wide)
        run(32, speculative_tokens=K, draft_ids=drafts(s_gen, 0)[:32].contiguous(), **k50, **wide)
    rows = []
    for K in ks:
        for ev in every:
            dg, ds = drafts(gen, ev), drafts(s_gen, ev)
            legs = {"greedy": [], "sampled": []}
            plain = {"greedy": [], "sampled": []}
            for _ in range(a.rounds):
                sp = run(**wide)[2]
                plain["greedy"].append(sp["decode_ms"] / sp["decode_steps"])
                legs["greedy"].append(leg(gen, n_gen, plain["greedy"][-1], speculative_tokens=K, draft_ids=dg, **wide))
                sp = run(**k50, **wide)[2]
                plain["sampled"].append(sp["decode_ms"] / sp["decode_steps"])
                legs["sampled"].append(leg(s_gen, s_n, plain["sampled"][-1], speculative_tokens=K, draft_ids=ds, **k50, **wide))
            row = dict(K=K, corrupt_every=ev)
            for name in ("greedy", "sampled"):
                ms = [r["ms_per_pass"] for r in legs[name]]
                row[name] = dict(plain_ms_per_token=[round(min(plain[name]), 4), round(max(plain[name]), 4)],
                                 plain_tok_s=round(1e3 / min(plain[name]), 1), spec_active=legs[name][0]["spec_active"],
                                 passes=legs[name][0]["passes"], accepted=legs[name][0]["accepted"], ms_per_pass_min=round(min(ms), 4),
                                 ms_per_pass_max=round(max(ms), 4), tok_s_best=round(max(r["tok_s"] for r in legs[name]), 1),
                                 tokens_differ=max(r["tokens_differ"] for r in legs[name]))
            row["sampled_minus_greedy_ms_per_pass"] = round(row["sampled"]["ms_per_pass_min"] - row["greedy"]["ms_per_pass_min"], 4)
            row["sampled_minus_greedy_plain_ms"] = round(row["sampled"]["plain_ms_per_token"][0] - row["greedy"]["plain_ms_per_token"][0], 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
    op.set_speculative_scope(0)
    op.set_speculative_sampling(0)
    return rows


if __name__ == "__main__":
    main()
