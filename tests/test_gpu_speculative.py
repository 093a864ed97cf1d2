"""-m gpu: speculative greedy decoding through GptNeoXOp: the tokens with speculative_tokens = K are those
without it and the oracle's, whatever the drafts are; the counters follow a host simulation of the accept rule; requests the
feature does not cover run exactly as before."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.helpers import load_tiny, quantize_layers, random_model, shard_weights, weight_list_to_layers
from tests.test_gpu_engine import MID

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


@pytest.fixture(scope="module")
def tiny():
    cfg, w, z = load_tiny()
    layers, glob = weight_list_to_layers(cfg, w)
    return cfg, w, layers, glob, z


def draft_ref(t, K, N):
    """The n-gram lookup's definition (include/ftcf.h ftcf_ngram_draft)."""
    n = len(t)
    for g in range(min(N, n - 1), 0, -1):
        for s in range(n - g - 1, -1, -1):
            if t[s:s + g] == t[n - g:n]:
                return t[s + g:min(s + g + K, n)]
    return []


def simulate(prompt, gen, K, N, out_len, draft_ids=None):
    """The engine's loop over the tokens `gen` greedy decoding produces (the end token included when it was hit): a step whose
    drafts -- draft_ids[j : j + K] cut at the first negative id, or the n-gram lookup -- are not empty is a verify pass over
    min(drafts, K, out_len - j - 1) of them; it emits the drafts that match and the model's own next token, cut after the end
    token.  The first step of a request never drafts (a prompt longer than one token has no decoder pass there).
    -> (verify passes, drafts proposed, drafts accepted, tokens emitted per pass)."""
    hist, j = list(prompt), 0
    passes = drafted = accepted = 0
    per_pass = []
    while j < len(gen):
        if draft_ids is not None:
            d = []
            for t in draft_ids[j:j + K]:
                if t < 0:
                    break
                d.append(int(t))
        else:
            d = draft_ref(hist, K, N)
        nd = 0 if j == 0 else min(len(d), K, out_len - j - 1)
        e = 0
        if nd > 0:
            passes += 1
            drafted += nd
            while True:
                tok = gen[j + e]
                e += 1
                hit = e - 1 < nd and d[e - 1] == tok
                accepted += 1 if hit else 0
                if not hit or j + e >= len(gen) or e > nd:
                    break
            per_pass.append(e)
        else:
            e = 1
        hist += gen[j:j + e]
        j += e
    return passes, drafted, accepted, per_pass


def forward(op, prompt, out_len, **kw):
    ids = torch.tensor([list(prompt)], dtype=torch.int32, device="cuda")
    lens = torch.tensor([len(prompt)], dtype=torch.int32, device="cuda")
    d = kw.pop("draft_ids", None)
    if d is not None:
        d = torch.tensor(list(d), dtype=torch.int32, device="cuda")
    o = op.forward(ids, lens, out_len, 1, torch.tensor([1], dtype=torch.int32), draft_ids=d, **kw)
    torch.cuda.synchronize()
    return o[0][0, 0].cpu().numpy().tolist(), int(o[1][0, 0].item()), op.stats()


def oracle_run(cfg, layers, glob, int8_mode, prompt, out_len):
    lay = quantize_layers(layers) if int8_mode else layers
    o = orc.Model(dict(cfg, fp16=1, int8_mode=int8_mode), lay, glob).generate(np.array([prompt], dtype=np.int32), [len(prompt)], out_len)
    ids, n = o["output_ids"][0].tolist(), int(o["sequence_lengths"][0])
    return ids, n, ids[len(prompt):n]


def repeating_prompt(V, seed=1):
    """A random block twice, then its first tokens: the continuation of an earlier occurrence is there to be looked up."""
    blk = np.random.RandomState(seed).randint(3, V, size=12).tolist()
    return blk + blk + blk[:4]


@pytest.mark.parametrize("int8_mode", [0, 1])
@pytest.mark.parametrize("K", [1, 4, 15])
def test_tiny_ngram_drafts_give_the_plain_tokens_and_some_are_accepted(gh, tiny, K, int8_mode):
    cfg, w, layers, glob, z = tiny
    prompt, out_len = repeating_prompt(cfg["vocab_size"]), 24
    o_ids, o_len, gen = oracle_run(cfg, layers, glob, int8_mode, prompt, out_len)
    passes, drafted, accepted, _ = simulate(prompt, gen, K, 3, out_len)
    assert accepted > 0, "the chosen prompt's greedy continuation never agrees with an n-gram draft: pick another seed"
    op = gh.make_op(cfg, w, int8_mode=int8_mode)
    p_ids, p_len, st = forward(op, prompt, out_len)
    assert st["spec_active"] == 0 and st["spec_steps"] == 0
    s_ids, s_len, st = forward(op, prompt, out_len, speculative_tokens=K)
    assert (s_ids, s_len) == (p_ids, p_len) == (o_ids, o_len)
    assert st["spec_active"] == 1 and st["spec_accepted"] > 0 and st["decode_steps"] == len(gen)
    assert (st["spec_steps"], st["spec_drafted"], st["spec_accepted"]) == (passes, drafted, accepted)
    # a longer n-gram and a shorter one: the same tokens
    for N in (1, 8):
        s_ids, s_len, st = forward(op, prompt, out_len, speculative_tokens=K, speculative_ngram=N)
        assert (s_ids, s_len) == (o_ids, o_len)
        assert (st["spec_steps"], st["spec_drafted"], st["spec_accepted"]) == simulate(prompt, gen, K, N, out_len)[:3]


@pytest.mark.parametrize("int8_mode", [0, 1])
@pytest.mark.parametrize("K", [1, 4, 15])
def test_tiny_caller_drafts_intact_corrupted_and_all_wrong(gh, tiny, K, int8_mode):
    cfg, w, layers, glob, z = tiny
    V, prompt, out_len = cfg["vocab_size"], z["prompt"].tolist(), 23  # (23: not a multiple of K + 1 for K = 1, 4, 15)
    o_ids, o_len, gen = oracle_run(cfg, layers, glob, int8_mode, prompt, out_len)
    assert len(gen) == out_len
    op = gh.make_op(cfg, w, int8_mode=int8_mode)
    p_ids, p_len, _ = forward(op, prompt, out_len)
    wrong = lambda t: 3 + (t - 3 + 1) % (V - 3)  # a different token, never the end token
    cases = {"intact": list(gen), "every third wrong": [wrong(t) if i % 3 == 2 else t for i, t in enumerate(gen)],
             "all wrong": [wrong(t) for t in gen]}
    for name, d in cases.items():
        s_ids, s_len, st = forward(op, prompt, out_len, speculative_tokens=K, draft_ids=d)
        assert (s_ids, s_len) == (p_ids, p_len) == (o_ids, o_len), name
        passes, drafted, accepted, per_pass = simulate(prompt, gen, K, 3, out_len, draft_ids=d)
        assert st["spec_active"] == 1 and st["decode_steps"] == out_len
        assert (st["spec_steps"], st["spec_drafted"], st["spec_accepted"]) == (passes, drafted, accepted), name
        if name == "intact":
            assert st["spec_accepted"] == st["spec_drafted"] > 0
        if name == "all wrong":
            assert st["spec_accepted"] == 0 and st["spec_steps"] == out_len - 2  # every pass emits one token; the first and the last step are plain
            assert all(e == 1 for e in per_pass)


@pytest.mark.parametrize("int8_mode", [0, 1])
def test_end_token_inside_an_accepted_run_and_the_edges_of_a_request(gh, tiny, int8_mode):
    cfg, w, layers, glob, z = tiny
    prompt = z["prompt"].tolist()
    _, _, gen = oracle_run(cfg, layers, glob, int8_mode, prompt, 12)
    # the end token = the 4th generated token (new at that position): with intact drafts and K = 4 the pass that starts at
    # generated index 1 has accepted it before it sees it
    k = next(i for i in range(3, 12) if gen[i] not in gen[:i] and gen[i] not in prompt)
    cfg2 = dict(cfg, end_id=int(gen[k]))
    o_ids, o_len, gen2 = oracle_run(cfg2, layers, glob, int8_mode, prompt, 12)
    assert gen2 == gen[:k + 1] and o_len == len(prompt) + k + 1
    op = gh.make_op(cfg2, w, int8_mode=int8_mode)
    p_ids, p_len, _ = forward(op, prompt, 12)
    drafts = gen + [5] * 12
    for K in (4, 15):
        s_ids, s_len, st = forward(op, prompt, 12, speculative_tokens=K, draft_ids=drafts[:12])
        assert (s_ids, s_len) == (p_ids, p_len) == (o_ids, o_len)
        assert s_ids[len(prompt) + k + 1:] == [cfg2["end_id"]] * (12 - k - 1)  # end_id padded as always
        assert st["decode_steps"] == k + 1
        assert (st["spec_steps"], st["spec_drafted"], st["spec_accepted"]) == simulate(prompt, gen2, K, 3, 12, draft_ids=drafts[:12])[:3]
    # output_len 1; a one-token prompt; a last pass that the cache's end cuts (K = 15 drafts against 7 positions)
    op = gh.make_op(cfg, w, int8_mode=int8_mode)
    for pr, out_len in ((prompt, 1), (prompt[:1], 9), (prompt, 7), (prompt, 2)):
        o_ids, o_len, g = oracle_run(cfg, layers, glob, int8_mode, pr, out_len)
        p_ids, p_len, _ = forward(op, pr, out_len)
        s_ids, s_len, st = forward(op, pr, out_len, speculative_tokens=15, draft_ids=g + [7] * (out_len - len(g)))
        assert (s_ids, s_len) == (p_ids, p_len) == (o_ids, o_len), (len(pr), out_len)
        assert st["spec_active"] == 1
        assert (st["spec_steps"], st["spec_drafted"], st["spec_accepted"]) == simulate(pr, g, 15, 3, out_len, draft_ids=g)[:3]


@pytest.mark.parametrize("int8_mode", [0, 1])
def test_begin_step_finish_never_overshoots_max_steps(gh, tiny, int8_mode):
    from fastertransformer4codefuse_amd import capi
    cfg, w, layers, glob, z = tiny
    prompt, out_len = z["prompt"].tolist(), 20
    o_ids, o_len, gen = oracle_run(cfg, layers, glob, int8_mode, prompt, out_len)
    op = gh.make_op(cfg, w, int8_mode=int8_mode)
    ids = torch.tensor([prompt], dtype=torch.int32, device="cuda")
    lens = torch.tensor([len(prompt)], dtype=torch.int32, device="cuda")
    drafts = torch.tensor(gen, dtype=torch.int32, device="cuda")
    out_ids = torch.zeros((1, 1, len(prompt) + out_len), dtype=torch.int32, device="cuda")
    seq = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    top_k = np.array([1], np.int32)
    fa = capi.ForwardArgs()
    fa.input_ids, fa.input_lengths = ids.data_ptr(), lens.data_ptr()
    fa.batch_size, fa.max_input_len, fa.output_len, fa.beam_width = 1, len(prompt), out_len, 1
    fa.top_k, fa.n_top_k = top_k.ctypes.data, 1
    fa.output_ids, fa.sequence_lengths = out_ids.data_ptr(), seq.data_ptr()
    fa.speculative_tokens, fa.draft_ids = 4, drafts.data_ptr()
    L = capi.lib()
    done = C.c_int(0)
    capi.check(L.ftcf_gptneox_begin(op._h, C.byref(fa)))
    total = 0
    for n in (3, 1, 2, 4, 100):
        capi.check(L.ftcf_gptneox_step(op._h, n, C.byref(done)))
        assert 1 <= done.value <= n
        if n != 100:
            assert done.value == n  # intact drafts: a pass is cut to what the call may still emit, not dropped
        total += done.value
    assert total == out_len
    capi.check(L.ftcf_gptneox_finish(op._h))
    torch.cuda.synchronize()
    assert out_ids[0, 0].cpu().numpy().tolist() == o_ids and int(seq[0, 0].item()) == o_len
    st = op.stats()
    assert st["spec_active"] == 1 and st["spec_accepted"] == st["spec_drafted"] > 0 and st["decode_steps"] == out_len


def _plain_with_logits(op, prompt, out_len, V):
    ids = torch.tensor([prompt], dtype=torch.int32, device="cuda")
    lens = torch.tensor([len(prompt)], dtype=torch.int32, device="cuda")
    dbg = torch.zeros((out_len, 1, V), dtype=torch.float32, device="cuda")
    o = op.forward(ids, lens, out_len, 1, torch.tensor([1], dtype=torch.int32), _debug_logits=dbg)
    torch.cuda.synchronize()
    return o[0][0, 0].cpu().numpy().tolist(), int(o[1][0, 0].item()), dbg[:, 0].cpu().numpy()


def _same_up_to_a_near_tie(got, ref, logits, S, what):
    """The repository's near-tie rule (tests/test_gpu_batcher_prefix.py): a first difference only where the top-2 logit margin of
    the plain run is <= 1e-2 * max|logit|."""
    for t, (a, b) in enumerate(zip(got[S:], ref[S:])):
        if a != b:
            top2 = np.sort(logits[t])[-2:]
            assert top2[1] - top2[0] <= 1e-2 * np.abs(logits[t]).max(), (what, t)
            return False
    return True


@pytest.mark.parametrize("int8_mode", [0, 1])
@pytest.mark.parametrize("persist", ["1", "0"])
@pytest.mark.parametrize("S", [37, 1500, 9000])
def test_mid_model_follows_its_plain_run(gh, monkeypatch, S, persist, int8_mode):
    """Random weights, H = 1024, short and long contexts; the plain steps between the verify passes run on the one-row persistent
    kernel where its plan takes the request (decode_path 1), on the rows kernel where it declines (3), and with FTCF_PERSIST=0
    on the per-stage launches (0).  Drafts: n-gram; the plain run's tokens with every third one corrupted; the same with
    holes (negative ids: no draft at that step), so that verify passes and plain steps alternate."""
    monkeypatch.setenv("FTCF_PERSIST", persist)
    cfg = MID
    V = cfg["vocab_size"]
    w = random_model(cfg, seed=5 + int8_mode, std=0.04)
    op = gh.make_op(cfg, w, int8_mode=int8_mode)
    rng = np.random.RandomState(S)
    blk = rng.randint(3, V, size=S // 2).tolist()
    prompt = (blk + blk + blk)[:S]
    out_len = 24
    p_ids, p_len, logits = _plain_with_logits(op, prompt, out_len, V)
    path = op.stats()["decode_path"]
    assert path == 0 if persist == "0" else path in (1, 3)
    gen = p_ids[S:]
    wrong = lambda t: 3 + (t - 3 + 1) % (V - 3)
    holes = [(-1 if (i // 3) % 2 == 0 else (wrong(t) if i % 5 == 4 else t)) for i, t in enumerate(gen)]
    for what, kw in (("n-gram", dict(speculative_tokens=4)), ("n-gram K 15", dict(speculative_tokens=15, speculative_ngram=2)),
                     ("every third wrong", dict(speculative_tokens=4, draft_ids=[wrong(t) if i % 3 == 2 else t for i, t in enumerate(gen)])),
                     ("holes", dict(speculative_tokens=8, draft_ids=holes))):
        s_ids, s_len, st = forward(op, prompt, out_len, **kw)
        same = _same_up_to_a_near_tie(s_ids, p_ids, logits, S, (what, S, int8_mode))
        print(f"[S {S} int8 {int8_mode} plain path {path} {what}: passes {st['spec_steps']} drafted {st['spec_drafted']} "
              f"accepted {st['spec_accepted']} same {same}] ", end="")
        assert st["spec_active"] == 1 and (st["spec_steps"] > 0 or "draft_ids" not in kw)
        if same:
            assert s_len == p_len
        if what == "holes" and same:
            assert 0 < st["spec_steps"] < out_len - 1 and st["spec_accepted"] > 0  # both kinds of step ran


def test_requests_the_feature_does_not_cover_run_as_before(gh, tiny):
    cfg, w, layers, glob, z = tiny
    V = cfg["vocab_size"]
    op = gh.make_op(cfg, w)
    ids1 = torch.from_numpy(z["prompt"][None, :].astype(np.int32)).cuda()
    ids2 = torch.from_numpy(np.stack([z["prompt"], z["prompt"][::-1]]).astype(np.int32)).cuda()
    l1 = torch.tensor([16], dtype=torch.int32, device="cuda")
    l2 = torch.tensor([16, 16], dtype=torch.int32, device="cuda")
    t = lambda v, dt=torch.int32: torch.tensor([v], dtype=dt)
    seen = []
    cases = {
        "batch 2": lambda o, **kw: o.forward(ids2, l2, 8, 1, t(1), return_cum_log_probs=0, **kw),
        "beam 2": lambda o, **kw: o.forward(ids1, l1, 8, 2, return_cum_log_probs=1, **kw),
        "top_k 50": lambda o, **kw: o.forward(ids1, l1, 8, 1, t(50), random_seed=t(7, torch.int64), **kw),
        "repetition penalty": lambda o, **kw: o.forward(ids1, l1, 8, 1, t(1), repetition_penalty=t(1.3, torch.float32), **kw),
        "callback": lambda o, **kw: o.forward(ids1, l1, 8, 1, t(1), callback=lambda d: seen.append(d["last_tokens"][0][0]), **kw),
        "short prompt in a longer row": lambda o, **kw: o.forward(ids1, torch.tensor([11], dtype=torch.int32, device="cuda"), 8, 1, t(1), **kw),
        "cum_log_probs": lambda o, **kw: o.forward(ids1, l1, 8, 1, t(1), return_cum_log_probs=1, **kw),
    }
    for name, run in cases.items():
        a = [x.cpu().numpy() for x in run(op)]
        n_seen = len(seen)
        b = [x.cpu().numpy() for x in run(op, speculative_tokens=4)]
        assert op.stats()["spec_active"] == 0 and op.stats()["spec_steps"] == 0, name
        assert len(a) == len(b) and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b)), name
        if name == "callback":
            assert seen[:n_seen] == seen[n_seen:] and n_seen > 0
    # an fp32 engine
    op32 = gh.make_op(cfg, w, dtype=torch.float32)
    a = [x.cpu().numpy() for x in op32.forward(ids1, l1, 8, 1, t(1))]
    b = [x.cpu().numpy() for x in op32.forward(ids1, l1, 8, 1, t(1), speculative_tokens=4)]
    assert op32.stats()["spec_active"] == 0 and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_tensor_parallel_ranks_run_as_before(gh, tiny):
    """TP 2 as a local group (two engines in this process): speculative_tokens is ignored, the outputs are bit-identical."""
    from fastertransformer4codefuse_amd.gptneox_op import LocalTensorParallelGroup
    cfg, w, layers, glob, z = tiny
    ids = torch.from_numpy(z["prompt"][None, :].astype(np.int32)).cuda()
    lens = torch.tensor([16], dtype=torch.int32, device="cuda")
    group = LocalTensorParallelGroup()
    res, err = [None, None], []

    def worker(r):
        try:
            op = gh.make_op(cfg, shard_weights(cfg, w, 2, r), tp=2, rank=r, comm=group)
            a = [x.cpu().numpy() for x in op.forward(ids, lens, 8, 1, torch.tensor([1], dtype=torch.int32))]
            b = [x.cpu().numpy() for x in op.forward(ids, lens, 8, 1, torch.tensor([1], dtype=torch.int32), speculative_tokens=4)]
            res[r] = (a, b, op.stats()["spec_active"])
        except BaseException as e:  # noqa: BLE001
            err.append((r, e))

    ths = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(2)]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=300)
    assert not err, err
    for r in range(2):
        a, b, active = res[r]
        assert active == 0 and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert res[0][0][0][0, 0, 16:].tolist() == z["hf_tokens"].tolist()


def test_out_of_range_arguments_are_refused_and_zero_is_off(gh, tiny):
    from fastertransformer4codefuse_amd import capi
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w)
    ids = torch.from_numpy(z["prompt"][None, :].astype(np.int32)).cuda()
    lens = torch.tensor([16], dtype=torch.int32, device="cuda")
    k1 = torch.tensor([1], dtype=torch.int32)
    for kw in (dict(speculative_tokens=16), dict(speculative_tokens=-1), dict(speculative_tokens=4, speculative_ngram=9),
               dict(speculative_tokens=4, speculative_ngram=-1), dict(draft_ids=torch.zeros(8, dtype=torch.int32, device="cuda")),
               dict(speculative_tokens=4, draft_ids=torch.zeros(7, dtype=torch.int32, device="cuda"))):
        with pytest.raises(RuntimeError):
            op.forward(ids, lens, 8, 1, k1, **kw)
    # the library itself refuses them too (a caller of the C ABI)
    out_ids = torch.zeros((1, 1, 24), dtype=torch.int32, device="cuda")
    seq = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    for K, N in ((16, 0), (-1, 0), (4, 9), (4, -2)):
        fa = capi.ForwardArgs()
        fa.input_ids, fa.input_lengths = ids.data_ptr(), lens.data_ptr()
        fa.batch_size, fa.max_input_len, fa.output_len, fa.beam_width = 1, 16, 8, 1
        fa.output_ids, fa.sequence_lengths = out_ids.data_ptr(), seq.data_ptr()
        fa.speculative_tokens, fa.speculative_ngram = K, N
        assert capi.lib().ftcf_gptneox_forward(op._h, C.byref(fa)) == -1  # FTCF_ERR_INVALID_ARG
    # omitted / 0: what the request returned before the fields existed, cum_log_probs included (the "defaults return what they
    # returned" test of tests/test_gpu_log_probs.py is the model)
    a = [x.cpu().numpy() for x in op.forward(ids, lens, 8, 1, k1, return_cum_log_probs=1)]
    b = [x.cpu().numpy() for x in op.forward(ids, lens, 8, 1, k1, return_cum_log_probs=1, speculative_tokens=0, speculative_ngram=0)]
    assert len(a) == len(b) == 3 and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    assert a[0][0, 0, 16:].tolist() == z["hf_tokens"].tolist()
    assert op.stats()["spec_active"] == 0


@pytest.mark.parametrize("int8_mode", [0, 1])
def test_no_state_leaks_between_speculative_and_plain_requests(gh, tiny, int8_mode):
    cfg, w, layers, glob, z = tiny
    op = gh.make_op(cfg, w, int8_mode=int8_mode)
    prompt, out_len = repeating_prompt(cfg["vocab_size"]), 24
    other = z["prompt"].tolist()
    plain_before = forward(op, other, 8)[:2]
    first = forward(op, prompt, out_len, speculative_tokens=4)
    plain_between = forward(op, other, 8)[:2]
    second = forward(op, prompt, out_len, speculative_tokens=4)
    plain_after = forward(op, other, 8)[:2]
    keys = ("spec_active", "spec_steps", "spec_drafted", "spec_accepted", "decode_steps")
    assert first[:2] == second[:2] and [first[2][k] for k in keys] == [second[2][k] for k in keys]
    assert plain_before == plain_between == plain_after
    assert plain_after[0][16:] == z["hf_tokens"].tolist()
