"""-m gpu: speculative decoding of top-k SAMPLED requests (GptNeoXOp.set_speculative_sampling(1)).  The
engine's random numbers are counter based, so a verify pass samples row i with the draw the plain step of that position would take
and the request returns the token sequence of the same request without speculative_tokens for the same seed -- not merely its
distribution.  Every check is therefore an equality with the unspeculated request (and the CPU oracle): tokens, sequence lengths
and callback invocations, for the requests of tests/speculative_sampled_cases.py, whose every step is stable against the logit
differences of two GEMM forms (tests/test_speculative_sampled_host.py); log-probabilities agree as two GEMM forms do and
cum_log_probs is the sequential fp32 sum of output_log_probs; the counters follow the host simulation of the accept rule."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import speculative_sampled_cases as sc
from tests.helpers import load_tiny, quantize_layers, random_model, weight_list_to_layers
from tests.test_gpu_engine import MID
from tests.test_gpu_speculative import simulate
from tests.test_gpu_speculative_scope import GEMM_FORM_TOL, _bits_equal, first_new, run, seq_sum

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

KEYS = ("spec_steps", "spec_drafted", "spec_accepted")


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


_OPS, _ORACLE = {}, {}


def sampling_op(gh, tiny, int8_mode):
    """one engine per weight form, speculative sampling on, scope 0"""
    if int8_mode not in _OPS:
        _OPS[int8_mode] = gh.make_op(tiny[0], tiny[1], int8_mode=int8_mode)
    op = _OPS[int8_mode]
    op.set_speculative_sampling(1)
    op.set_speculative_scope(0)
    return op


def oracle_tokens(tiny, case):
    if case not in _ORACLE:
        from oracle import oracle as orc
        cfg, w, layers, glob, z = tiny
        lay = quantize_layers(layers) if case[1] else layers
        model = orc.Model(dict(cfg, fp16=1, int8_mode=case[1]), lay, glob)
        _ORACLE[case] = sc.replay(model, sc.prompt_of(case[0], cfg, z), case)[0]
    return _ORACLE[case]


def sampled(case):
    """the sampling arguments of a case, as GptNeoXOp.forward takes them"""
    _, _, k, T, top_p, seed = case
    kw = dict(top_k=k, random_seed=torch.tensor([seed], dtype=torch.int64))
    if T != 1.0:
        kw["temperature"] = torch.tensor([T], dtype=torch.float32)
    if top_p != 0.0:
        kw["top_p"] = torch.tensor([top_p], dtype=torch.float32)
    return kw


def draft_forms(V):
    wrong = lambda t: 3 + (t - 3 + 1) % (V - 3)
    return {
        "n-gram": None,
        "intact": lambda gen: list(gen),
        "every third wrong": lambda gen: [wrong(t) if i % 3 == 2 else t for i, t in enumerate(gen)],
        "all wrong": lambda gen: [wrong(t) for t in gen],
        "holes": lambda gen: [-1 if i % 4 == 1 else t for i, t in enumerate(gen)],  # passes and plain steps alternate
    }


def check_counters(stats, prompt, gen, K, out_len, drafts, what):
    want = simulate(prompt, gen, K, 3, out_len, drafts)[:3]
    assert tuple(stats[k] for k in KEYS) == want, (what, [stats[k] for k in KEYS], want)


@pytest.mark.parametrize("K", [1, 4, 15])
@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_a_sampled_request_speculates_and_returns_its_plain_run_token_for_token(gh, tiny, case, K):
    cfg, z = tiny[0], tiny[4]
    V, end = cfg["vocab_size"], cfg["end_id"]
    op = sampling_op(gh, tiny, case[1])
    prompt, out_len = sc.prompt_of(case[0], cfg, z), sc.OUT_LEN
    S = len(prompt)
    samp = sampled(case)
    # the unspeculated request, bare: the oracle's tokens, with picks that are not the arg max (the host test says which)
    plain = run(op, prompt, out_len, **samp)
    gen = plain["ids"][S:plain["len"]]
    assert plain["stats"]["spec_active"] == 0
    assert gen == oracle_tokens(tiny, case) and plain["len"] == S + len(gen), case
    # ... and as the harness sends it: log-probabilities, a callback, a stop word of its own tokens behind one that never completes
    req = dict(cum=1, olp=True, cb=True, stop=[[end, end], [gen[first_new(gen, 6)]]])
    plain_full = run(op, prompt, out_len, **req, **samp)
    gen_full = plain_full["ids"][S:plain_full["len"]]
    assert plain_full["stats"]["spec_active"] == 0 and gen_full == gen[:len(gen_full)] and 0 < len(gen_full) <= len(gen)
    assert seq_sum(plain_full["olp"]).tobytes() == np.float32(plain_full["cum"]).tobytes()
    accepted = 0
    for name, make in draft_forms(V).items():
        drafts = None if make is None else make(plain["ids"][S:])
        kw = dict(speculative_tokens=K, **({} if drafts is None else dict(draft_ids=drafts)))
        what = (case, K, name)
        # bare, scope 0
        op.set_speculative_scope(0)
        got = run(op, prompt, out_len, **samp, **kw)
        st = got["stats"]
        assert st["spec_active"] == 1, what
        assert (got["ids"], got["len"]) == (plain["ids"], plain["len"]), what
        assert st["decode_steps"] == plain["stats"]["decode_steps"], what
        check_counters(st, prompt, gen, K, out_len, drafts, what)
        accepted += st["spec_accepted"]
        # scope 1, everything together
        op.set_speculative_scope(1)
        full = run(op, prompt, out_len, **req, **samp, **kw)
        st = full["stats"]
        print(f"[{name}: passes {st['spec_steps']} drafted {st['spec_drafted']} accepted {st['spec_accepted']}] ", end="")
        assert st["spec_active"] == 1, what
        assert (full["ids"], full["len"]) == (plain_full["ids"], plain_full["len"]), what
        assert full["seen"] == plain_full["seen"] and len(full["seen"]) > 0, what
        check_counters(st, prompt, gen_full, K, out_len, drafts, what)
        np.testing.assert_allclose(full["olp"], plain_full["olp"], err_msg=str(what), **GEMM_FORM_TOL)
        np.testing.assert_allclose(full["cum"], plain_full["cum"], err_msg=str(what), **GEMM_FORM_TOL)
        assert seq_sum(full["olp"]).tobytes() == np.float32(full["cum"]).tobytes(), what
    op.set_speculative_scope(0)
    assert accepted > 0, "the intact drafts at least are accepted"


@pytest.mark.parametrize("int8_mode", [0, 1])
def test_begin_step_finish_never_overshoots_max_steps(gh, tiny, int8_mode):
    from fastertransformer4codefuse_amd import capi
    cfg, z = tiny[0], tiny[4]
    case = next(c for c in sc.CASES if c[:5] == ("golden", int8_mode, 50, 1.0, 0.0))
    op = sampling_op(gh, tiny, int8_mode)
    prompt, out_len = z["prompt"].tolist(), sc.OUT_LEN
    plain = run(op, prompt, out_len, **sampled(case))
    gen = plain["ids"][len(prompt):]
    ids = torch.tensor([prompt], dtype=torch.int32, device="cuda")
    lens = torch.tensor([len(prompt)], dtype=torch.int32, device="cuda")
    drafts = torch.tensor(gen, dtype=torch.int32, device="cuda")
    out_ids = torch.zeros((1, 1, len(prompt) + out_len), dtype=torch.int32, device="cuda")
    seq = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    top_k, seed = np.array([case[2]], np.int32), np.array([case[5]], np.uint64)
    fa = capi.ForwardArgs()
    fa.input_ids, fa.input_lengths = ids.data_ptr(), lens.data_ptr()
    fa.batch_size, fa.max_input_len, fa.output_len, fa.beam_width = 1, len(prompt), out_len, 1
    fa.top_k, fa.n_top_k, fa.random_seed, fa.n_random_seed = top_k.ctypes.data, 1, seed.ctypes.data, 1
    fa.output_ids, fa.sequence_lengths = out_ids.data_ptr(), seq.data_ptr()
    fa.speculative_tokens, fa.draft_ids = 4, drafts.data_ptr()
    L = capi.lib()
    done = C.c_int(0)
    capi.check(L.ftcf_gptneox_begin(op._h, C.byref(fa)))
    total, limits = 0, itertools.chain([3, 1, 2, 4], itertools.repeat(100))
    while total < out_len:
        limit = next(limits)
        capi.check(L.ftcf_gptneox_step(op._h, limit, C.byref(done)))
        assert 1 <= done.value <= limit and total + done.value <= out_len
        total += done.value
    assert total == out_len
    capi.check(L.ftcf_gptneox_finish(op._h))
    torch.cuda.synchronize()
    st = op.stats()
    assert st["spec_active"] == 1 and st["spec_accepted"] > 0 and st["decode_steps"] == out_len
    assert out_ids[0, 0].cpu().numpy().tolist() == plain["ids"] and int(seq[0, 0].item()) == plain["len"]


def test_the_switch_off_is_as_before_and_a_bad_value_is_refused(gh, tiny):
    from fastertransformer4codefuse_amd.capi import FtcfError
    cfg, z = tiny[0], tiny[4]
    op = gh.make_op(cfg, tiny[1])
    for case in [c for c in sc.CASES if c[1] == 0 and c[2] == 50]:
        prompt = sc.prompt_of(case[0], cfg, z)
        for scope, req in ((0, {}), (1, dict(cum=1, olp=True, cb=True))):
            op.set_speculative_scope(scope)
            plain = run(op, prompt, sc.OUT_LEN, **req, **sampled(case))
            # the default is off: the request does not speculate and is bit-identical to plain
            off = run(op, prompt, sc.OUT_LEN, speculative_tokens=4, **req, **sampled(case))
            assert off["stats"]["spec_active"] == 0 and off["stats"]["spec_steps"] == 0, (case, scope)
            assert _bits_equal(off["raw"], plain["raw"]) and off["seen"] == plain["seen"], (case, scope)
            op.set_speculative_sampling(1)
            on = run(op, prompt, sc.OUT_LEN, speculative_tokens=4, **req, **sampled(case))
            assert on["stats"]["spec_active"] == 1 and (on["ids"], on["len"], on["seen"]) == (plain["ids"], plain["len"], plain["seen"])
            # a greedy request is not the switch's business: it speculates as it did, with the same bits
            greedy = [run(op, prompt, sc.OUT_LEN, speculative_tokens=4, **req) for _ in range(1)]
            for bad in (2, -1):
                with pytest.raises(FtcfError) as e:
                    op.set_speculative_sampling(bad)
                assert e.value.code == -1
            assert run(op, prompt, sc.OUT_LEN, speculative_tokens=4, **req, **sampled(case))["stats"]["spec_active"] == 1  # (still on)
            op.set_speculative_sampling(0)
            again = run(op, prompt, sc.OUT_LEN, speculative_tokens=4, **req, **sampled(case))
            assert again["stats"]["spec_active"] == 0 and _bits_equal(again["raw"], plain["raw"]), (case, scope)
            greedy.append(run(op, prompt, sc.OUT_LEN, speculative_tokens=4, **req))
            assert greedy[0]["stats"]["spec_active"] == greedy[1]["stats"]["spec_active"] == 1
            assert _bits_equal(greedy[0]["raw"], greedy[1]["raw"])


def test_requests_the_switch_still_excludes_run_as_before(gh, tiny):
    cfg, z = tiny[0], tiny[4]
    op = sampling_op(gh, tiny, 0)
    op.set_speculative_scope(1)
    ids1 = torch.from_numpy(z["prompt"][None, :].astype(np.int32)).cuda()
    ids2 = torch.from_numpy(np.stack([z["prompt"], z["prompt"][::-1]]).astype(np.int32)).cuda()
    l1 = torch.tensor([16], dtype=torch.int32, device="cuda")
    l2 = torch.tensor([16, 16], dtype=torch.int32, device="cuda")
    t = lambda v, dt=torch.int32: torch.tensor([v], dtype=dt)
    seed = t(7, torch.int64)
    cases = {
        "pure top-p": lambda **kw: op.forward(ids1, l1, 8, 1, t(0), t(0.8, torch.float32), random_seed=seed, **kw),
        "top_k 65": lambda **kw: op.forward(ids1, l1, 8, 1, t(65), random_seed=seed, **kw),
        "repetition penalty": lambda **kw: op.forward(ids1, l1, 8, 1, t(50), repetition_penalty=t(1.3, torch.float32), random_seed=seed, **kw),
        "batch 2": lambda **kw: op.forward(ids2, l2, 8, 1, t(50), random_seed=seed, return_cum_log_probs=1, **kw),
    }
    for name, call in cases.items():
        a = [x.cpu().numpy() for x in call()]
        b = [x.cpu().numpy() for x in call(speculative_tokens=4)]
        assert op.stats()["spec_active"] == 0 and op.stats()["spec_steps"] == 0, name
        assert _bits_equal(a, b), name
    op.set_speculative_scope(0)


@pytest.mark.parametrize("int8_mode", [0, 1])
def test_mid_model_completes_and_counts_as_the_simulation_of_its_own_tokens(gh, int8_mode):
    """Random weights, H = 1024, a 1500-token prompt, top_k 4: the run completes and its counters are the accept rule's on the tokens
    it emitted.  No token comparison with the plain run: this model's logits reach |40|, and the near-tie allowance the project
    grants it (1e-2 of the largest logit) would excuse almost every sampled step."""
    cfg, S = MID, 1500
    V = cfg["vocab_size"]
    op = gh.make_op(cfg, random_model(cfg, seed=5 + int8_mode, std=0.04), int8_mode=int8_mode)
    op.set_speculative_sampling(1)
    op.set_speculative_scope(1)
    blk = np.random.RandomState(S).randint(3, V, size=S // 2).tolist()
    prompt, out_len = (blk + blk + blk)[:S], 24
    got = run(op, prompt, out_len, cum=1, olp=True, cb=True, top_k=4, random_seed=torch.tensor([3], dtype=torch.int64), speculative_tokens=4)
    st = got["stats"]
    gen = got["ids"][S:got["len"]]
    print(f"[int8 {int8_mode}: {len(gen)} tokens, passes {st['spec_steps']} drafted {st['spec_drafted']} accepted {st['spec_accepted']}] ", end="")
    assert st["spec_active"] == 1 and 0 < len(gen) <= out_len
    check_counters(st, prompt, gen, 4, out_len, None, ("mid", int8_mode))
    assert st["spec_steps"] > 0
    assert seq_sum(got["olp"]).tobytes() == np.float32(got["cum"]).tobytes() and np.isfinite(got["olp"]).all()
