"""-m gpu: speculative greedy decoding under the wider scope (GptNeoXOp.set_speculative_scope(1)): a greedy
request with return_cum_log_probs, output_log_probs, a callback, stop words or optional_last_tokens -- alone, and all together as
harness.generate() sends them -- speculates and returns the tokens, the sequence lengths and the callback invocations of the same
request without speculative_tokens; its log-probabilities agree with that run's as two GEMM forms do (a pass runs the burst
GEMMs, the plain step the persistent kernel: the tolerance of tests/test_gpu_log_probs.py) and cum_log_probs is the sequential
fp32 sum of output_log_probs.  What the scope still excludes, and everything at scope 0, runs exactly as before."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import load_tiny, random_model
from tests.test_gpu_engine import MID
from tests.test_gpu_speculative import _plain_with_logits, _same_up_to_a_near_tie, draft_ref, repeating_prompt

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

GEMM_FORM_TOL = dict(atol=5e-3, rtol=1e-2)  # tests/test_gpu_log_probs.py: runs that take different GEMM forms
# optional_last_tokens, by prompt: for the golden prompt three tokens the model would not choose (every token of the request changes;
# the drafts are that request's own plain tokens), for the repeating prompt a list that holds the model's own choice, 33 (the
# tokens stay the ones the n-gram lookup finds; the request's plain steps still all take the general decode form)
LAST_TOKENS = {"caller drafts": [[7, 11, 13, -1]], "n-gram": [[33, 7, 11, -1]]}


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


@pytest.fixture(scope="module")
def tiny():
    return load_tiny()


_OPS = {}


def scoped_op(gh, tiny, int8_mode):
    """one engine per weight form, at scope 1"""
    if int8_mode not in _OPS:
        cfg, w, z = tiny
        _OPS[int8_mode] = gh.make_op(cfg, w, int8_mode=int8_mode)
    _OPS[int8_mode].set_speculative_scope(1)
    return _OPS[int8_mode]


def stop_list(words):
    """the reference's word list for one row: [1, 2, n] (ids back to back, then cumulative end offsets, -1 padded)"""
    ids = [t for w in words for t in w]
    out = np.full((1, 2, len(ids) + 1), -1, np.int32)
    out[0, 0, :] = 0
    out[0, 0, :len(ids)] = ids
    out[0, 1, :len(words)] = np.cumsum([len(w) for w in words])
    return out


def seq_sum(values):
    acc = np.float32(0.0)
    for v in np.asarray(values, np.float32):
        acc = np.float32(acc + v)
    return acc


def run(op, prompt, out_len, cum=0, olp=False, cb=False, stop=None, last=None, top_k=1, draft_ids=None, **kw):
    ids = torch.tensor([list(prompt)], dtype=torch.int32, device="cuda")
    lens = torch.tensor([len(prompt)], dtype=torch.int32, device="cuda")
    seen = []
    if draft_ids is not None:
        d = list(draft_ids) + [-1] * (out_len - len(draft_ids))
        draft_ids = torch.tensor(d[:out_len], dtype=torch.int32, device="cuda")
    o = op.forward(ids, lens, out_len, 1, torch.tensor([top_k], dtype=torch.int32),
                   stop_words_list=None if stop is None else torch.from_numpy(stop_list(stop)).cuda(),
                   optional_last_tokens=None if last is None else torch.tensor(last, dtype=torch.int32, device="cuda"),
                   return_cum_log_probs=cum, callback=(lambda d: seen.append((d["last_tokens"], d["idxs"]))) if cb else None,
                   return_output_log_probs=olp, draft_ids=draft_ids, **kw)
    torch.cuda.synchronize()
    o = [x.cpu().numpy() for x in o]
    res = dict(raw=o, ids=o[0][0, 0].tolist(), len=int(o[1][0, 0]), seen=seen, stats=op.stats())
    rest = o[2:]
    if cum:
        res["cum"] = rest.pop(0)[0, 0]
    if olp:
        res["olp"] = rest.pop(0)[0, 0]
    return res


def first_new(gen, lo):
    """the first generated index >= lo whose token has not been generated before (a run that repeats itself from there on: the
    last such index below lo)"""
    new = [j for j in range(1, len(gen)) if gen[j] not in gen[:j]]
    return next((j for j in new if j >= lo), new[-1])


def passes(prompt, gen, K, N, out_len, draft_ids=None):
    """[(first generated index, tokens emitted)] of the verify passes of a request whose plain tokens are `gen`: the loop of
    tests/test_gpu_speculative.py simulate()"""
    hist, j, out = list(prompt), 0, []
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
        e = 1
        if nd > 0:
            e = 0
            while True:
                tok = gen[j + e]
                e += 1
                hit = e - 1 < nd and d[e - 1] == tok
                if not hit or j + e >= len(gen) or e > nd:
                    break
            out.append((j, e))
        hist += gen[j:j + e]
        j += e
    return out


def word_landing_at(prompt, gen, positions, lengths):
    """a stop word (the tokens that end at generated index x, of one of `lengths`) whose FIRST completion in the generated tokens is
    at x, for the first x of `positions` that has one -> (word, x)"""
    seq, S = list(prompt) + list(gen), len(prompt)
    for x in positions:
        for n in lengths:
            word = seq[S + x - n + 1:S + x + 1]
            first = next(y for y in range(len(gen)) if S + y + 1 >= n and seq[S + y - n + 1:S + y + 1] == word)
            if len(word) == n and first == x:
                return word, x
    raise AssertionError("no stop word lands where the test wants it: choose another prompt")


def stop_words_for(prompt, gen, runs):
    """A stop word that lands INSIDE an accepted run (at an accepted draft that is not the pass's last token) and one that lands at a
    run's LAST token, taken from the plain run's tokens; one and two tokens long where such a word exists (a token the lookup
    drafts has been seen before: a word that first completes there may need more tokens)."""
    inside = [x for j, e in runs if e >= 2 for x in range(j, j + e - 1)]
    last = [j + e - 1 for j, e in runs if e >= 2]
    return word_landing_at(prompt, gen, inside, (1, 2, 3, 4))[0], word_landing_at(prompt, gen, last, (2, 1, 3, 4))[0]


def variants(last):
    """the requests the scope adds, each alone (the stop words: stop_words_for), then all together as the harness sends them"""
    return {
        "cum_log_probs": dict(cum=1),
        "output_log_probs": dict(olp=True),
        "callback": dict(cb=True),
        "optional_last_tokens": dict(last=last),
        "all together": dict(cum=1, olp=True, cb=True, last=last),  # (+ a stop word of ITS plain run: see the test)
    }


def check(op, prompt, out_len, req, drafts, what):
    """the request `req` plain, then with speculative_tokens = 4 and each of `drafts` (name -> function of the plain tokens, None =
    the n-gram lookup): spec_active, accepted drafts, the plain run's tokens, lengths, callbacks and log-probabilities"""
    plain = run(op, prompt, out_len, **req)
    assert plain["stats"]["spec_active"] == 0
    gen = plain["ids"][len(prompt):plain["len"]]
    for name, make in drafts.items():
        kw = dict(speculative_tokens=4)
        if make is not None:
            kw["draft_ids"] = make(plain["ids"][len(prompt):])
        got = run(op, prompt, out_len, **req, **kw)
        st = got["stats"]
        print(f"[{what} / {name}: {len(gen)} tokens, passes {st['spec_steps']} drafted {st['spec_drafted']} accepted {st['spec_accepted']}] ", end="")
        assert st["spec_active"] == 1 and st["spec_accepted"] > 0, (what, name, st)
        assert st["decode_steps"] == plain["stats"]["decode_steps"], (what, name)
        assert (got["ids"], got["len"]) == (plain["ids"], plain["len"]), (what, name)
        assert got["seen"] == plain["seen"], (what, name)
        if req.get("cb"):
            assert len(got["seen"]) > 0
        for k in ("cum", "olp"):
            if k in plain:
                np.testing.assert_allclose(got[k], plain[k], err_msg=f"{what} / {name} / {k}", **GEMM_FORM_TOL)
        if "cum" in got and "olp" in got:
            assert seq_sum(got["olp"]).tobytes() == np.float32(got["cum"]).tobytes(), (what, name)
            assert seq_sum(plain["olp"]).tobytes() == np.float32(plain["cum"]).tobytes()
    return plain


def wrong_every_second(V):
    wrong = lambda t: 3 + (t - 3 + 1) % (V - 3)
    return lambda gen: [wrong(t) if i % 2 == 1 else t for i, t in enumerate(gen)]


@pytest.mark.parametrize("int8_mode", [0, 1])
@pytest.mark.parametrize("which", ["cum_log_probs", "output_log_probs", "callback", "stop word inside a run", "stop word at a run's last token",
                                   "optional_last_tokens", "all together"])
def test_tiny_requests_of_the_wider_scope_speculate_and_follow_their_plain_run(gh, tiny, which, int8_mode):
    cfg, w, z = tiny
    V = cfg["vocab_size"]
    op = scoped_op(gh, tiny, int8_mode)
    for pname, prompt, out_len, drafts in (
            ("caller drafts", z["prompt"].tolist(), 23, {"intact": lambda gen: gen, "every 2nd wrong": wrong_every_second(V)}),
            ("n-gram", repeating_prompt(V), 24, {"n-gram": None})):
        for dname, make in drafts.items():
            what = f"int8 {int8_mode} {pname} {which}"
            if "stop word" in which:
                # from the bare request's tokens and the passes these drafts give it
                bare = run(op, prompt, out_len)
                gen = bare["ids"][len(prompt):bare["len"]]
                runs = passes(prompt, gen, 4, 3, out_len, None if make is None else make(gen))
                inside, at_last = stop_words_for(prompt, gen, runs)
                req = dict(stop=[[cfg["end_id"], cfg["end_id"]], inside if "inside" in which else at_last])
                plain = check(op, prompt, out_len, req, {dname: make}, what)
                assert plain["len"] < len(prompt) + len(gen), "the stop word ended the request early"
                continue
            req = variants(LAST_TOKENS[pname])[which]
            if which == "all together":
                # the stop word comes from the tokens THIS request produces (optional_last_tokens may change them from the first
                # on); in front of it a word that never completes (the end token twice)
                g = run(op, prompt, out_len, **req)
                g = g["ids"][len(prompt):g["len"]]
                req = dict(req, stop=[[cfg["end_id"], cfg["end_id"]], [g[first_new(g, 6)]]])
            check(op, prompt, out_len, req, {dname: make}, what)


@pytest.mark.parametrize("int8_mode", [0, 1])
@pytest.mark.parametrize("S", [37, 1500])
def test_mid_model_follows_its_plain_run_within_the_near_tie_rule(gh, S, int8_mode):
    """Random weights, H = 1024: all of the scope's outputs together; a first token difference only at a near tie of the plain run's
    logits (tests/test_gpu_speculative.py), everything else compared while the tokens agree."""
    cfg = MID
    V = cfg["vocab_size"]
    op = gh.make_op(cfg, random_model(cfg, seed=5 + int8_mode, std=0.04), int8_mode=int8_mode)
    op.set_speculative_scope(1)
    rng = np.random.RandomState(S)
    blk = rng.randint(3, V, size=S // 2).tolist()
    prompt, out_len = (blk + blk + blk)[:S], 24
    p_ids, p_len, logits = _plain_with_logits(op, prompt, out_len, V)
    gen = p_ids[S:p_len]
    req = dict(cum=1, olp=True, cb=True, stop=[[gen[first_new(gen, 14)]], [cfg["end_id"], cfg["end_id"]]])
    plain = run(op, prompt, out_len, **req)
    assert plain["stats"]["spec_active"] == 0 and plain["ids"][:plain["len"]] == p_ids[:plain["len"]]
    wrong = lambda t: 3 + (t - 3 + 1) % (V - 3)
    for what, kw in (("n-gram", {}), ("intact", dict(draft_ids=p_ids[S:])),
                     ("every third wrong", dict(draft_ids=[wrong(t) if i % 3 == 2 else t for i, t in enumerate(p_ids[S:])]))):
        got = run(op, prompt, out_len, speculative_tokens=4, **req, **kw)
        st = got["stats"]
        same = _same_up_to_a_near_tie(got["ids"], plain["ids"], logits, S, (what, S, int8_mode))
        print(f"[S {S} int8 {int8_mode} {what}: passes {st['spec_steps']} accepted {st['spec_accepted']} same {same}] ", end="")
        assert st["spec_active"] == 1 and (st["spec_steps"] > 0 or what == "n-gram")
        assert seq_sum(got["olp"]).tobytes() == np.float32(got["cum"]).tobytes()
        if same:
            assert got["len"] == plain["len"] and got["seen"] == plain["seen"]
            np.testing.assert_allclose(got["olp"], plain["olp"], **GEMM_FORM_TOL)
            np.testing.assert_allclose(got["cum"], plain["cum"], **GEMM_FORM_TOL)


@pytest.mark.parametrize("int8_mode", [0, 1])
def test_begin_step_finish_with_a_callback_never_emits_more_than_max_steps(gh, tiny, int8_mode):
    from fastertransformer4codefuse_amd import capi
    cfg, w, z = tiny
    op = scoped_op(gh, tiny, int8_mode)
    prompt, out_len = z["prompt"].tolist(), 20
    plain = run(op, prompt, out_len, cum=1, cb=True)
    gen = plain["ids"][len(prompt):]
    ids = torch.tensor([prompt], dtype=torch.int32, device="cuda")
    lens = torch.tensor([len(prompt)], dtype=torch.int32, device="cuda")
    drafts = torch.tensor(gen, dtype=torch.int32, device="cuda")
    out_ids = torch.zeros((1, 1, len(prompt) + out_len), dtype=torch.int32, device="cuda")
    seq = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    cum = torch.zeros((1, 1), dtype=torch.float32, device="cuda")
    top_k = np.array([1], np.int32)
    seen = []
    cb = capi.TOKEN_CALLBACK(lambda tokens, idxs, batch, beam, user: seen.append(([[int(tokens[0])]], [[int(idxs[0])]])))
    fa = capi.ForwardArgs()
    fa.input_ids, fa.input_lengths = ids.data_ptr(), lens.data_ptr()
    fa.batch_size, fa.max_input_len, fa.output_len, fa.beam_width = 1, len(prompt), out_len, 1
    fa.top_k, fa.n_top_k = top_k.ctypes.data, 1
    fa.output_ids, fa.sequence_lengths, fa.cum_log_probs = out_ids.data_ptr(), seq.data_ptr(), cum.data_ptr()
    fa.return_cum_log_probs, fa.callback = 1, cb
    fa.speculative_tokens, fa.draft_ids = 4, drafts.data_ptr()
    L = capi.lib()
    done = C.c_int(0)
    capi.check(L.ftcf_gptneox_begin(op._h, C.byref(fa)))
    total = 0
    while total < out_len:
        before = len(seen)
        capi.check(L.ftcf_gptneox_step(op._h, 3, C.byref(done)))
        assert 1 <= done.value <= 3 and len(seen) - before <= done.value
        total += done.value
    assert total == out_len
    capi.check(L.ftcf_gptneox_finish(op._h))
    torch.cuda.synchronize()
    st = op.stats()
    assert st["spec_active"] == 1 and st["spec_accepted"] > 0 and st["decode_steps"] == out_len
    assert out_ids[0, 0].cpu().numpy().tolist() == plain["ids"] and int(seq[0, 0].item()) == plain["len"]
    assert seen == plain["seen"] and len(seen) == out_len - 1  # (the request's last position is not reported)
    np.testing.assert_allclose(cum.cpu().numpy()[0, 0], plain["cum"], **GEMM_FORM_TOL)


def _bits_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_requests_the_wider_scope_still_excludes_run_as_before(gh, tiny):
    cfg, w, z = tiny
    op = scoped_op(gh, tiny, 0)
    ids1 = torch.from_numpy(z["prompt"][None, :].astype(np.int32)).cuda()
    ids2 = torch.from_numpy(np.stack([z["prompt"], z["prompt"][::-1]]).astype(np.int32)).cuda()
    l1 = torch.tensor([16], dtype=torch.int32, device="cuda")
    l2 = torch.tensor([16, 16], dtype=torch.int32, device="cuda")
    t = lambda v, dt=torch.int32: torch.tensor([v], dtype=dt)
    cases = {
        "top_k 50": lambda **kw: op.forward(ids1, l1, 8, 1, t(50), random_seed=t(7, torch.int64), **kw),
        "repetition penalty": lambda **kw: op.forward(ids1, l1, 8, 1, t(1), repetition_penalty=t(1.3, torch.float32), **kw),
        "batch 2": lambda **kw: op.forward(ids2, l2, 8, 1, t(1), return_cum_log_probs=1, **kw),
        "beams": lambda **kw: op.forward(ids1, l1, 8, 2, return_cum_log_probs=1, **kw),
        "top_logprobs": lambda **kw: op.forward(ids1, l1, 8, 1, t(1), top_logprobs=3, **kw),
        "temperature 0.7 with cum_log_probs": lambda **kw: op.forward(ids1, l1, 8, 1, t(1), temperature=t(0.7, torch.float32),
                                                                      return_cum_log_probs=1, **kw),
    }
    for name, call in cases.items():
        a = [x.cpu().numpy() for x in call()]
        b = [x.cpu().numpy() for x in call(speculative_tokens=4)]
        assert op.stats()["spec_active"] == 0 and op.stats()["spec_steps"] == 0, name
        assert _bits_equal(a, b), name


def test_scope_0_is_as_before_and_nothing_leaks_between_scopes(gh, tiny):
    from fastertransformer4codefuse_amd.capi import FtcfError
    cfg, w, z = tiny
    op = gh.make_op(cfg, w)
    prompt, other = repeating_prompt(cfg["vocab_size"]), z["prompt"].tolist()
    keys = ("spec_active", "spec_steps", "spec_drafted", "spec_accepted", "decode_steps")
    plain = {name: run(op, prompt, 24, **req) for name, req in (("callback", dict(cb=True)), ("cum", dict(cum=1)))}
    bare_before = run(op, other, 8)
    # the default scope is 0: the two requests do not speculate
    for name, req in (("callback", dict(cb=True)), ("cum", dict(cum=1))):
        got = run(op, prompt, 24, speculative_tokens=4, **req)
        assert got["stats"]["spec_active"] == 0 and _bits_equal(got["raw"], plain[name]["raw"]) and got["seen"] == plain[name]["seen"]
    # a value that is no scope is refused and changes nothing
    for bad in (2, -1):
        with pytest.raises(FtcfError) as e:
            op.set_speculative_scope(bad)
        assert e.value.code == -1
    assert run(op, prompt, 24, speculative_tokens=4, cum=1)["stats"]["spec_active"] == 0
    op.set_speculative_scope(1)
    first = {name: run(op, prompt, 24, speculative_tokens=4, **req) for name, req in (("callback", dict(cb=True)), ("cum", dict(cum=1)))}
    assert all(r["stats"]["spec_active"] == 1 and r["stats"]["spec_accepted"] > 0 for r in first.values())
    bare_between = run(op, other, 8)
    # back to 0: again unspeculated and bit-identical to plain
    op.set_speculative_scope(0)
    for name, req in (("callback", dict(cb=True)), ("cum", dict(cum=1))):
        got = run(op, prompt, 24, speculative_tokens=4, **req)
        assert got["stats"]["spec_active"] == 0 and _bits_equal(got["raw"], plain[name]["raw"]) and got["seen"] == plain[name]["seen"]
    # a bare request speculates at either scope, with the same tokens and counters
    bare0 = run(op, prompt, 24, speculative_tokens=4)
    op.set_speculative_scope(1)
    bare1 = run(op, prompt, 24, speculative_tokens=4)
    assert bare0["stats"]["spec_active"] == bare1["stats"]["spec_active"] == 1
    assert (bare0["ids"], bare0["len"]) == (bare1["ids"], bare1["len"]) and [bare0["stats"][k] for k in keys] == [bare1["stats"][k] for k in keys]
    second = {name: run(op, prompt, 24, speculative_tokens=4, **req) for name, req in (("callback", dict(cb=True)), ("cum", dict(cum=1)))}
    for name in first:
        assert _bits_equal(first[name]["raw"], second[name]["raw"]) and first[name]["seen"] == second[name]["seen"]
        assert [first[name]["stats"][k] for k in keys] == [second[name]["stats"][k] for k in keys]
    bare_after = run(op, other, 8)
    assert _bits_equal(bare_before["raw"], bare_between["raw"]) and _bits_equal(bare_before["raw"], bare_after["raw"])
    assert bare_after["ids"][16:] == z["hf_tokens"].tolist()
