"""-m gpu: per-token log-probabilities of beam hypotheses.  The step's record (k_beam_batch through ftcf_beam_search_step) to the
bit, the engine's getter (ftcf_gptneox_beam_log_probs / GptNeoXOp.beam_log_probs) against the replay of the GPU's own logits
through the oracle's beam layer and the numpy walk (tests/beam_log_probs_reference.py), the telescoping sum against
cum_log_probs, and the getter's edges."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library: see tests/test_gpu_engine.py)

from oracle import oracle as orc
from tests.beam_log_probs_reference import gather_tree_with_payload, step_differences
from tests.helpers import GOLDEN, load_tiny, random_model
from tests.test_gpu_beam import MID, _pick_end_id, _replay

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


@pytest.fixture(scope="module")
def tiny():
    cfg, w, _ = load_tiny()
    return cfg, w, np.load(os.path.join(GOLDEN, "tiny_gptneox_beam.npz"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the step, to the bit
# ---------------------------------------------------------------------------------------------------------------------
PATTERN = np.float32(777.25)
STEP_CASES = [
    (1, 2, 2, dict()),
    (2, 3, 97, dict(temperature=[0.7, 1.3], repetition_penalty=[1.3, 1.0])),
    (1, 64, 100, dict(beam_search_diversity_rate=[-0.2], len_penalty=[0.5])),
]


def run_steps(B, K, V, kw, record, n_steps=4, S=3):
    """n_steps consecutive ftcf_beam_search_step calls from cum = [0, -1e20, ...]; from the second on, beam 0 of every batch entry
    (the best one: its end token at cum + 0 beats its own continuations) is forced to be finished.  Returns the state around
    every step and at the end."""
    from fastertransformer4codefuse_amd import capi
    BK, total, end_id = B * K, S + n_steps + 1, min(2, V - 1)
    rng = np.random.RandomState(1000 * B + 10 * K + V)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ids0 = np.zeros((total, BK), np.int32)
    ids0[:S] = rng.randint(0, V, size=(S, BK))
    ids, par = d(ids0), d(np.zeros((total, BK), np.int32))
    fin, seq = d(np.zeros(BK, np.uint8)), d(np.full(BK, S - 1, np.int32))
    cum = d(np.where(np.arange(BK) % K == 0, 0.0, -1e20).astype(np.float32))
    indir = d(np.zeros((2, BK, total), np.int32))
    in_len = d(np.full(BK, S, np.int32))
    lp = d(np.full((total, BK), PATTERN, np.float32)) if record else None
    host = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in kw.items()}
    a = capi.BeamSearchArgs()
    a.output_ids, a.parent_ids, a.cache_indir = ids.data_ptr(), par.data_ptr(), indir.data_ptr()
    a.finished, a.seq_len, a.cum_log_probs, a.input_lengths = fin.data_ptr(), seq.data_ptr(), cum.data_ptr(), in_len.data_ptr()
    for name, v in host.items():
        setattr(a, name, v.ctypes.data)
        setattr(a, "n_" + name, v.size)
    a.B, a.K, a.V, a.max_input_len, a.total_len, a.s_max, a.end_id = B, K, V, S, total, total, end_id
    a.step_log_probs = lp.data_ptr() if record else None
    trace = []
    for t in range(n_steps):
        if t >= 1:
            fin[::K] = 1
        torch.cuda.synchronize()
        before, fin_before = cum.cpu().numpy(), fin.cpu().numpy()
        logits = d((rng.standard_normal((BK, V)) * 2).astype(np.float32))
        a.logits, a.step = logits.data_ptr(), S + t
        capi.check(capi.lib().ftcf_beam_search_step(C.byref(a), None))
        torch.cuda.synchronize()
        trace.append(dict(before=before, fin_before=fin_before, after=cum.cpu().numpy(), parents=par[S + t].cpu().numpy()))
    end = dict(output_ids=ids.cpu().numpy(), parent_ids=par.cpu().numpy(), finished=fin.cpu().numpy(), seq_len=seq.cpu().numpy(),
               cum_log_probs=cum.cpu().numpy(), cache_indir=indir.cpu().numpy())
    return trace, end, (lp.cpu().numpy() if record else None), S


@pytest.mark.parametrize("B,K,V,kw", STEP_CASES, ids=lambda v: str(v) if isinstance(v, int) else "args")
def test_the_step_records_new_cum_minus_the_parents_old_cum_to_the_bit(gh, B, K, V, kw):
    trace, end, lp, S = run_steps(B, K, V, kw, record=True)
    BK = B * K
    zero_rows = 0
    for t, st in enumerate(trace):
        pb = (np.arange(BK) // K) * K + st["parents"]
        want = step_differences(st["before"], st["after"], st["parents"], K)
        print(f"step {S + t}: parents {st['parents'].tolist()[:8]} recorded {lp[S + t].tolist()[:8]}")
        assert bits(lp[S + t]).tolist() == bits(want).tolist(), (t, lp[S + t], want)
        from_finished = st["fin_before"][pb] != 0
        zero_rows += int(from_finished.sum())
        assert (bits(lp[S + t])[from_finished] == 0).all(), "a finished beam's value is +0.0"
    assert zero_rows > 0, "the case selects a finished beam's end token"
    untouched = np.ones(lp.shape[0], bool)
    untouched[S:S + len(trace)] = False
    assert (bits(lp[untouched]) == bits(PATTERN)).all(), "rows the steps did not write"
    # the same steps with the pointer NULL: every other output bit for bit
    trace0, end0, _, _ = run_steps(B, K, V, kw, record=False)
    for key in end:
        assert end[key].tobytes() == end0[key].tobytes(), key
    for st, st0 in zip(trace, trace0):
        assert st["after"].tobytes() == st0["after"].tobytes() and st["parents"].tolist() == st0["parents"].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the engine against the replay of its own logits
# ---------------------------------------------------------------------------------------------------------------------
def replay_values(cfg, ids, lens, n_new, K, gpu_logits, bp):
    """(tokens, lengths, values, from_cell) of the hypotheses: the oracle's beam layer on the GPU's logits gives cum before every
    step and the parents; the fp32 differences go through the reference walk."""
    B, S = ids.shape
    total, BK = S + n_new, B * K
    o_ids, o_len, o_cum, tr = _replay(cfg, ids, lens, n_new, K, gpu_logits, bp)
    steps = tr["ids"].shape[0]
    out = np.zeros((total, BK), np.int32)
    par = np.zeros((total, BK), np.int32)
    pay = np.zeros((total, BK), np.float32)
    for bb in range(BK):
        out[:S, bb] = ids[bb // K]
    for t in range(steps):
        after = tr["cum"][t + 1] if t + 1 < steps else o_cum.reshape(-1)
        out[S + t], par[S + t] = tr["ids"][t], tr["parents"][t]
        pay[S + t] = step_differences(tr["cum"][t], after, tr["parents"][t], K)
    r_ids, r_len, val, src = gather_tree_with_payload(out, par, pay, o_len.reshape(-1) - 1, np.repeat(np.asarray(lens, np.int32), K), K,
                                                      S, cfg["end_id"])
    assert r_ids.tolist() == o_ids.tolist() and r_len.tolist() == o_len.tolist()
    return r_ids, r_len, val, src, o_cum


def check_against_replay(gh, op, cfg, ids, lens, n_new, K, kw):
    B = ids.shape[0]
    r = gh.run_op_beam(op, ids, lens, n_new, cfg["vocab_size"], K, return_logits=True, **kw)
    got = op.beam_log_probs().cpu().numpy()
    assert got.shape == (B, K, n_new) and got.dtype == np.float32
    okw = {k: v for k, v in kw.items() if k != "beam_search_diversity_rate"}
    bp = orc.BeamParams(B, diversity_rate=kw.get("beam_search_diversity_rate"), **okw)
    r_ids, r_len, val, src, _ = replay_values(cfg, ids, lens, n_new, K, r["logits"], bp)
    assert r["output_ids"].tolist() == r_ids.tolist()
    assert r["sequence_lengths"].tolist() == r_len.tolist()
    print("max |gpu - replay|", float(np.abs(got - val).max()), "cells", int(src.sum()), "of", src.size)
    np.testing.assert_allclose(got, val, rtol=1e-5, atol=1e-4)
    assert (bits(got)[~src] == 0).all(), "exactly 0 where the tree takes no token from a cell"
    for b in range(B):
        for k in range(K):
            toks = r["output_ids"][b, k, lens[b]:lens[b] + n_new]
            ends = np.flatnonzero(toks == cfg["end_id"])
            ends = ends[ends + lens[b] >= ids.shape[1]]  # (the tree's scan starts at row max_input_len, as written)
            if ends.size:
                assert (bits(got[b, k, ends[0] + 1:]) == 0).all(), (b, k, toks, got[b, k])
    return r, got, src


@pytest.mark.parametrize("kw", [
    dict(),
    dict(temperature=[0.8, 0.6], repetition_penalty=[1.2, 1.5], beam_search_diversity_rate=[-0.2, 0.0], len_penalty=0.3),
], ids=["plain", "args"])
def test_engine_values_follow_the_replay_of_its_own_logits(gh, tiny, kw):
    cfg, w, g = tiny
    cfg = dict(cfg, end_id=_pick_end_id(g, "b"))
    op = gh.make_op(cfg, w)
    ids, lens = g["ids_b"], g["lens_b"]
    r, got, src = check_against_replay(gh, op, cfg, ids, lens, 10, 4, kw)
    assert (r["output_ids"][0, :, lens[0]:lens[0] + 10] == cfg["end_id"]).any(), "the case really finishes beams"
    assert not src.all() and src.any()


def test_fp32_engine_values_follow_the_replay(gh, tiny):
    cfg, w, g = tiny
    cfg = dict(cfg, end_id=_pick_end_id(g, "b"))
    op = gh.make_op(cfg, w, dtype=torch.float32)
    check_against_replay(gh, op, cfg, g["ids_b"], g["lens_b"], 10, 4, dict())


def test_mid_int8_engine_values_follow_the_replay(gh):
    cfg, B, K, S, n_new = MID, 2, 4, 29, 10
    w = random_model(cfg, seed=38, std=0.04)
    rng = np.random.RandomState(B * 7 + K)
    lens = rng.randint(12, S + 1, size=B).astype(np.int32)
    lens[0] = S
    ids = np.full((B, S), cfg["end_id"], dtype=np.int32)
    for b in range(B):
        ids[b, :lens[b]] = rng.randint(3, cfg["vocab_size"], size=lens[b])
    op = gh.make_op(cfg, w, int8_mode=1)
    check_against_replay(gh, op, cfg, ids, lens, n_new, K, dict())


# ---------------------------------------------------------------------------------------------------------------------
# 3. telescoping: no replay needed
# ---------------------------------------------------------------------------------------------------------------------
def assert_telescopes(log_probs, cum):
    """Every value is one rounded subtraction (relative error <= 2^-24) and the differences telescope along the parent chain
    from 0: the float64 sum is the hypothesis' cum_log_probs within 2^-23 * sum |values| (twice the derived bound)."""
    lp = np.asarray(log_probs, np.float64)
    total, bound = lp.sum(-1), 2.0 ** -23 * np.abs(lp).sum(-1)
    err = np.abs(total - np.asarray(cum, np.float64))
    print("telescoping: max err", float(err.max()), "bound", float(bound.min()))
    assert (err <= bound).all(), (err, bound)


@pytest.mark.parametrize("kw", [dict(), dict(temperature=[0.8, 0.6], beam_search_diversity_rate=[-0.2, 0.0])], ids=["plain", "args"])
def test_the_values_of_a_hypothesis_sum_to_its_cum_log_probs(gh, tiny, kw):
    cfg, w, g = tiny
    ids, lens, K, n_new = g["ids_b"], g["lens_b"], 4, 10
    op = gh.make_op(cfg, w)
    free = gh.run_op_beam(op, ids, lens, n_new, cfg["vocab_size"], K, **kw)
    end_id = next(t for t in range(cfg["vocab_size"]) if not (free["output_ids"] == t).any())  # an end id no beam emits
    cfg = dict(cfg, end_id=end_id)
    op = gh.make_op(cfg, w)
    r = gh.run_op_beam(op, ids, lens, n_new, cfg["vocab_size"], K, **kw)
    assert (r["sequence_lengths"] == ids.shape[1] + n_new).all()
    got = op.beam_log_probs().cpu().numpy()
    assert (got != 0).all()
    assert_telescopes(got, r["cum_log_probs"])


# ---------------------------------------------------------------------------------------------------------------------
# 4. nothing else moves; the getter's edges
# ---------------------------------------------------------------------------------------------------------------------
def test_the_getter_changes_nothing_and_refuses_what_it_cannot_serve(gh, tiny):
    from fastertransformer4codefuse_amd import capi
    cfg, w, g = tiny
    cfg = dict(cfg, end_id=_pick_end_id(g, "b"))
    ids, lens, K, n_new = g["ids_b"], g["lens_b"], 4, 10
    B = ids.shape[0]
    L = capi.lib()
    op = gh.make_op(cfg, w)
    buf = torch.zeros(B * K * n_new, dtype=torch.float32, device="cuda")
    assert L.ftcf_gptneox_beam_log_probs(op._h, buf.data_ptr(), buf.numel()) == -1, "no request has run"
    with pytest.raises(capi.FtcfError):
        op.beam_log_probs()
    plain = gh.run_op_beam(op, ids, lens, n_new, cfg["vocab_size"], K)
    r = gh.run_op_beam(op, ids, lens, n_new, cfg["vocab_size"], K)
    a = op.beam_log_probs().cpu().numpy()
    b = op.beam_log_probs().cpu().numpy()
    assert a.tobytes() == b.tobytes()
    again = gh.run_op_beam(op, ids, lens, n_new, cfg["vocab_size"], K)
    for key in ("output_ids", "sequence_lengths", "cum_log_probs"):
        assert plain[key].tobytes() == r[key].tobytes() == again[key].tobytes(), key
    assert L.ftcf_gptneox_beam_log_probs(op._h, buf.data_ptr(), buf.numel() - 1) == -1 and b"capacity" in L.ftcf_last_error()
    assert L.ftcf_gptneox_beam_log_probs(op._h, None, buf.numel()) == -1  # FTCF_ERR_INVALID_ARG
    assert L.ftcf_gptneox_beam_log_probs(op._h, buf.data_ptr(), buf.numel()) == 0
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == a.tobytes()
    gh.run_op(op, ids, lens, 4, cfg["vocab_size"], top_k=1)  # beam_width 1
    assert L.ftcf_gptneox_beam_log_probs(op._h, buf.data_ptr(), buf.numel()) == -1
    with pytest.raises(capi.FtcfError):
        op.beam_log_probs()
