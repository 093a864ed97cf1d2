"""CPU (-m "not gpu"): the per-token log-probabilities of beam hypotheses -- the numpy yardstick (tests/beam_log_probs_reference.py)
against the oracle's gather tree on random trees, and the surface of the C ABI: the field appended to ftcf_beam_search_args,
ftcf_beam_options, the three new entry points."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library: one HIP runtime in the process)

from fastertransformer4codefuse_amd import capi
from oracle import oracle as orc
from tests.beam_log_probs_reference import gather_tree_with_payload, step_differences
from tests.test_capi_abi import CC, check_mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ftcf_gptneox_beam_log_probs", "ftcf_batcher_submit_beam_opts", "ftcf_batcher_beam_result_ex")


def random_tree(B, K, S, out_len, end_id, seed, ends_before_total):
    """A search that could have happened: ragged prompts, parents drawn per step, some beams ending on end_id early (their
    lengths stop growing, as update_kernel leaves them), and with ends_before_total every beam finished two steps early, so
    that the rows behind were never written."""
    rng = np.random.RandomState(seed)
    total, BK = S + out_len, B * K
    lens = rng.randint(max(1, S - 5), S + 1, size=B).astype(np.int32)
    lens[0] = S
    tl = np.repeat(lens, K)
    ids = np.zeros((total, BK), np.int32)
    par = np.zeros((total, BK), np.int32)
    for bb in range(BK):
        ids[:tl[bb], bb] = rng.randint(3, 50, size=tl[bb])
    seq = np.full(BK, S - 1, np.int32)
    fin = np.zeros(BK, bool)
    steps = out_len - (2 if ends_before_total else 0)
    for t in range(steps):
        step = S + t
        parent = rng.randint(0, K, size=BK)
        pb = (np.arange(BK) // K) * K + parent
        tok = rng.randint(3, 50, size=BK)
        tok[fin[pb]] = end_id  # (a finished parent offers its end token only)
        tok[rng.rand(BK) < 0.25] = end_id
        if ends_before_total and t == steps - 1:
            tok[:] = end_id
        seq = np.where(fin[pb], seq[pb], seq[pb] + 1).astype(np.int32)
        fin = tok == end_id
        ids[step], par[step] = tok, parent
    # a distinct payload in every cell: a value read from the wrong cell cannot pass
    payload = (1.0 + np.arange(total * BK, dtype=np.float32).reshape(total, BK)) / 8
    return ids, par, payload, seq, tl, lens


CASES = [(B, K, early) for B in (1, 3) for K in (2, 5) for early in (False, True)]


@pytest.mark.parametrize("B,K,early", CASES)
def test_reference_walk_returns_the_oracles_tokens_and_each_tokens_own_cell(B, K, early):
    S, out_len, end_id = 9, 8, 2
    ends_seen = rewrites = 0
    for seed in range(6):
        ids, par, payload, seq, tl, lens = random_tree(B, K, S, out_len, end_id, 100 * seed + 10 * B + K, early)
        o_ids, o_len = orc.gather_tree_beam(ids, par, seq, tl, K, S, end_id)
        r_ids, r_len, val, src = gather_tree_with_payload(ids, par, payload, seq, tl, K, S, end_id)
        assert r_ids.tolist() == o_ids.tolist() and r_len.tolist() == o_len.tolist()
        assert val.shape == (B, K, out_len) and val.dtype == np.float32
        assert ((val == 0) == ~src).all(), "0 exactly where the token was not read from a cell"
        for b in range(B):
            for k in range(K):
                toks = r_ids[b, k, lens[b]:lens[b] + out_len]
                for i in np.flatnonzero(src[b, k]):
                    level, slot = np.argwhere(payload == val[b, k, i])[0]  # (the payload names its cell)
                    assert level == S + i and slot // K == b and ids[level, slot] == toks[i]
                # behind the first end token the tree's scan meets (it starts at row S of the hypothesis): rewritten, no cell
                row = r_ids[b, k]
                hits = np.flatnonzero(row[S:min(int(seq[b * K:b * K + K].max()) + 1, S + out_len)] == end_id)
                if hits.size:
                    ends_seen += 1
                    first = S + hits[0] - lens[b]
                    rewrites += int((~src[b, k, first + 1:]).sum())
                    assert not src[b, k, first + 1:].any() and (val[b, k, first + 1:] == 0).all()
        if early:
            assert int(seq.max()) + 1 < S + out_len, "the request ended before total"
            assert (val[:, :, -1] == 0).all()
    assert ends_seen > 0 and rewrites > 0, "the trees end beams early"


def test_step_differences_are_one_fp32_subtraction_against_the_parents_old_score():
    before = np.array([0.0, -1e20, -3.25, -1.5], np.float32)
    after = np.array([-0.75, -1.25, -3.25, -4.0], np.float32)
    d = step_differences(before, after, np.array([0, 0, 0, 1]), 2)
    assert d.dtype == np.float32
    assert d.tolist() == [-0.75, -1.25, 0.0, np.float32(-4.0) - np.float32(-1.5)]
    assert not np.signbit(d[2])


@pytest.mark.skipif(CC is None, reason="no C compiler")
def test_the_appended_field_and_the_options_struct_sit_where_the_header_puts_them():
    check_mirror("ftcf_beam_search_args")  # (every field's offset and size and the struct's size: tests/test_capi_abi.py)
    check_mirror("ftcf_beam_options")
    A, O = capi.BeamSearchArgs, capi.BeamOptions
    assert A._fields_[-1][0] == "step_log_probs" and A._fields_[-2][0] == "end_id", "appended: the old fields keep their places"
    assert O._fields_[0][0] == "struct_size" and O.struct_size.offset == 0


def test_the_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ftcf.h")).read()
    assert "int ftcf_gptneox_beam_log_probs(ftcf_gptneox_t h, float* log_probs, size_t capacity);" in hdr
    assert "int ftcf_batcher_submit_beam_opts(ftcf_batcher_t b, const int* prompt_ids, int prompt_len, int max_new_tokens," in hdr
    assert "int ftcf_batcher_beam_result_ex(ftcf_batcher_t b, long request_id, int* output_ids, int* sequence_lengths" in hdr
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED and hasattr(L, name), name
        restype, argtypes = capi.PROTOTYPES[name]
        assert argtypes and list(getattr(L, name).argtypes) == argtypes and getattr(L, name).restype is restype is C.c_int, name
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    from fastertransformer4codefuse_amd.gptneox_op import GptNeoXOp
    p = list(inspect.signature(ContinuousBatcher.submit_beam).parameters.values())
    assert p[-1].name == "token_log_probs" and p[-1].default is False
    assert callable(GptNeoXOp.beam_log_probs)
    # GptNeoXOp.forward keeps its signature: the values come through the getter
    assert "beam_log_probs" not in inspect.signature(GptNeoXOp.forward).parameters


@pytest.mark.skipif(capi.device_count() > 0, reason="a HIP device is visible")
def test_without_a_device_the_entry_points_say_so():
    L = capi.lib()
    buf = (C.c_int * 64)()
    k, t, rid = C.c_int(0), C.c_int(0), C.c_long(0)
    o = capi.BeamOptions(struct_size=C.sizeof(capi.BeamOptions), beam_width=2, temperature=1.0, repetition_penalty=1.0)
    calls = [
        lambda: L.ftcf_gptneox_beam_log_probs(None, C.addressof(buf), 64),
        lambda: L.ftcf_batcher_submit_beam_opts(None, C.addressof(buf), 4, 4, C.byref(o), C.byref(rid)),
        lambda: L.ftcf_batcher_beam_result_ex(None, 0, None, None, None, None, 0, C.byref(k), C.byref(t)),
    ]
    for call in calls:
        assert call() == -5 and b"no HIP device" in L.ftcf_last_error()  # FTCF_ERR_NO_DEVICE


def test_zero_initialised_arguments_ask_for_nothing():
    assert not capi.BeamSearchArgs().step_log_probs
    assert capi.BeamOptions().token_log_probs == 0
