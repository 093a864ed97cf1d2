"""CPU: the float64 reference of the prompt-phase attention (tests/context_attention_reference.py) against the oracle, the mirror of
the launcher's key-split rule on the case table, and the condition on the inputs that makes the single-key probes of
tests/test_gpu_context_attention.py decisive."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.context_attention_reference import (CASES, CHAIN, CTX_FRAC, FP32_CASES, MEASURED, PROBE_SETS, SPLITS, case_and_reference,
                                               ctx_unit, probe_inputs, probe_list, probe_reference, split_count, split_cut)

_WHOLE = [(n, False) for n, kw in CASES.items() if kw.get("s_lo", 0) == 0 and kw.get("s_hi", kw["S"]) == kw["S"]] + [(n, True) for n in FP32_CASES]


@pytest.mark.parametrize("name,fp32", _WHOLE, ids=[n + ("-fp32" if f else "") for n, f in _WHOLE])
def test_reference_agrees_with_the_oracle_on_whole_prompts(name, fp32):
    """The oracle rounds P as the reference project does and the float64 reference rounds only where the kernel must: this ties
    the two together at the tolerance of the oracle tests of tests/test_gpu_kernels.py."""
    c, ref = case_and_reference(name, fp32)
    B, S, nh, dh = c["B"], c["S"], c["nh"], c["dh"]
    kc_o = np.zeros((B, nh, c["s_max"], dh), dtype=np.float32)
    vc_o = np.zeros_like(kc_o)
    o = orc.context_attention(c["qkv"].astype(np.float32).reshape(B * S, 3 * nh * dh), c["bias"].astype(np.float32).reshape(-1), c["lens"],
                              kc_o, vc_o, B, S, nh, dh, c["rot"], fp16=not fp32).reshape(B, S, nh, dh)
    for b in range(B):
        n = int(c["lens"][b])
        np.testing.assert_allclose(ref["ctx"][b].astype(np.float64), o[b, :n], rtol=1e-2, atol=2e-3)
        np.testing.assert_allclose(ref["k"][b].astype(np.float64).transpose(1, 0, 2), kc_o[b, :, :n], rtol=2e-3, atol=2e-3)
        np.testing.assert_array_equal(ref["v"][b].astype(np.float32).transpose(1, 0, 2), vc_o[b, :, :n])


def test_split_rule_mirror_and_the_table():
    assert set(SPLITS) <= set(CASES) and all(n in CASES for n in FP32_CASES + list(PROBE_SETS) + [CHAIN[0]])
    for name, kw in CASES.items():
        s_lo, s_hi = kw.get("s_lo", 0), kw.get("s_hi", kw["S"])
        assert split_count(kw["dh"], s_lo, s_hi) == SPLITS.get(name, 0), name
    # the launcher's rule on shapes worked out by hand: 8 tiles of 64 keys is the threshold; 1024 tokens split their last 8 blocks
    assert split_count(128, 0, 448) == 0 and split_count(128, 0, 449) == 4 and split_count(128, 0, 1024) == 8
    assert split_count(256, 0, 224) == 0 and split_count(256, 0, 225) == 2 and split_count(64, 449, 450) == 1
    assert split_cut(128, 449) == 256 and split_cut(128, 519) == 256 and split_cut(128, 463) == 256 and split_cut(256, 259) == 128
    for name, cut in PROBE_SETS.items():  # the probes' cut is that of every split block of the launch
        kw = CASES[name]
        blocks = [min(q0 + 63, kw["s_hi"] - 1) for q0 in range(kw["s_lo"], kw["s_hi"], 64)]
        assert (cut is None and name not in SPLITS) or (SPLITS[name] == len(blocks) and {split_cut(kw["dh"], q) for q in blocks} == {cut})
    assert CTX_FRAC == min(1.0, np.ceil(150 * MEASURED[0] - 1e-9) / 100)  # 1.5 x the measured worst, two digits, capped


@pytest.mark.parametrize("name", list(PROBE_SETS))
def test_every_probe_moves_every_later_row(name):
    """The probe condition, decided by the reference alone: a replaced VALUE of position j moves every context row i >= j of the
    range by more than 4 U on at least one element of every head, and no earlier row at all.  A replaced KEY cannot do that for
    every row whatever the seed -- where the new key scores low the change is the loss of the old weight, and among hundreds of
    keys some rows give that key next to none -- so for a key at least half the rows must move; the GPU test requires a changed
    bit of exactly the rows that move here."""
    c, ref = case_and_reference(name)
    s_lo = c["s_lo"]
    u = ctx_unit(ref, 0)
    for kind, j in probe_list(name):
        qkv, kc, vc = probe_inputs(c, kind, j)
        assert (qkv != c["qkv"]).sum() + (kc != c["kc"]).sum() + (vc != c["vc"]).sum() >= c["nh"] * c["dh"] - 2
        r_d = np.abs(probe_reference(name, kind, j)["ctx64"][0] - ref["ctx64"][0]) / u
        i0 = max(j - s_lo, 0)
        assert not r_d[:i0].any(), (kind, j)
        moved = r_d[i0:].max(axis=2).min(axis=1) > 4.0
        if kind == "v":
            assert moved.all(), (kind, j, np.flatnonzero(~moved)[:8].tolist(), float(r_d[i0:].max(axis=2).min()))
        else:
            assert 2 * moved.sum() >= moved.size, (kind, j, int(moved.sum()), moved.size)


def test_no_case_holds_a_non_finite_value_where_the_reference_reads():
    """reference_context asserts it of the keys and values it gathers; here: every input of every case outside the caches is finite,
    and so is every reference output"""
    for name in CASES:
        for fp32 in ((False, True) if name in FP32_CASES else (False,)):
            c, ref = case_and_reference(name, fp32)
            assert np.isfinite(c["qkv"].astype(np.float64)).all() and np.isfinite(c["bias"].astype(np.float64)).all()
            assert np.isfinite(c["ctx0"].view(c["ft"]).astype(np.float64)).all()
            for b in range(c["B"]):
                e = min(int(c["lens"][b]), c["s_hi"])
                assert (ref["ctx"][b] is None) == (e <= c["s_lo"]), (name, b)
                if ref["ctx"][b] is not None:
                    assert all(np.isfinite(np.asarray(ref[k][b], dtype=np.float64)).all() for k in ref), name
                    assert ref["ctx"][b].shape == (e - c["s_lo"], c["nh"], c["dh"])
