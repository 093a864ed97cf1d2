"""CPU (-m "not gpu"): what the float64 reference of beam search's decode attention (tests/attention_reference.py) can see.

tests/test_gpu_beam_attention.py plants no keys: every cache row holds random values of its own, and the test relies on one
key read from a wrong beam's row moving the context by far more than the bound.  That is checked here, on the reference alone:
redirecting ONE generated key of a row to a neighbouring beam moves the worst element of every (row, head) of every case by at
least 5 x CTX_ULPS; ignoring the indirection replaces nearly every key of a row, so its context becomes an unrelated vector (a
distance of about its own size, 1024 ulps and more): at least 100 x CTX_ULPS for every (row, head) is asked."""
import numpy as np
import pytest

from tests.attention_reference import (BEAM_CASES, CTX_FLOOR, CTX_ULPS, FP32_CASES, PICKED_SPLITS, _ulps, beam_case, beam_reference, beam_source_rows,
                                       in_registers)

_GENERATED = [n for n, (kw, _) in BEAM_CASES.items() if kw["tl"] > kw["max_input_len"]]


def _moved(c, ref, other):
    """per live (row, head): the worst element's distance between two references, in the ulps the GPU test counts"""
    out = {}
    for b in range(c["rows"]):
        if not c["fin"][b]:
            e = _ulps(other[0][b], ref[0][b], CTX_FLOOR * ref[3][b])
            for h in range(c["nh"]):
                out[b, h] = float(e[h].max())
    return out


@pytest.mark.parametrize("name", _GENERATED)
def test_one_key_from_a_neighbouring_beam_shows(name):
    c = beam_case(**BEAM_CASES[name][0])
    ref = beam_reference(c)
    K, mil, tl, plane = c["K"], c["max_input_len"], c["tl"], (c["step"] - c["max_input_len"]) & 1
    low = []
    for trial in range(6):
        rng = np.random.RandomState(1000 + trial)
        ind = c["indir"].copy()
        for b in range(c["rows"]):
            t = rng.randint(mil, tl)
            ind[plane, b, t] = (ind[plane, b, t] + 1) % K
        moved = _moved(c, ref, beam_reference(c, ind))
        low.append(min(moved.values()))
        assert low[-1] >= 5 * CTX_ULPS, (name, trial, min(moved, key=moved.get), low[-1])
    print(f"[{name}: one redirected key moves every (row, head) by >= {min(low):.0f} ulp] ", end="")


@pytest.mark.parametrize("name", _GENERATED)
def test_ignoring_the_indirection_shows(name):
    c = beam_case(**BEAM_CASES[name][0])
    ref = beam_reference(c)
    moved = _moved(c, ref, beam_reference(c, None))
    for (b, h), e in moved.items():
        own = (beam_source_rows(c["indir"], c["K"], c["max_input_len"], c["step"], b, c["tl"]) == b).all()
        assert (own and b % c["K"] == 0) or e >= 100 * CTX_ULPS, (name, b, h, e)  # (own: beam 0 of F2, whose one generated key may be its own)
    print(f"[{name}: without the indirection every (row, head) moves by >= {min(moved.values()):.0f} ulp] ", end="")


def test_cases_reach_the_forms_they_are_named_for():
    """registers / looped per case as the kernel decides it, the indirection's range, the NaN fill and the fp32 subset"""
    want = {"A1": [True], "A2": [True], "B": [False], "C": [False], "D": [True], "E": [True, False], "J": [False]}
    for name, (kw, splits) in BEAM_CASES.items():
        forms = [in_registers(kw["dh"], kw["s_max"], s or PICKED_SPLITS) for s in splits]
        if name in want:
            assert forms == want[name], name
        if name.startswith("H"):
            assert forms == [False, True], name
        assert all(s == 0 or kw["s_max"] > (s - 1) * 16 for s in splits)
    for name in ("A1", "A2", "F0", "G2x33"):
        c = beam_case(**BEAM_CASES[name][0])
        K, tl, mil = c["K"], c["tl"], c["max_input_len"]
        plane = (c["step"] - mil) & 1
        assert c["indir"].shape == (2, c["rows"], c["s_max"]) and c["indir"].min() >= 0 and c["indir"].max() < K
        assert (c["indir"][plane, :, :mil] == 0).all() and (c["indir"][1 - plane] == (c["indir"][plane] + 1) % K).all()
        assert np.isnan(c["kc"].view(np.float16)[:, :, tl:]).all() and np.isfinite(c["kc"].view(np.float16)[:, :, :tl]).all()
        assert np.isnan(c["vc"].view(np.float16)[:, :, tl:]).all() and np.isfinite(c["vc"].view(np.float16)[:, :, :tl]).all()
    for name in ("G2x33", "G1x64"):  # mmha_pick_nsplit: aim for 640 workgroups, at least 64 keys per split, at most 16 splits
        kw = BEAM_CASES[name][0]
        rows_heads = kw["batch"] * kw["K"] * kw["nh"]
        assert PICKED_SPLITS == max(1, min(-(-640 // rows_heads), -(-kw["s_max"] // 64), 16))
    assert BEAM_CASES["A1"][0]["tl"] % 2 != BEAM_CASES["A2"][0]["tl"] % 2
    c = beam_case(fp32=True, **BEAM_CASES["F2"][0])
    assert np.isnan(c["kc"].view(np.float32)[:, :, 2:]).all() and np.isfinite(c["kc"].view(np.float32)[:, :, :2]).all()
    assert set(FP32_CASES) <= set(BEAM_CASES)
