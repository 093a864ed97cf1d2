"""CPU (-m "not gpu"): the case table of the tiled GEMM's GPU test (tests/tiled_gemm_cases.py) reaches every launch form of
launch_gemm_tiled, as the launcher's own decision says (include/ftcf.h ftcf_gemm_tiled_plan: the host function the launcher
launches from, no device needed).  A threshold that a later change moves makes this test fail, naming the form or the row step the
table no longer covers, instead of the GPU test silently running another kernel.

Out of scope: the fall-back of the split-K family to the other forms when gx * gy exceeds its 4096 tickets (n ~ 175 000 at one row
block: no model's GEMM, and minutes of CPU reference)."""
import ctypes as C

import pytest

from fastertransformer4codefuse_amd import capi
from tests import tiled_gemm_cases as tc
from tests.test_capi_abi import CC, check_mirror

TYPE = {True: "int8", False: "fp16"}


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in ("FTCF_GEMM_SPLITK", "FTCF_GEMM_SK128_MIN_M"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.skipif(CC is None, reason="no C compiler")
def test_the_plan_struct_mirrors_the_header():
    check_mirror("ftcf_gemm_plan")


def test_the_query_needs_no_device_and_refuses_bad_shapes():
    p = capi.GemmPlan()
    L = capi.lib()
    assert L.ftcf_gemm_tiled_plan(64, 256, 128, 1, 1, C.byref(p)) == 0
    assert (p.family, p.tile_rows, p.gx, p.gy) == (tc.SPLITK, 64, 1, 1)
    for m, n, k in ((0, 256, 128), (64, 250, 128), (64, 256, 100), (64, 0, 128), (64, 256, 0)):
        assert L.ftcf_gemm_tiled_plan(m, n, k, 1, 1, C.byref(p)) == -1, (m, n, k)
    assert L.ftcf_gemm_tiled_plan(64, 256, 128, 1, 1, None) == -1


def test_the_plan_is_consistent_for_every_case():
    """what the kernel relies on: the grid covers every tile and slice, no slice is empty, a ring runs whole rounds"""
    for c in tc.CASES:
        p = tc.plan(capi, c)
        what = (tc.case_id(c), tc.describe(p))
        ksteps = c.k // 64
        assert p.gy * p.tile_rows >= c.m > (p.gy - 1) * p.tile_rows, what
        cols = 64 if p.family == tc.ROWS32 else 256
        assert p.gx * cols >= c.n > (p.gx - 1) * cols, what
        assert p.slices * p.steps_per_slice >= ksteps > (p.slices - 1) * p.steps_per_slice, what
        if p.family == tc.SPLITK:
            assert 1 <= p.slices <= 8 and p.grid == 8 * ((p.gx + 7) // 8) * p.gy * p.slices and p.ring in (0, 4), what
            assert p.ring == 0 or (ksteps % 4 == 0 and p.steps_per_slice % 4 == 0), what
            assert p.tile_rows in (32, 48, 64, 128) and (p.gy == 1 or p.tile_rows >= 64), what
        elif p.family == tc.ROWS32:
            assert c.m <= 32 and p.slices == 1 and p.ring == 0 and p.grid == p.gx * p.gy, what
        else:
            assert p.slices == 1 and p.tile_rows in (64, 128) and p.grid == 8 * ((p.gx + 7) // 8) * p.gy, what
            assert p.ring in (0, 2) and (p.ring == 0 or ksteps % 2 == 0), what
            assert p.lone == int(p.gx * p.gy <= 256), what
            if p.family == tc.FOUR_WAVE:
                assert not c.int8 and p.tile_rows == 128 and p.ring == 0 and p.two_per_cu == 1, what


def test_the_table_reaches_every_form():
    missing = [f"{TYPE[int8]}: {name}" for (name, int8), cases in tc.reached(capi).items() if not cases]
    assert not missing, "no case of tests/tiled_gemm_cases.py reaches: " + "; ".join(missing)


@pytest.mark.parametrize("int8", [True, False], ids=["int8", "fp16"])
def test_the_table_has_both_sides_of_every_row_step(int8):
    """the row counts at which the family or the tile height changes, found by asking the query for every m from 17 rows to one
    row block past the last split-K row count (the 32 / 33, 48 / 49, 64 / 65 steps, the switch to 128-row split-K tiles, the last
    split-K row count): the table holds a case with that family, tile height and one / several row blocks at the last m before
    and at the first m after"""
    n, k = 272, 5120
    last = tc.entry_workspace_max_m(capi)

    def shape(p):
        return p.family, p.tile_rows, p.family == tc.SPLITK and p.gy > 1  # (split-K: one row block / several)

    def form(m):
        return shape(tc.plan(capi, tc.Case(int8, m, n, k, None)))

    steps = [m for m in range(17, last + 128) if form(m) != form(m + 1)]
    families = [form(m)[0] for m in steps]
    assert len(steps) >= 5 and tc.SPLITK in families and form(steps[-1] + 1)[0] != tc.SPLITK, (steps, "the scan found no split-K range")
    have = {(c.m, shape(p)) for c in tc.CASES if c.int8 == int8 and c.splitk is None for p in [tc.plan(capi, c)]}
    for m in steps:
        for side in (m, m + 1):
            assert (side, form(side)) in have, (f"{TYPE[int8]}: the form changes between {m} and {m + 1} rows "
                                                f"({form(m)} -> {form(m + 1)}) and no case has m = {side} in that form")


def test_every_group_shares_one_weight_matrix_and_no_case_repeats():
    assert len(set(tc.CASES)) == len(tc.CASES)
    assert len({(g.int8, g.k, g.n) for g in tc.GROUPS}) == len(tc.GROUPS)
    for g in tc.GROUPS:
        assert g.cases and all((c.int8, c.k, c.n) == (g.int8, g.k, g.n) and c.m > 16 for c in g.cases)


def test_one_case_per_form_covers_every_form():
    picked = set(tc.one_case_per_form(capi))
    for (name, int8), cases in tc.reached(capi).items():
        assert picked & set(cases), (TYPE[int8], name)
