"""-m gpu: the tiled MFMA GEMM (launch_gemm_tiled / k_gemm_tiled, csrc/kernels_gemm.hip) in every launch form, through the entry
points the engine's dispatch sits behind (include/ftcf.h ftcf_fpA_intB_gemm / ftcf_fp16_gemm), against (a) the exact integer
result, bit for bit, and (b) a float64 product of the same half inputs, in half ulps.

The cases come from tests/tiled_gemm_cases.py; test_gemm_tiled_plan_host.py holds that table to the launcher's own decision
(ftcf_gemm_tiled_plan), so a form is not lost when a threshold moves.  Every failure message carries the form the case ran in.

The kernel accumulates in fp32 throughout (v_mfma_f32_16x16x32_f16 accumulators in consume_tile_raw, the fp32 adds of the split-K
partial tiles in slice order, one conversion to half in the epilogue; int8 weights are dequantised as half(q) * scale in half,
exact for |q| <= 3 and a power-of-two scale): with the exact inputs of tests/kernel_inputs.py the result does not depend on the
order of any sum, so a mismatch is a dropped, doubled or misplaced term -- the last k-step of a ragged slice, a clamped duplicate
row, a slice added twice after a ticket was re-armed.  {-1, 0, 1} x {-3..3} sums have sigma ~ 1.63 sqrt(k) units, ~117 at k = 5120,
and a bias adds at most 64: far below the 2048 units up to which a half is exact (assert_units checks each case).

Out of scope: the split-K family's fall-back when gx * gy exceeds its 4096 tickets (n ~ 175 000).

Which forms the engine reaches.  Before this file the kernel-level tests (test_gpu_kernels.py, test_gpu_headline_shapes.py) ran
Gaussian data at rtol 1e-3 / atol 2e-3 on a fixed shape list and could not tell which form they ran; exact inputs reached two
forms at most (k = 128, n = 256).  By the launcher's rules (gemm_tiled_plan) and the callers' workspaces:
  split-K, 32 / 48 / 64 / 128-row tiles: every prompt phase of 17 .. 384 (int8) / 768 (fp16) tokens (engine.hip.h plans the
    workspace whenever the prompt phase has more than 16 rows), the continuous batcher's decode steps above 16 rows on its main
    stream, and the speculative verify pass.  13B (k = 5120, 20480: k / 64 a multiple of 4): the ring of four, e.g. the
    out-projection at <= 64 rows is 7 slices of 12 k-steps with a last slice of 8.  The plain split-K loop and its ragged slices
    need k / 64 not a multiple of 4: a tensor-parallel rank's out-projection at TP = 8 (k = 640), or a model whose hidden size is
    not a multiple of 256.
  one workgroup per tile: prompt phases above those row counts.  13B: 64-row tiles at n = 5120 (out-projection, FFN2) up to 896
    rows and at 1025 .. 1536 rows, 128-row tiles else; lone (prefetch) where that gives at most 256 tiles (n = 5120 up to 768
    rows and at 897 .. 1024), not lone (int8: two per CU) for QKV and FFN1; the plain loop only where k / 64 is odd (no 13B GEMM; TP
    ranks and small models).
  four-wave: fp16 weights, prompt phases from 2048 tokens (128-row tiles, i.e. not the n = 5120 GEMMs at 1025 .. 1536 rows).
  32-row form, and one workgroup per tile at 33 .. 768 rows: a caller that passes no workspace -- the continuous batcher's
    overlapped decode step runs its second micro-batch's GEMMs on a second stream without one (batcher.hip: `s2 == st ? tiled_ws
    : nullptr`), and a batcher whose max_batch exceeds the split-K row limit holds none; also FTCF_GEMM_SPLITK=0 (a switch for
    measurements).
  n = 16 / 272 and other column counts that are no multiple of 256: the entry points accept any n % 16 == 0; the 13B shapes are all
    multiples of 256, a tensor-parallel slice or a small model need not be.

Gaussian inputs (weights N(0, 0.02) through the real quantiser, activations N(0, 1), no epilogue): error in half ulps at
max(|ref|, S / 128), S = sum |a||w| (kernel_inputs.ulps), against half(float64 product).  ORACLE_ULPS is the worst value of the
project's CPU restatement (orc.gemm) on exactly these cases, measured on the CPU: see the figures at the constant.  The kernel
gets one more: another summation order may land on the other side of one rounding boundary; split-K adds fp32 partials and rounds
once, so it earns no further allowance."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import kernel_inputs as ki
from tests import tiled_gemm_cases as tc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

# orc.gemm against half(float64 product) on the one-case-per-form list (52 cases), measured on the CPU: 0 .. 1.00 ulp, the worst
# 1.00 ulp in each of the four parts (int8 / fp16 x split-K / other).  Kernel on MI355X over the same list: 0 .. 1.00 ulp, the worst 1.00 ulp in
# each part too
ORACLE_ULPS = 1
KERNEL_ULPS = ORACLE_ULPS + 1

PAD_ROWS = 16  # rows of the output buffer past m: they must keep the sentinel (the kernels compute clamped duplicate rows there)
capi = None


@pytest.fixture(scope="module", autouse=True)
def _lib():
    global capi
    from fastertransformer4codefuse_amd import capi as _c
    capi = _c
    capi.require_gpu()
    yield


def sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def gemm(monkeypatch, c, p):
    """one launch of problem p in the form of case c, through the public entry point of its weight type"""
    W = p.W
    assert (W.int8, p.m, W.n, W.k) == (c.int8, c.m, c.n, c.k)
    with monkeypatch.context() as mp:
        if c.splitk is None:
            mp.delenv("FTCF_GEMM_SPLITK", raising=False)
        else:
            mp.setenv("FTCF_GEMM_SPLITK", c.splitk)  # (the launcher reads it at every call)
        act = 1 if p.epi == 2 else 0
        if W.int8:
            capi.check(capi.lib().ftcf_fpA_intB_gemm(capi.vp(p.dA), capi.vp(W.W), capi.vp(W.scale), capi.vp(p.dB), act, capi.vp(p.dC),
                                                     p.m, W.n, W.k, sp()))
        else:
            capi.check(capi.lib().ftcf_fp16_gemm(capi.vp(p.dA), capi.vp(W.W), capi.vp(p.dB), act, capi.vp(p.dC), p.m, W.n, W.k, sp()))


def tag(c, epi):
    return (tc.case_id(c), f"epilogue {epi}", tc.describe(tc.plan(capi, c)))


def seed(c):
    return c.m + 3 * c.n + 7 * c.k + int(c.int8) + (0 if c.splitk is None else 1000)


def problem(rng, W, c, epi):
    return ki.GemmProblem(rng, W, c.m, epi, c.m + PAD_ROWS)


@pytest.mark.parametrize("g", tc.GROUPS, ids=tc.group_id)
def test_tiled_gemm_is_bit_exact_on_exact_inputs(g, monkeypatch):
    """every case of the table on one weight matrix per group: no epilogue and a bias, new activations each; the output equals
    half(acc * unit) bit for bit, rows >= m keep their sentinel, and a second launch gives the same bits.  The FTCF_GEMM_SPLITK=0
    cases (the 32-row and non-split forms at 17 .. 64 and 200 rows) equal the same integers, hence the split-K run."""
    rng = np.random.RandomState(g.k + g.n + g.int8)
    W = ki.Weights(capi, rng, g.k, g.n, g.int8, exact=True)
    for c in g.cases:
        for epi in (0, 1):
            p = problem(rng, W, c, epi)
            gemm(monkeypatch, c, p)
            out = p.check(ORACLE_ULPS, KERNEL_ULPS, tag=tag(c, epi))
            gemm(monkeypatch, c, p)
            assert np.array_equal(p.got(), out), ("a repeated launch changed bits", tag(c, epi))


@pytest.mark.parametrize("int8", [True, False], ids=["int8", "fp16"])
def test_split_k_launches_of_different_grids_share_the_workspace_and_tickets(int8, monkeypatch):
    """A, B, A, C, A, B on one stream: split-K launches of different (gx, gy, slices) through the one workspace and ticket table the
    entry points keep per device and stream -- B's partial tiles land on A's and B takes tickets A re-armed.  New activations
    every time, every result exact."""
    last = max(c.m for c in tc.CASES if c.int8 == int8 and c.splitk is None and tc.plan(capi, c).family == tc.SPLITK)
    A, B, Cc = tc.Case(int8, 129, 272, 5120, None), tc.Case(int8, 17, 5120, 1088, None), tc.Case(int8, last, 1280, 4160, None)
    assert {A, B, Cc} <= set(tc.CASES)
    plans = [tc.plan(capi, c) for c in (A, B, Cc)]
    assert all(p.family == tc.SPLITK and p.slices > 1 for p in plans)
    assert len({(p.gx, p.gy, p.slices) for p in plans}) == 3 and len({p.gx for p in plans}) == 3 and len({p.slices for p in plans}) == 3
    rng = np.random.RandomState(41 + int8)
    Ws = {c: ki.Weights(capi, rng, c.k, c.n, int8, exact=True) for c in (A, B, Cc)}
    probs = []
    for i, c in enumerate((A, B, A, Cc, A, B)):
        p = problem(rng, Ws[c], c, i % 2)
        gemm(monkeypatch, c, p)  # (no synchronisation in between: the launches queue up on the stream)
        probs.append((c, p))
    for c, p in probs:
        p.check(ORACLE_ULPS, KERNEL_ULPS, tag=tag(c, p.epi))


def _first_of_each_family():
    """(resolved when the test runs: the table needs the library)"""
    seen, out = set(), []
    for c in tc.CASES:
        key = (c.int8, tc.plan(capi, c).family, c.splitk)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def test_bias_gelu_epilogue_in_every_family(monkeypatch):
    """bias + gelu is not exact: Gaussian inputs against orc.gemm at the tolerances of test_gpu_kernels.py (rtol 1e-3, atol 2e-3),
    the first case of the table in each family, with and without FTCF_GEMM_SPLITK=0, for both weight types"""
    cases = _first_of_each_family()
    assert {(c.int8, tc.plan(capi, c).family) for c in cases} >= {(True, tc.SPLITK), (True, tc.ROWS32), (True, tc.ONE_WG), (False, tc.SPLITK),
                                                                  (False, tc.ROWS32), (False, tc.ONE_WG), (False, tc.FOUR_WAVE)}
    for c in cases:
        rng = np.random.RandomState(5 + seed(c))
        W = ki.Weights(capi, rng, c.k, c.n, c.int8, exact=False)
        p = problem(rng, W, c, 2)
        gemm(monkeypatch, c, p)
        p.check(ORACLE_ULPS, KERNEL_ULPS, tag=tag(c, 2))


PARTS = {"split-K": lambda f: f == tc.SPLITK, "other": lambda f: f != tc.SPLITK}


@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("int8", [True, False], ids=["int8", "fp16"])
def test_tiled_gemm_gaussian_inputs_within_ulps_of_float64(int8, part, monkeypatch):
    """one case per form of the host test's list (tiled_gemm_cases.one_case_per_form), no epilogue"""
    cases = [c for c in tc.one_case_per_form(capi) if c.int8 == int8 and PARTS[part](tc.plan(capi, c).family)]
    assert cases
    worst = [0.0, 0.0]
    for c in cases:
        rng = np.random.RandomState(seed(c))
        W = ki.Weights(capi, rng, c.k, c.n, c.int8, exact=False)
        p = problem(rng, W, c, 0)
        gemm(monkeypatch, c, p)
        p.check(ORACLE_ULPS, KERNEL_ULPS, worst, tag=tag(c, 0))
    print(f"[worst: oracle {worst[0]:.2f} ulp, kernel {worst[1]:.2f} ulp] ", end="")
