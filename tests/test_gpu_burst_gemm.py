"""-m gpu: the batched-decode GEMM in the form the ENGINE launches it (include/ftcf.h ftcf_gemm_smallm_group ->
launch_gemm_smallm_group -> k_gemm_smallm_burst: K slices of 20 tiles, {tag, value} granules, the owner of the last slice
reduces, one launch for up to two GEMMs, partial_offset for two streams on one workspace, tag = device step + launch counter)
against (a) the exact integer result, bit for bit, and (b) a float64 product of the same half inputs, in half ulps.

The kernel accumulates in fp32 throughout (v_mfma_f32_16x16x32_f16 accumulators in consume_tile_raw, fp32 adds of the granules
and of the reducer's own sums, one conversion to half in smallm_epilogue; the int8 weights are dequantised as half(q) * scale in
half, which is exact for |q| <= 3 and a power-of-two scale): with the exact inputs of tests/kernel_inputs.py the result does not
depend on the order of any sum."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import kernel_inputs as ki

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

# Gaussian inputs: error in half ulps at max(|ref|, S / 128), S = sum |a||w| (kernel_inputs.ulps), against half(float64 product).
# ORACLE_ULPS bounds the project's CPU restatement (orc.gemm on the same inputs); measured on the CPU at m = 16, n = 256,
# k = 1344 / 5120 / 20480: int8 0 / 0 / 0 ulp, fp16 1 / 0 / 0 ulp.  The kernel gets one more: another summation order may land
# on the other side of one rounding boundary.  Worst measured on MI355X over every case below: oracle 1.00 ulp, kernel 1.00 ulp.
ORACLE_ULPS = 1
KERNEL_ULPS = ORACLE_ULPS + 1

SMB_T = 20  # tiles per slice (kernels_gemm.hip)
capi = None


@pytest.fixture(scope="module", autouse=True)
def _lib():
    global capi
    from fastertransformer4codefuse_amd import capi as _c
    capi = _c
    capi.require_gpu()
    yield


def L():
    return capi.lib()


def sp(stream=None):
    return C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


dev16 = ki.dev16


def slices(k, int8):
    kt = k // (64 if int8 else 32)
    return (kt + SMB_T - 1) // SMB_T


def ws_bytes(m, n, k, int8):
    return int(L().ftcf_gemm_smallm_workspace_bytes(m, n, k, int(int8)))


class Workspace:
    """[partial_bytes of granules][ticket bytes], zeroed once, and the workspace's launch counter"""

    def __init__(self, partial_bytes, seq=0):
        self.partial_bytes = int(partial_bytes)
        self.buf = torch.zeros(self.partial_bytes + int(L().ftcf_gemm_smallm_ticket_bytes()), dtype=torch.uint8, device="cuda")
        self.seq = C.c_uint(seq)

    def err(self):
        torch.cuda.synchronize()
        return int(self.buf[self.partial_bytes:self.partial_bytes + 4].view(torch.int32).item())


ROWS = 17  # rows of every output buffer: rows >= m must keep the sentinel


class Problem(ki.GemmProblem):
    """one GEMM on new activations (kernel_inputs.GemmProblem) as a descriptor of the group launch; ROWS output rows"""

    def __init__(self, rng, W, m, epi):
        super().__init__(rng, W, m, epi, ROWS)

    def desc(self):
        return capi.SmallmProblem(A=self.dA.data_ptr(), W=self.W.W.data_ptr(), scale=0 if self.W.scale is None else self.W.scale.data_ptr(),
                                  bias=0 if self.dB is None else self.dB.data_ptr(), act=1 if self.epi == 2 else 0, C=self.dC.data_ptr(),
                                  n=self.W.n, k=self.W.k)

    def check(self, worst=None):
        return super().check(ORACLE_ULPS, KERNEL_ULPS, worst)


def launch(ws, probs, m, int8, d_step=None, offset=0, stream=None):
    arr = (capi.SmallmProblem * len(probs))(*[p.desc() for p in probs])
    capi.check(L().ftcf_gemm_smallm_group(arr, len(probs), m, int(int8), capi.vp(ws.buf), C.c_size_t(ws.partial_bytes), C.c_size_t(offset),
                                          capi.vp(d_step), C.byref(ws.seq), sp(stream)))


# k by slice count ks = ceil((k / TK) / 20): 1 (the direct epilogue), 2 (int8: 21 tiles -> 10 + 11), 4, 6 (one full reducer round of
# five siblings), 7 (one round plus one), 16; fp16 tiles are 32 k, and 44 of them make three uneven slices (14 + 15 + 15)
K_BY_SLICES = {True: {1: 1280, 2: 1344, 4: 5120, 6: 7040, 7: 8320, 16: 20480},
               False: {1: 640, 2: 704, 3: 1408, 4: 2560, 6: 3520, 7: 4160, 16: 10240}}
MS = (1, 5, 7, 15, 16)


def _shapes(ns, ks_list):
    out = []
    for int8 in (True, False):
        for n in ns:
            for ks in ks_list:
                if ks in K_BY_SLICES[int8]:
                    out.append(pytest.param(int8, n, K_BY_SLICES[int8][ks], id=f"{'int8' if int8 else 'fp16'}-n{n}-ks{ks}"))
    return out


@pytest.mark.parametrize("int8,n,k", _shapes((16, 80), (1, 2, 3, 4, 6, 7, 16)) + _shapes((5120,), (1, 2, 3, 16)))
def test_burst_gemm_is_bit_exact_on_exact_inputs(int8, n, k):
    """n 16: one active wave of four; 80: the last column block has one active wave (the reducer's cc >= n exit); 5120 (its slice
    counts 4, 6 and 7 run in the group, two-stream and workspace-reuse tests below, on exact inputs too).  Every m with
    no epilogue and with a bias; bias + gelu (not exact: the oracle's tolerance) at 7 rows.  One workspace and one advancing
    device step for the whole sequence; every launch repeated once: the same bits."""
    assert slices(k, int8) in K_BY_SLICES[int8] and K_BY_SLICES[int8][slices(k, int8)] == k
    rng = np.random.RandomState(n + k + int8)
    W = ki.Weights(capi, rng, k, n, int8, exact=True)
    ws = Workspace(ws_bytes(16, n, k, int8), seq=4090)
    step = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    for m in MS:
        for epi in (0, 1, 2) if m == 7 else (0, 1):
            p = Problem(rng, W, m, epi)
            launch(ws, [p], m, int8, d_step=step)
            out = p.check()
            step.add_(1)
            launch(ws, [p], m, int8, d_step=step)
            assert np.array_equal(p.got(), out), ("a repeated launch changed bits", m, epi)
    assert ws.err() == 0


@pytest.mark.parametrize("int8,n,k", _shapes((16,), (1, 2, 3, 7)) + _shapes((80,), (1, 2, 3, 4, 6, 7, 16)) + _shapes((5120,), (4,)))
def test_burst_gemm_gaussian_inputs_within_ulps_of_float64(int8, n, k):
    """weights N(0, 0.02) through the real quantiser, activations N(0, 1); bias at 5 rows, bias + gelu at 16 rows."""
    rng = np.random.RandomState(3 * n + k + int8)
    W = ki.Weights(capi, rng, k, n, int8, exact=False)
    ws = Workspace(ws_bytes(16, n, k, int8))
    worst = [0.0, 0.0]
    for i, m in enumerate(MS):
        p = Problem(rng, W, m, 0)
        launch(ws, [p], m, int8, d_step=None)
        p.check(worst)
        if m in (5, 16):
            p = Problem(rng, W, m, 1 if m == 5 else 2)
            launch(ws, [p], m, int8, d_step=None)
            p.check()
    print(f"[worst: oracle {worst[0]:.2f} ulp, kernel {worst[1]:.2f} ulp] ", end="")
    assert ws.err() == 0


@pytest.mark.parametrize("int8", [True, False], ids=["int8", "fp16"])
@pytest.mark.parametrize("m", [5, 16])
def test_a_group_of_two_equals_two_single_launches(int8, m):
    """np = 2 with different (n, k, act) per problem against the two np = 1 launches, bit for bit, on exact inputs (the bias-only /
    no-epilogue problem also against the integer result).  The second problem's scales differ from the first one's."""
    rng = np.random.RandomState(100 + m + int8)
    kk = K_BY_SLICES[int8]
    for (n0, k0, e0), (n1, k1, e1) in ((((5120, kk[2], 0)), (80, kk[4], 2)), ((80, kk[7], 1), (16, kk[2], 0)), ((80, kk[1], 0), (80, kk[6], 1))):
        W0, W1 = ki.Weights(capi, rng, k0, n0, int8, True), ki.Weights(capi, rng, k1, n1, int8, True)
        p0, p1 = Problem(rng, W0, m, e0), Problem(rng, W1, m, e1)
        ws = Workspace(ws_bytes(m, n0, k0, int8) + ws_bytes(m, n1, k1, int8), seq=4094)
        launch(ws, [p0, p1], m, int8)
        g0, g1 = p0.check(), p1.check()
        launch(ws, [p0, p1], m, int8)
        assert np.array_equal(p0.got(), g0) and np.array_equal(p1.got(), g1), "a repeated group launch changed bits"
        for p, g in ((p0, g0), (p1, g1)):
            p.dC.copy_(dev16(p.sent))
            single = Workspace(ws_bytes(m, p.W.n, p.W.k, int8))
            launch(single, [p], m, int8)
            assert np.array_equal(p.got(), g), ("group != single launch", p.W.n, p.W.k)
            assert single.err() == 0
        assert ws.err() == 0


@pytest.mark.parametrize("int8", [True, False], ids=["int8", "fp16"])
@pytest.mark.parametrize("with_step", [True, False], ids=["d_step", "no_d_step"])
def test_one_workspace_serves_gemms_of_different_shapes_in_turn(int8, with_step):
    """GEMM X, then a GEMM of another (m, n) whose granules land on X's, then X again, each on new activations and each exact;
    the device step advances between launches and the launch counter crosses 0xfff during the sequence."""
    rng = np.random.RandomState(17 + int8)
    kk = K_BY_SLICES[int8]
    WX, WY = ki.Weights(capi, rng, kk[4], 80, int8, True), ki.Weights(capi, rng, kk[7], 5120, int8, True)
    ws = Workspace(max(ws_bytes(16, 80, kk[4], int8), ws_bytes(7, 5120, kk[7], int8)), seq=4090)
    step = torch.full((1,), 3, dtype=torch.int32, device="cuda") if with_step else None
    for rnd in range(3):
        for W, m in ((WX, 16), (WY, 7), (WX, 16), (WX, 5)):
            p = Problem(rng, W, m, rnd % 2)
            launch(ws, [p], m, int8, d_step=step)
            p.check()
            if with_step:
                step.add_(1)
    assert ws.seq.value == 4090 + 12 and ws.err() == 0


@pytest.mark.parametrize("int8", [True, False], ids=["int8", "fp16"])
def test_two_streams_share_one_workspace_and_counter(int8):
    """two launches on two streams with disjoint partial_offset regions of one workspace, one counter and one device step, as the
    engine's dual-chunk step for 17..32 rows does; exact inputs."""
    rng = np.random.RandomState(29 + int8)
    kk = K_BY_SLICES[int8]
    W = ki.Weights(capi, rng, kk[6], 5120, int8, True)
    m0, m1 = 16, 9
    off = ws_bytes(m0, 5120, kk[6], int8)
    ws = Workspace(off + ws_bytes(m1, 5120, kk[6], int8), seq=4093)
    step = torch.full((1,), 11, dtype=torch.int32, device="cuda")
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(4):
        p0, p1 = Problem(rng, W, m0, 1), Problem(rng, W, m1, 0)
        torch.cuda.synchronize()
        launch(ws, [p0], m0, int8, d_step=step, offset=0, stream=s0)
        launch(ws, [p1], m1, int8, d_step=step, offset=off, stream=s1)
        p0.check()
        p1.check()
        step.add_(1)
    assert ws.err() == 0


def test_bad_arguments_are_refused_before_any_launch():
    rng = np.random.RandomState(1)
    W = ki.Weights(capi, rng, 1344, 80, True, True)
    p = Problem(rng, W, 5, 0)
    ws = Workspace(ws_bytes(5, 80, 1344, True))

    def code(probs, m, partial=None, offset=0, np_=None):
        arr = (capi.SmallmProblem * len(probs))(*probs)
        return L().ftcf_gemm_smallm_group(arr, len(probs) if np_ is None else np_, m, 1, capi.vp(ws.buf),
                                          C.c_size_t(ws.partial_bytes if partial is None else partial), C.c_size_t(offset), None,
                                          C.byref(ws.seq), sp())

    d = p.desc()
    assert code([d], 17) == -1 and code([d], 0) == -1 and code([d], 5, np_=3) == -1
    assert code([d], 5, partial=ws.partial_bytes - 8) == -1  # workspace too small
    assert code([d], 5, offset=8) == -1                     # ... past its end
    for field, bad in (("n", 72), ("k", 1312), ("A", 0), ("scale", 0)):
        d2 = p.desc()
        setattr(d2, field, bad)
        assert code([d2], 5) == -1, field
    assert b"GEMM" in L().ftcf_last_error()
    launch(ws, [p], 5, True)  # the library stays usable and nothing was written meanwhile
    p.check()
    assert ws.err() == 0
