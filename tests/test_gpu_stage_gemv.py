"""-m gpu: the per-stage decode step's GEMV launches for 1..4 rows at kernel level (include/ftcf.h ftcf_ln_gemv -> launch_ln_gemv /
launch_ln_gemv_group; ftcf_residual_gemv -> plan_splitk + launch_gemv_splitk(EPI_RESIDUAL) / launch_gemv_chunked), as
stage_launch runs them, against exact integer inputs (tests/kernel_inputs.py) bit for bit and Gaussian inputs in half ulps of a
float64 product.

All of them accumulate in fp32 (consume_tile's v_mfma_f32_16x16x32_f16, the fp32 LDS / granule reductions) and round to half
once per GEMV result; the residual epilogue then adds in half (or in fp32, rounded once: inplace_variant).  The fused LayerNorm
is ftcf_layernorm's arithmetic: with balanced +-1 rows and eps = 0 it is exactly x * gamma + beta."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import kernel_inputs as ki

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

# Half ulps at max(|ref|, S / 128) of a GEMV result against half(float64 product of the same half inputs), as in
# test_gpu_burst_gemm.py (the CPU restatement orc.gemm measured 0..1 ulp there; the kernel gets one more).
# Worst measured on MI355X over every case below: LN + GEMV 1.00 ulp (oracle 1.00 ulp); the residual GEMV reached 0.24 of the
# error its test allows.
ORACLE_ULPS = 1
KERNEL_ULPS = ORACLE_ULPS + 1
LDS = 64 * 1024  # dynamic LDS a launch may ask for without raising the kernel's limit
XPAD = 8

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


def sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


dev16 = ki.dev16


def devh(x):
    return dev16(ki.bits(ki.half(x)))


def host16(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint16)


def ptr(t):
    return 0 if t is None else t.data_ptr()


PAD = 2  # sentinel rows behind the m rows of every output


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm -> GEMV (QKV and / or FFN1 + bias + gelu)
# ---------------------------------------------------------------------------------------------------------------------
def ln_gemv(x, g0, b0, W0, g1, b1, W1, bias1, out0, out1, K, m, int8, wpg, eps):
    a = capi.LnGemvArgs(x=ptr(x), gamma0=ptr(g0), beta0=ptr(b0), gamma1=ptr(g1), beta1=ptr(b1), W0=ptr(W0 and W0.W), W1=ptr(W1 and W1.W),
                        scale0=ptr(W0 and W0.scale), scale1=ptr(W1 and W1.scale), bias1=ptr(bias1), out0=ptr(out0), out1=ptr(out1), K=K,
                        N0=W0.n if W0 else 0, N1=W1.n if W1 else 0, eps=eps)
    return L().ftcf_ln_gemv(C.byref(a), m, int(int8), wpg, sp())


N0, N1 = 80, 112  # 5 and 7 column groups: the block form's last workgroup of each segment has idle waves


@pytest.mark.parametrize("int8", [True, False], ids=["int8", "fp16"])
@pytest.mark.parametrize("K", [384, 2048, 5120])
def test_ln_gemv_is_bit_exact_through_the_layernorm(int8, K):
    """balanced +-1 rows, integer gamma / beta, eps 0: QKV is the integer result bit for bit in the block form (wpg 0) and the
    group form (wpg 1, 2, 4), for segment 0 alone, segment 1 alone and both; FFN1's gelu output (not exact) against the oracle on
    the exact pre-activation."""
    rng = np.random.RandomState(K + int8)
    W0, W1 = ki.Weights(capi, rng, K, N0, int8, True), ki.Weights(capi, rng, K, N1, int8, True)
    (g0, b0), (g1, b1) = ki.small_gamma_beta(rng, K), ki.small_gamma_beta(rng, K)
    G0, B0, G1, B1 = devh(g0), devh(b0), devh(g1), devh(b1)
    bi = rng.randint(-8, 9, size=N1)
    Bias = devh(bi * W1.unit)
    for m in (1, 2, 3, 4):
        x = ki.balanced_rows(rng, m, K)
        X = devh(x)
        a0, a1 = x * g0 + b0, x * g1 + b1  # LN(x), exactly
        acc0 = np.rint(a0.astype(np.float32) @ W0.qf).astype(np.int64)
        ki.assert_units(acc0, "QKV")
        want0 = ki.bits(ki.half(acc0 * W0.unit))
        want1 = W1.oracle(a1.astype(np.float32), (bi * W1.unit).astype(np.float32), 1)
        for wpg in (0, 1, 2, 4):
            for segs in ((1, 0), (0, 1), (1, 1)):
                s0, s1 = ki.sentinel(rng, (m + PAD) * N0).reshape(-1, N0), ki.sentinel(rng, (m + PAD) * N1).reshape(-1, N1)
                O0, O1 = dev16(s0), dev16(s1)
                capi.check(ln_gemv(X, G0 if segs[0] else None, B0 if segs[0] else None, W0 if segs[0] else None, G1 if segs[1] else None,
                                   B1 if segs[1] else None, W1 if segs[1] else None, Bias if segs[1] else None, O0, O1, K, m, int8, wpg, 0.0))
                o0, o1 = host16(O0), host16(O1)
                tag = ("int8" if int8 else "fp16", K, m, wpg, segs)
                assert np.array_equal(o0[m:], s0[m:]) and np.array_equal(o1[m:], s1[m:]), (tag, "rows behind m written")
                if segs[0]:
                    bad = np.argwhere(o0[:m] != want0)
                    assert bad.size == 0, (tag, "QKV not bit exact at (row, col)", bad[:8].tolist())
                else:
                    assert np.array_equal(o0, s0), (tag, "absent segment 0 written")
                if segs[1]:
                    torch.testing.assert_close(torch.from_numpy(o1[:m].view(np.float16).astype(np.float32)), torch.from_numpy(want1), rtol=1e-3,
                                               atol=2e-3, msg=lambda t: f"{tag}: {t}")
                else:
                    assert np.array_equal(o1, s1), (tag, "absent segment 1 written")


@pytest.mark.parametrize("int8", [True, False], ids=["int8", "fp16"])
@pytest.mark.parametrize("K", [384, 2048, 5120])
def test_ln_gemv_gaussian_inputs_within_ulps_of_float64(int8, K):
    """weights N(0, 0.02) through the real quantiser, x N(0, 1) (scaled and shifted so that the LayerNorm has work to do): the
    reference is ftcf_layernorm of x followed by a float64 product."""
    rng = np.random.RandomState(7 * K + int8)
    W0, W1 = ki.Weights(capi, rng, K, N0, int8, False), ki.Weights(capi, rng, K, N1, int8, False)
    g = [ki.half(1 + 0.1 * rng.randn(K)) for _ in range(2)]
    b = [ki.half(0.1 * rng.randn(K)) for _ in range(2)]
    G, B = [devh(a) for a in g], [devh(a) for a in b]
    bias = ki.half(rng.randn(N1))
    Bias = devh(bias)
    worst = 0.0
    for m in (1, 2, 3, 4):
        X = devh(0.3 + 1.7 * rng.randn(m, K))
        nrm = []
        for i in range(2):
            o = torch.empty((m, K), dtype=torch.int16, device="cuda")
            capi.check(L().ftcf_layernorm(capi.vp(X), capi.vp(G[i]), capi.vp(B[i]), capi.vp(o), m, K, C.c_float(1e-5), 1, sp()))
            nrm.append(host16(o).view(np.float16))
        A64 = nrm[0].astype(np.float64)
        ref0 = ki.half(A64 @ W0.w64())
        mag = (np.abs(A64) @ np.abs(W0.w64())) / 128
        e_o = float(ki.ulps(W0.oracle(nrm[0].astype(np.float32), None, 0), ref0, mag).max())
        assert e_o <= ORACLE_ULPS, ("oracle vs float64", K, m, e_o)
        want1 = W1.oracle(nrm[1].astype(np.float32), bias.astype(np.float32), 1)
        for wpg in (0, 1, 2, 4):
            O0, O1 = dev16(ki.sentinel(rng, m * N0)), dev16(ki.sentinel(rng, m * N1))
            capi.check(ln_gemv(X, G[0], B[0], W0, G[1], B[1], W1, Bias, O0, O1, K, m, int8, wpg, 1e-5))
            e_k = float(ki.ulps(host16(O0).view(np.float16).reshape(m, N0), ref0, mag).max())
            worst = max(worst, e_k)
            assert e_k <= KERNEL_ULPS, ("QKV vs float64", "int8" if int8 else "fp16", K, m, wpg, e_k)
            torch.testing.assert_close(torch.from_numpy(host16(O1).view(np.float16).astype(np.float32).reshape(m, N1)),
                                       torch.from_numpy(want1), rtol=1e-3, atol=2e-3)
    print(f"[LN + GEMV K {K}: worst {worst:.2f} ulp] ", end="")


def test_ln_gemv_refuses_bad_shapes():
    z = torch.zeros(4096, dtype=torch.int16, device="cuda")
    a = capi.LnGemvArgs(x=ptr(z), gamma0=ptr(z), beta0=ptr(z), W0=ptr(z), scale0=ptr(z), out0=ptr(z), K=384, N0=16, N1=0, eps=0.0)
    for field, bad in (("K", 400), ("N0", 24), ("out0", 0), ("N0", 0)):
        a2 = capi.LnGemvArgs.from_buffer_copy(a)
        setattr(a2, field, bad)
        assert L().ftcf_ln_gemv(C.byref(a2), 1, 1, 0, sp()) == -1, field
    assert L().ftcf_ln_gemv(C.byref(a), 5, 1, 0, sp()) == -1 and L().ftcf_ln_gemv(C.byref(a), 1, 1, 5, sp()) == -1
    big = capi.LnGemvArgs.from_buffer_copy(a)
    big.K = 16384
    assert L().ftcf_ln_gemv(C.byref(big), 4, 1, 0, sp()) == -1  # 4 rows of 16384 do not fit the LDS
    torch.cuda.synchronize()
    assert not bool(z.any())


# ---------------------------------------------------------------------------------------------------------------------
# [out-projection U FFN2] -> residual
# ---------------------------------------------------------------------------------------------------------------------
def lds_need(Q, m, kt_a, kt_b, int8):
    """the launchers' dynamic LDS (kernels_gemv.hip: launch_splitk_m after plan_splitk(.., 10), launch_chunked_m)"""
    tk = 64 if int8 else 32
    if Q == 0:
        total, nw = kt_a + kt_b, 10
        while nw > 1 and total // nw < 8:
            nw -= 1
        wa = min(max(int(kt_a / total * nw + 0.5), 1), nw - 1)
        if nw == 1:
            nw, wa = 2, 1
        maxnt = max(-(-kt_a // wa), -(-kt_b // (nw - wa)))
        return nw * m * (maxnt * tk + XPAD) * 2 + nw * m * 16 * 4
    T = -(-(kt_a + kt_b) // Q)
    return 2 * m * ((T // 2 + 2) * tk + XPAD) * 2 + 2 * 2 * m * 16 * 4


class ResidualCase:
    """two exact (or Gaussian) weight matrices whose columns share their unit, a granule workspace shared by every launch"""

    def __init__(self, rng, kt_a, kt_b, N, int8, exact):
        tk = 64 if int8 else 32
        self.int8, self.exact, self.N, self.kt = int8, exact, N, (kt_a, kt_b)
        self.Wa = ki.Weights(capi, rng, kt_a * tk, N, int8, exact)
        self.Wb = ki.Weights(capi, rng, kt_b * tk, N, int8, exact, e=self.Wa.e if exact else None)
        self.gran_bytes = int(L().ftcf_residual_gemv_workspace_bytes(N, 4, 8))
        self.gran = torch.zeros(self.gran_bytes, dtype=torch.uint8, device="cuda")
        self.d_step = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.launches = 0

    def run(self, rng, m, Q, tp, inplace, worst=None):
        Wa, Wb, N = self.Wa, self.Wb, self.N
        tag = ("int8" if self.int8 else "fp16", self.kt, N, "m", m, "Q", Q, "tp", tp, "inplace", inplace)
        if self.exact:
            xa, xb = ki.exact_acts(rng, m, Wa.k), ki.exact_acts(rng, m, Wb.k)
            attn = np.rint(xa.astype(np.float32) @ Wa.qf).astype(np.int64)
            ffn = np.rint(xb.astype(np.float32) @ Wb.qf).astype(np.int64)
            b, xin = rng.randint(-16, 17, size=N), rng.randint(-16, 17, size=(m + PAD, N))
            for v in (attn, ffn, ffn + attn, ffn + attn + b, ffn + attn + b + xin[:m]):  # every value rounded to half, kernel order
                ki.assert_units(v, tag)
            want = ki.bits(ki.half((ffn + attn + b + xin[:m]) * Wa.unit))
            bias, x_in = b * Wa.unit, xin * tp * Wa.unit
        else:
            xa, xb = ki.half(rng.randn(m, Wa.k)), ki.half(rng.randn(m, Wb.k))
            bias, x_in = ki.half(0.1 * rng.randn(N)), ki.half(rng.randn(m + PAD, N))
        XA, XB, Bi = devh(xa), devh(xb), devh(bias)
        xbits = ki.bits(ki.half(x_in))
        X = dev16(xbits)  # in place: out = x_in, as the engine runs it
        a = capi.ResidualGemvArgs(x_a=ptr(XA), x_b=ptr(XB), W_a=ptr(Wa.W), W_b=ptr(Wb.W), scale_a=ptr(Wa.scale), scale_b=ptr(Wb.scale),
                                  bias=ptr(Bi), x_in=ptr(X), out=ptr(X), N=N, K_a=Wa.k, K_b=Wb.k, tp=tp, inplace_variant=inplace)
        # consecutive launches on one granule workspace: (step, salt) advances; the step alternately from the device and the host
        i = self.launches
        self.launches += 1
        step, salt = 5 + i // 3, (i % 3) * 7
        on_device = i % 2 == 0
        if on_device:
            self.d_step.fill_(step)
        code = L().ftcf_residual_gemv(C.byref(a), m, int(self.int8), Q, capi.vp(self.gran), C.c_size_t(self.gran_bytes),
                                      capi.vp(self.d_step if on_device else None), 0 if on_device else step, salt, sp())
        if lds_need(Q, m, *self.kt, self.int8) > LDS:
            assert code == -1 and b"LDS" in L().ftcf_last_error(), (tag, "a shape over the LDS limit must be refused", code)
            return False
        capi.check(code)
        got = host16(X)
        assert np.array_equal(got[m:], xbits[m:]), (tag, "rows behind m written")
        if self.exact:
            bad = np.argwhere(got[:m] != want)
            assert bad.size == 0, (tag, "not bit exact at (row, col)", bad[:8].tolist())
            return True
        # Gaussian: the residual of the two float64 GEMV results rounded to half.  The kernel's attn / ffn may each be KERNEL_ULPS off
        # (at their own magnitude, floored as usual); the chain of half additions (three roundings, or one) then moves the sum by at
        # most that plus one ulp of the largest intermediate per rounding that lands on the other side.
        A64, B64 = xa.astype(np.float64), xb.astype(np.float64)
        ra, rb = ki.half(A64 @ Wa.w64()), ki.half(B64 @ Wb.w64())
        ma, mb = (np.abs(A64) @ np.abs(Wa.w64())) / 128, (np.abs(B64) @ np.abs(Wb.w64())) / 128
        ref = orc.add_bias_attn_ffn_residual(rb.astype(np.float32), ra.astype(np.float32), x_in[:m].astype(np.float32),
                                             bias.astype(np.float32), tp=tp, inplace_variant=bool(inplace), fp16=True)
        sp16 = lambda v: np.spacing(np.maximum(v, 2.0 ** -14).astype(np.float16)).astype(np.float64)
        big = np.abs(ra.astype(np.float64)) + np.abs(rb.astype(np.float64)) + np.abs(bias.astype(np.float64)) + np.abs(x_in[:m].astype(np.float64))
        allowed = KERNEL_ULPS * (sp16(np.maximum(np.abs(ra), ma)) + sp16(np.maximum(np.abs(rb), mb))) + (1 if inplace else 3) * sp16(big)
        err = np.abs(got[:m].view(np.float16).astype(np.float64) - ref)
        frac = float((err / allowed).max())
        if worst is not None:
            worst[0] = max(worst[0], frac)
        assert frac <= 1.0, (tag, "error / allowed", frac)
        return True


# (KT_a, KT_b, N) in tiles: (7, 33) puts the a / b boundary inside a wave's range for every Q (chunks of 40, 20, 10, 5 tiles); (20, 20) on a
# chunk edge for Q 2 / 4 / 8; (5, 4): nine tiles, Q 8 leaves empty chunks and no wave has a full batch of eight tiles; (24, 40): one to
# four full batches per wave (WaveStream's ping-pong loop and its clamped reload)
_SHAPES = [(7, 33, 80), (20, 20, 48), (5, 4, 32), (24, 40, 112)]


@pytest.mark.parametrize("int8", [True, False], ids=["int8", "fp16"])
@pytest.mark.parametrize("kt_a,kt_b,N", _SHAPES)
def test_residual_gemv_is_bit_exact_on_exact_inputs(int8, kt_a, kt_b, N):
    rng = np.random.RandomState(kt_a * 100 + kt_b + int8)
    case = ResidualCase(rng, kt_a, kt_b, N, int8, True)
    ran = 0
    for Q in (0, 1, 2, 4, 8):
        for m in (1, 2, 3, 4):
            for tp, inplace in ((1, 0), (2, 1)) if (m + Q) % 2 else ((1, 1), (2, 0)):
                ran += case.run(rng, m, Q, tp, inplace)
    assert ran == 40  # (every one of these shapes fits the LDS)


@pytest.mark.parametrize("int8", [True, False], ids=["int8", "fp16"])
def test_residual_gemv_at_codefuse_13b_shape(int8):
    """hl = 5120, il = 20480, N = 5120 on exact inputs; the engine runs Q = 4 there.  (Q, m) whose x slices exceed 64 KiB of LDS are
    refused by the entry point."""
    tk = 64 if int8 else 32
    rng = np.random.RandomState(13 + int8)
    case = ResidualCase(rng, 5120 // tk, 20480 // tk, 5120, int8, True)
    ran = {}
    for Q in (0, 1, 2, 4, 8):
        for m in (1, 2, 3, 4):
            ran[(Q, m)] = case.run(rng, m, Q, 1 + (m % 2), (m + Q) % 2)
    assert all(ran[(Q, m)] for Q in (4, 8) for m in (1, 2, 3, 4)) and ran[(0, 1)] and ran[(1, 1)] and ran[(2, 1)], ran


@pytest.mark.parametrize("int8", [True, False], ids=["int8", "fp16"])
def test_residual_gemv_gaussian_inputs(int8):
    rng = np.random.RandomState(41 + int8)
    worst = [0.0]
    for (kt_a, kt_b, N) in ((7, 33, 80), (24, 40, 112)):
        case = ResidualCase(rng, kt_a, kt_b, N, int8, False)
        for Q in (0, 1, 2, 4, 8):
            for m in (1, 2, 3, 4):
                assert case.run(rng, m, Q, 1 + (m % 2), (m + Q) % 2, worst)
    print(f"[residual GEMV: worst error / allowed {worst[0]:.2f}] ", end="")


def test_residual_gemv_refuses_bad_arguments():
    rng = np.random.RandomState(2)
    case = ResidualCase(rng, 7, 33, 80, True, True)
    z = torch.zeros(4 * 2112, dtype=torch.int16, device="cuda")
    a = capi.ResidualGemvArgs(x_a=ptr(z), x_b=ptr(z), W_a=ptr(case.Wa.W), W_b=ptr(case.Wb.W), scale_a=ptr(case.Wa.scale),
                              scale_b=ptr(case.Wb.scale), bias=ptr(z), x_in=ptr(z), out=ptr(z), N=80, K_a=448, K_b=2112, tp=1, inplace_variant=0)
    call = lambda a_, m=2, Q=2, gb=None, salt=0: L().ftcf_residual_gemv(C.byref(a_), m, 1, Q, capi.vp(case.gran),
                                                                       C.c_size_t(case.gran_bytes if gb is None else gb), None, 1, salt, sp())
    assert call(a, m=5) == -1 and call(a, Q=9) == -1 and call(a, gb=64) == -1 and call(a, salt=1024) == -1
    for field, bad in (("N", 72), ("K_a", 480), ("K_b", 0), ("tp", 0), ("bias", 0)):
        a2 = capi.ResidualGemvArgs.from_buffer_copy(a)
        setattr(a2, field, bad)
        assert call(a2) == -1, field
    capi.check(call(a))  # all zeros in, all zeros out
    torch.cuda.synchronize()
    assert not bool(z.any())
