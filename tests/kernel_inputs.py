"""Inputs and error measures shared by the kernel-level tests of the forms the engine launches (test_gpu_burst_gemm.py,
test_gpu_fused_ln.py, test_gpu_stage_gemv.py, test_gpu_tiled_gemm.py).  Plain numpy, but for dev16 and Weights, which put their data on the GPU.

EXACT inputs: activations in {-1, 0, 1} (dense), weights small integers q in {-3..3} times a power of two that varies by column
(the int8 scale, or folded into the fp16 weight), biases and residual inputs integer multiples of the column's unit.  Every
product and every partial sum is then an integer multiple of the column's unit far below 2^24 of them: fp32 accumulation (the
MFMA accumulators of k_gemm_smallm_burst / consume_tile, the fp32 adds of the reducers, v_dot2 of the LM head) is exact in ANY
order, and as long as the value a kernel rounds to half is at most 2048 units, so is the half.  The kernel's output must equal
the integer result bit for bit: any mismatch is a dropped, doubled or misplaced term, never rounding.  assert_units() is the
precondition, checked in integer arithmetic by each test."""
import ctypes as C

import numpy as np

HALF_EXACT_UNITS = 2048  # integers up to 2^11 are binary16 values


def sentinel(rng, n):
    """n random fp16 bit patterns, all finite (bit 10 clear: the exponent is never all ones), as uint16."""
    return (rng.randint(0, 1 << 16, size=n).astype(np.uint16) & np.uint16(0xFBFF))


def half(x):
    return np.asarray(x, dtype=np.float64).astype(np.float16)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint16)


def ulps(got, ref, mag):
    """|got - ref| (ref already rounded to half) in half-precision ulps at max(|ref|, mag): mag = S / 128 with S = sum |a||w| keeps
    an output that cancels to near zero from being judged at a tiny ulp (one ulp there is still 2^7 fp32 ulps of S)."""
    m = np.maximum(np.maximum(np.abs(ref.astype(np.float64)), mag), 2.0 ** -14).astype(np.float16)
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(m).astype(np.float64)


def assert_units(v, what=""):
    """v: int64 values in units of their column -- everything a kernel rounds to half."""
    worst = int(np.abs(v).max()) if np.size(v) else 0
    assert worst <= HALF_EXACT_UNITS, (what, "exact-input precondition: |value| in units", worst)


def exact_acts(rng, m, k):
    return rng.randint(-1, 2, size=(m, k)).astype(np.int64)


def fast_rng(rng):
    """a numpy Generator seeded from rng: draws the large matrices several times faster than RandomState (int8 and float32
    directly)"""
    return np.random.Generator(np.random.PCG64(int(rng.randint(1 << 31))))


def exact_weights(rng, k, n):
    """q int8 [k, n] in {-3..3}, e int [n]: the column's unit is 2^e[col] (both exponents inside every 16-column group)."""
    q = fast_rng(rng).integers(-3, 4, size=(k, n), dtype=np.int8)
    e = np.where(rng.randint(0, 2, size=n) == 1, -3, -5)
    e[0::16], e[1::16] = -3, -5
    return q, e


def unit(e):
    return np.ldexp(1.0, e)  # float64 [n]


def balanced_rows(rng, m, n):
    """rows of +-1 with equal counts, shuffled: mean exactly 0, E[x^2] exactly 1 (with eps = 0 the LayerNorm's rstd is 1.0)."""
    assert n % 2 == 0
    x = np.empty((m, n), dtype=np.int64)
    for r in range(m):
        x[r] = rng.permutation(np.repeat([1, -1], n // 2))
    return x


def small_gamma_beta(rng, n):
    """gamma in {-1, 1, 2}, beta in {-1, 0, 1}: LN(x) of a balanced row is exactly x * gamma + beta, an integer in -3..3"""
    return rng.choice([-1, 1, 2], size=n).astype(np.int64), rng.randint(-1, 2, size=n).astype(np.int64)


def tile_int8(capi, q):
    """row-major int8 [k, n] -> the engine's tile layout (host)"""
    q = np.ascontiguousarray(q, dtype=np.int8)
    out = np.empty_like(q)
    capi.check(capi.lib().ftcf_int8_rowmajor_to_tiled(capi.vp(q), C.c_size_t(q.shape[0]), C.c_size_t(q.shape[1]), capi.vp(out)))
    return out


def dev16(a):
    """uint16 bit patterns -> device (an int16 tensor)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).cuda()


class Weights:
    """one [k, n] matrix: the engine image on the device and what the references need"""

    def __init__(self, capi, rng, k, n, int8, exact, e=None):
        import torch
        from oracle import oracle as orc
        self.k, self.n, self.int8, self.exact = k, n, int8, exact
        self.scale = None
        if exact:
            self.q, e_own = exact_weights(rng, k, n)
            self.e = e_own if e is None else e  # (e: the exponents of another matrix whose columns share their unit with this one's)
            self.unit = unit(self.e)
            self.qf = self.q.astype(np.float32)  # (sums of |a q| <= 3 k < 2^24: an fp32 product of these is exact)
            w16 = (self.qf * self.unit.astype(np.float32)).astype(np.float16)  # (exact: |q| <= 3 times a power of two)
            self.s32 = self.unit.astype(np.float32)
        else:
            w16 = (np.float32(0.02) * fast_rng(rng).standard_normal((k, n), dtype=np.float32)).astype(np.float16)
        if int8:
            if exact:
                self.W = torch.from_numpy(tile_int8(capi, self.q)).cuda()
                self.scale = dev16(bits(half(self.unit)))
            else:
                from fastertransformer4codefuse_amd.gptneox_op import symmetric_quantize_last_axis_of_batched_matrix_int8 as qf
                qt, s = qf(torch.from_numpy(w16.astype(np.float32)).half().contiguous())  # the real quantiser
                self.W, self.scale = qt.cuda(), s.cuda()
                self.q, self.s32 = orc.symmetric_quantize_int8(w16.astype(np.float32), True)
                assert np.array_equal(self.s32, s.float().numpy())
                w16 = (self.q.astype(np.float32) * self.s32).astype(np.float16)  # W = half(q * scale), the product in fp32
        else:
            rm = dev16(bits(w16))
            self.W = torch.empty((k, n), dtype=torch.int16, device="cuda")
            capi.check(capi.lib().ftcf_fp16_rowmajor_to_tiled(capi.vp(rm), C.c_size_t(k), C.c_size_t(n), capi.vp(self.W), None))
            torch.cuda.synchronize()
        self.w32 = w16.astype(np.float32)
        self._w64 = None

    def w64(self):
        if self._w64 is None:
            self._w64 = self.w32.astype(np.float64)
        return self._w64

    def oracle(self, A, bias, act):
        from oracle import oracle as orc
        if self.int8:
            return orc.gemm(A, q=self.q, scale=self.s32, bias=bias, act=act, fp16=True)
        return orc.gemm(A, W=self.w32, bias=bias, act=act, fp16=True)


class GemmProblem:
    """one GEMM C[m, n] = epilogue(A[m, k] x W) on new activations: device operands, an output of `rows` >= m rows filled with a
    sentinel, and its reference.  epi 0: none, 1: bias, 2: bias + gelu."""

    def __init__(self, rng, W, m, epi, rows):
        self.W, self.m, self.epi = W, m, epi
        k, n = W.k, W.n
        self.expect = None
        bias = None
        if W.exact:
            a = exact_acts(rng, m, k)
            acc = np.rint(a.astype(np.float32) @ W.qf).astype(np.int64)  # exact: every partial sum is an integer < 2^24
            assert_units(acc, "GEMM result")
            self.A = a.astype(np.float32)
            if epi:
                b = rng.randint(-64, 65, size=n).astype(np.int64)
                assert_units(acc + b, "GEMM result + bias")
                bias = (b * W.unit).astype(np.float32)
                acc = acc + b
            if epi < 2:
                self.expect = bits(half(acc * W.unit))
        else:
            self.A = half(rng.randn(m, k)).astype(np.float32)
            if epi:
                bias = half(rng.randn(n)).astype(np.float32)
        self.bias = bias
        self.dA = dev16(bits(half(self.A)))
        self.dB = None if bias is None else dev16(bits(half(bias)))
        self.sent = sentinel(rng, rows * n).reshape(rows, n)
        self.dC = dev16(self.sent)

    def tag(self):
        return ("int8" if self.W.int8 else "fp16", self.m, self.W.n, self.W.k, self.epi)

    def got(self):
        import torch
        torch.cuda.synchronize()
        out = self.dC.cpu().numpy().view(np.uint16)
        assert np.array_equal(out[self.m:], self.sent[self.m:]), ("rows >= m written", self.m, self.W.n, self.W.k)
        return out[:self.m]

    def check(self, oracle_ulps, kernel_ulps, worst=None, tag=None):
        """-> the output bits.  exact: bit for bit; Gaussian without epilogue: ulps against float64 (and the oracle against it);
        bias / gelu epilogues: the oracle at the tolerances test_gpu_kernels.py uses for it."""
        import torch
        out = self.got()
        W, tag = self.W, tag or self.tag()
        if self.expect is not None:
            bad = np.argwhere(out != self.expect)
            assert bad.size == 0, (tag, "not bit exact at (row, col)", bad[:8].tolist(),
                                   out.view(np.float16)[tuple(bad[0])], self.expect.view(np.float16)[tuple(bad[0])])
        elif self.epi:
            ref = W.oracle(self.A, self.bias, 1 if self.epi == 2 else 0)
            torch.testing.assert_close(torch.from_numpy(out.view(np.float16).astype(np.float32)), torch.from_numpy(ref), rtol=1e-3,
                                       atol=2e-3, msg=lambda t: f"{tag}: {t}")
        else:
            A64 = self.A.astype(np.float64)
            ref = half(A64 @ W.w64())
            mag = (np.abs(A64) @ np.abs(W.w64())) / 128
            e_o = float(ulps(W.oracle(self.A, None, 0), ref, mag).max())
            e_k = float(ulps(out.view(np.float16), ref, mag).max())
            print(f"[{tag}: oracle {e_o:.2f} ulp, kernel {e_k:.2f} ulp] ", end="")
            if worst is not None:
                worst[0], worst[1] = max(worst[0], e_o), max(worst[1], e_k)
            assert e_o <= oracle_ulps, (tag, "oracle vs float64", e_o)
            assert e_k <= kernel_ulps, (tag, "kernel vs float64", e_k)
        return out
