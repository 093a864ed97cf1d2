"""-m gpu: the fused residual / LayerNorm kernels the batched paths launch in every layer, and the LM head in the forms the
engine runs, at kernel level (include/ftcf.h ftcf_residual_dual_layernorm, ftcf_add_bias_residual, ftcf_lm_head_layernorm, and
ftcf_lm_head for more than 4 rows) against the oracle's rounding points, ftcf_layernorm bit for bit, and exact integer inputs
(tests/kernel_inputs.py: rows of +-1 in equal counts with eps = 0 have mean 0 and rstd 1.0 exactly, so LN(x) = x * gamma + beta
with small-integer gamma / beta, and the LM head's fp32 sums of integers are exact in any order)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import kernel_inputs as ki

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

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


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).cuda()


def devh(x):
    """values -> half -> device"""
    return dev16(ki.bits(ki.half(x)))


def host16(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint16)


def f32(h_bits):
    return h_bits.view(np.float16).astype(np.float32)


PAD = 2  # sentinel rows behind the m rows of every buffer a kernel writes


def dual_ln(x, ffn, attn, bias, tp, inplace, g1, b1, g2, b2, o1, o2, m, n, eps, bias_mul=1, sum_mul=1):
    return L().ftcf_residual_dual_layernorm(capi.vp(x), capi.vp(ffn), capi.vp(attn), capi.vp(bias), tp, inplace, capi.vp(g1), capi.vp(b1),
                                            capi.vp(g2), capi.vp(b2), capi.vp(o1), capi.vp(o2), m, n, C.c_float(eps), bias_mul, sum_mul,
                                            sp())


def layernorm(x, g, b, m, n, eps):
    out = torch.empty((m, n), dtype=torch.int16, device="cuda")
    capi.check(L().ftcf_layernorm(capi.vp(x), capi.vp(g), capi.vp(b), capi.vp(out), m, n, C.c_float(eps), 1, sp()))
    return host16(out)


# (residual, tp, inplace_variant, bias_mul, sum_mul)
_DLN_CONFIGS = [(0, 1, 0, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 1, 1), (1, 2, 0, 2, 1), (1, 2, 1, 1, 2), (1, 8, 1, 8, 1), (1, 8, 0, 1, 8),
                (1, 2, 1, 2, 2), (1, 1, 0, 8, 2)]


@pytest.mark.parametrize("n", [8, 384, 2048, 2056, 5120, 8192])
def test_residual_dual_layernorm_matches_its_unfused_parts(n):
    """the updated x: bit-equal to the oracle's residual on inputs pre-scaled as the kernel scales them; out1 / out2: bit-equal to
    ftcf_layernorm of the updated x (the kernel's documented claim) and within the existing LayerNorm test's bounds of
    orc.layernorm; g1 == NULL: the residual only; rows behind m untouched."""
    rng = np.random.RandomState(n)
    g = [ki.half(1 + 0.1 * rng.randn(n)) for _ in range(2)]
    b = [ki.half(0.1 * rng.randn(n)) for _ in range(2)]
    G, Bt = [devh(a) for a in g], [devh(a) for a in b]
    for m in (1, 7, 33):
        for (resid, tp, inplace, bias_mul, sum_mul) in _DLN_CONFIGS:
            for with_ln in (True, False) if resid else (True,):
                x = ki.half(rng.randn(m + PAD, n))
                ffn, attn, bias = ki.half(0.5 * rng.randn(m, n)), ki.half(0.25 * rng.randn(m, n)), ki.half(0.1 * rng.randn(n))
                X = devh(x)
                s1, s2 = ki.sentinel(rng, (m + PAD) * n).reshape(-1, n), ki.sentinel(rng, (m + PAD) * n).reshape(-1, n)
                O1, O2 = dev16(s1), dev16(s2)
                F, A, Bi = (devh(ffn), devh(attn), devh(bias)) if resid else (None, None, None)
                gp = (G[0], Bt[0], G[1], Bt[1]) if with_ln else (None, None, None, None)
                capi.check(dual_ln(X, F, A, Bi, tp, inplace, *gp, O1, O2, m, n, 1e-5, bias_mul, sum_mul))
                tag = (m, n, resid, tp, inplace, bias_mul, sum_mul, with_ln)
                xs = x.astype(np.float32)
                if resid:
                    scaled = lambda a, k: ki.half(a.astype(np.float32) * np.float32(k)).astype(np.float32)  # half(float * mul)
                    want = orc.add_bias_attn_ffn_residual(scaled(ffn, sum_mul), scaled(attn, sum_mul), xs[:m], scaled(bias, bias_mul), tp=tp,
                                                          inplace_variant=bool(inplace), fp16=True)
                else:
                    want = xs[:m]
                xg = host16(X)
                assert np.array_equal(xg[m:], ki.bits(x)[m:]), (tag, "x rows behind m written")
                assert np.array_equal(f32(xg[:m]), want), (tag, "updated x")
                o1, o2 = host16(O1), host16(O2)
                if not with_ln:
                    assert np.array_equal(o1, s1) and np.array_equal(o2, s2), (tag, "g1 == NULL must leave out1 / out2 alone")
                    continue
                assert np.array_equal(o1[m:], s1[m:]) and np.array_equal(o2[m:], s2[m:]), (tag, "out rows behind m written")
                for i, o in enumerate((o1, o2)):
                    assert np.array_equal(o[:m], layernorm(X, G[i], Bt[i], m, n, 1e-5)), (tag, "out%d != ftcf_layernorm(x)" % (i + 1))
                    ref = orc.layernorm(want, g[i].astype(np.float32), b[i].astype(np.float32), fp16=True)
                    got = f32(o[:m])
                    assert np.mean(got != ref) < 0.02, tag
                    np.testing.assert_allclose(got, ref, rtol=4e-3, atol=4e-3)


@pytest.mark.parametrize("n", [8, 384, 2056, 8192])
@pytest.mark.parametrize("tp,inplace,bias_mul,sum_mul", [(1, 0, 1, 1), (1, 1, 1, 1), (2, 0, 2, 1), (2, 1, 1, 2), (8, 1, 8, 1)])
def test_residual_dual_layernorm_exact_inputs(n, tp, inplace, bias_mul, sum_mul):
    """integer inputs chosen so that the updated row is +-1 in equal counts: with eps = 0 both outputs are exactly x * gamma + beta.
    A LayerNorm that skips columns, or a residual that drops a term, cannot hide behind rounding."""
    rng = np.random.RandomState(n + tp + inplace)
    for m in (1, 7, 33):
        t = ki.balanced_rows(rng, m, n)
        ffn, attn, bias = rng.randint(-3, 4, size=(m, n)), rng.randint(-3, 4, size=(m, n)), rng.randint(-2, 3, size=n)
        x = (t - sum_mul * (ffn + attn) - bias_mul * bias) * tp
        ki.assert_units(x)
        (g1, b1), (g2, b2) = ki.small_gamma_beta(rng, n), ki.small_gamma_beta(rng, n)
        X = devh(x)
        O1, O2 = dev16(ki.sentinel(rng, m * n)), dev16(ki.sentinel(rng, m * n))
        capi.check(dual_ln(X, devh(ffn), devh(attn), devh(bias), tp, inplace, devh(g1), devh(b1), devh(g2), devh(b2), O1, O2, m, n, 0.0,
                           bias_mul, sum_mul))
        assert np.array_equal(host16(X), ki.bits(ki.half(t))), (m, "updated x")
        assert np.array_equal(host16(O1).reshape(m, n), ki.bits(ki.half(t * g1 + b1))), (m, "out1")
        assert np.array_equal(host16(O2).reshape(m, n), ki.bits(ki.half(t * g2 + b2))), (m, "out2")
        # without the residual: the same row straight through both LayerNorms
        O1, O2 = dev16(ki.sentinel(rng, m * n)), dev16(ki.sentinel(rng, m * n))
        capi.check(dual_ln(X, None, None, None, 1, 0, devh(g1), devh(b1), devh(g2), devh(b2), O1, O2, m, n, 0.0))
        assert np.array_equal(host16(X), ki.bits(ki.half(t)))
        assert np.array_equal(host16(O1).reshape(m, n), ki.bits(ki.half(t * g1 + b1)))
        assert np.array_equal(host16(O2).reshape(m, n), ki.bits(ki.half(t * g2 + b2)))


@pytest.mark.parametrize("n", [12, 8200, 0])
def test_residual_dual_layernorm_refuses_row_lengths_it_cannot_do(n):
    z = torch.zeros(4 * 8200, dtype=torch.int16, device="cuda")
    assert dual_ln(z, None, None, None, 1, 0, z, z, z, z, z, z, 2, n, 1e-5) == -1
    assert b"LayerNorm" in L().ftcf_last_error()
    torch.cuda.synchronize()
    assert not bool(z.any())


@pytest.mark.parametrize("m,n", [(1, 8), (7, 384), (33, 5120), (7, 2056), (3, 7)])
def test_add_bias_residual_rounds_once(m, n):
    """out = half((float(bias) + float(a)) + float(b)); also with out aliasing b, as the engine calls it, and without a bias"""
    rng = np.random.RandomState(m * n)
    a, b, bias = ki.half(rng.randn(m, n)), ki.half(rng.randn(m + PAD, n)), ki.half(rng.randn(n))
    for with_bias in (True, False):
        bv = bias.astype(np.float32) if with_bias else np.zeros(n, np.float32)
        want = ki.bits(((bv[None] + a.astype(np.float32)) + b[:m].astype(np.float32)).astype(np.float16))
        Bi = devh(bias) if with_bias else None
        sent = ki.sentinel(rng, (m + PAD) * n).reshape(-1, n)
        out, A, Bd = dev16(sent), devh(a), devh(b)
        capi.check(L().ftcf_add_bias_residual(capi.vp(out), capi.vp(A), capi.vp(Bd), capi.vp(Bi), m, n, sp()))
        got = host16(out)
        assert np.array_equal(got[:m], want) and np.array_equal(got[m:], sent[m:])
        capi.check(L().ftcf_add_bias_residual(capi.vp(Bd), capi.vp(A), capi.vp(Bd), capi.vp(Bi), m, n, sp()))  # in place over b
        got = host16(Bd)
        assert np.array_equal(got[:m], want) and np.array_equal(got[m:], ki.bits(b)[m:])


# ---------------------------------------------------------------------------------------------------------------------
# LM head
# ---------------------------------------------------------------------------------------------------------------------
def _logit_buffer(rng, rows, ldc):
    s = rng.randn(rows, ldc).astype(np.float32)
    return s, torch.from_numpy(s.copy()).cuda()


def _check_logits(out, sent, want, m, n, tag, exact):
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[m:], sent[m:]) and np.array_equal(got[:, n:], sent[:, n:]), (tag, "wrote outside [m, n]")
    if exact:
        bad = np.argwhere(got[:m, :n] != want)
        assert bad.size == 0, (tag, "logits not exact at (row, col)", bad[:8].tolist())
    else:
        np.testing.assert_allclose(got[:m, :n], want, rtol=1e-4, atol=1e-3, err_msg=str(tag))


@pytest.mark.parametrize("V", [2000, 100864])
def test_lm_head_with_fused_layernorm(V):
    """the <= 4-row form the token loop runs: final LayerNorm fused in front; V 100864 makes the 2048-workgroup grid cap loop;
    ldc > n; d_stop set leaves the sentinel."""
    H = 512
    rng = np.random.RandomState(V)
    ldc = V + 24
    # exact: balanced +-1 rows, integer gamma / beta / weights, eps 0
    Wi = ki.fast_rng(rng).integers(-3, 4, size=(V, H), dtype=np.int8).astype(np.float32)
    gi, bi = ki.small_gamma_beta(rng, H)
    Wd, Gd, Bd = dev16(ki.bits((Wi * np.float32(0.125)).astype(np.float16))), devh(gi), devh(bi)
    # Gaussian
    Wg = (np.float32(0.1) * ki.fast_rng(rng).standard_normal((V, H), dtype=np.float32)).astype(np.float16)
    gg, bg = ki.half(1 + 0.1 * rng.randn(H)), ki.half(0.1 * rng.randn(H))
    Wgd, Ggd, Bgd = dev16(ki.bits(Wg)), devh(gg), devh(bg)
    Wg64 = Wg.astype(np.float64)
    stop = torch.ones(1, dtype=torch.int32, device="cuda")
    go = torch.zeros(1, dtype=torch.int32, device="cuda")
    for m in (1, 2, 3, 4):
        x = ki.balanced_rows(rng, m, H)
        want = ((x * gi + bi).astype(np.float32) @ Wi.T) * np.float32(0.125)  # (integers below 2^24: the fp32 product is exact)
        assert np.abs(want).max() * 8 < 2 ** 24
        sent, out = _logit_buffer(rng, m + 1, ldc)
        X = devh(x)
        capi.check(L().ftcf_lm_head_layernorm(capi.vp(X), capi.vp(Wd), capi.vp(Gd), capi.vp(Bd), C.c_float(0.0), capi.vp(stop), capi.vp(out),
                                              m, V, H, ldc, sp()))
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), sent), "d_stop set: nothing may be written"
        for flag in (go, None):
            sent, out = _logit_buffer(rng, m + 1, ldc)
            capi.check(L().ftcf_lm_head_layernorm(capi.vp(X), capi.vp(Wd), capi.vp(Gd), capi.vp(Bd), C.c_float(0.0), capi.vp(flag),
                                                  capi.vp(out), m, V, H, ldc, sp()))
            _check_logits(out, sent, want, m, V, ("exact", m, V), True)
        xg = ki.half(rng.randn(m, H))
        nrm = orc.layernorm(xg.astype(np.float32), gg.astype(np.float32), bg.astype(np.float32), fp16=True)
        want = (nrm.astype(np.float64) @ Wg64.T).astype(np.float32)
        sent, out = _logit_buffer(rng, m + 1, ldc)
        capi.check(L().ftcf_lm_head_layernorm(capi.vp(devh(xg)), capi.vp(Wgd), capi.vp(Ggd), capi.vp(Bgd), C.c_float(1e-5), None, capi.vp(out),
                                              m, V, H, ldc, sp()))
        _check_logits(out, sent, want, m, V, ("gaussian", m, V), False)
    # refused: more than 4 rows, ldc < n
    assert L().ftcf_lm_head_layernorm(capi.vp(Wd), capi.vp(Wd), capi.vp(Gd), capi.vp(Bd), C.c_float(0.0), None, capi.vp(out), 5, V, H, ldc, sp()) == -1
    assert L().ftcf_lm_head_layernorm(capi.vp(Wd), capi.vp(Wd), capi.vp(Gd), capi.vp(Bd), C.c_float(0.0), None, capi.vp(out), 2, V, H, V - 1, sp()) == -1


@pytest.mark.parametrize("k", [512, 384])
@pytest.mark.parametrize("n", [7, 16, 2000, 2005])
def test_lm_head_above_four_rows_is_exact_on_integer_inputs(n, k):
    """the m > 4 form behind ftcf_lm_head: k 512 runs the whole-row kernel (n >= 16), k 384 (H of the 64-wide test model) the
    fragment-order one; more than 16 rows (a second row block), n % 16 != 0, ldc > n (a tensor-parallel rank's slice)."""
    rng = np.random.RandomState(n + k)
    Wi = rng.randint(-3, 4, size=(n, k))
    Wd = devh(Wi * 0.125)
    for m in (5, 16, 17, 33):
        x = rng.randint(-3, 4, size=(m, k))
        want = (x.astype(np.float64) @ (Wi.T * 0.125)).astype(np.float32)
        for ldc in (n, n + 9):
            sent, out = _logit_buffer(rng, m + 1, ldc)
            capi.check(L().ftcf_lm_head(capi.vp(devh(x)), capi.vp(Wd), capi.vp(out), m, n, k, ldc, sp()))
            _check_logits(out, sent, want, m, n, (m, n, k, ldc), True)
