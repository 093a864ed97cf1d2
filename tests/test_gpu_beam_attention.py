"""-m gpu: beam search's decode attention at kernel level (include/ftcf.h ftcf_masked_multihead_attention_beams: k_mmha_split<DH, true>
and, for fp32, k32_mmha reading the caches through the cache indirection) against the float64 reference of
tests/attention_reference.py, past one KV split and in the looped form.

Every cache row holds values of its own, so a key read from a wrong beam's row is wrong; positions beyond the live length hold NaN
bit patterns, so a consumed speculative fetch is NaN.  Each case is also run without beams on a dense cache gathered through the
indirection here in numpy: the two forms read the same values in the same order and must agree bit for bit, which ties the beam
form to the form tests/test_gpu_kernels.py covers and makes that launch the yardstick of the float64 bounds.

Measured on MI355X (profiles/beam_attention_tests.md has every case): worst context error 1.50 ulp and worst appended-key error
1.00 ulp (dh 256, 600 keys, both forms), with and without beams alike -- the two were bit-identical in every case, so the bounds of
tests/attention_reference.py (6 / 2) hold unchanged; fp32: context 1.7e-6, appended key 2.0e-5 of the term size (bound 5e-5)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.attention_reference import (BEAM_CASES, CTX_FLOOR, CTX_ULPS, FP32_CASES, K_ULPS, PICKED_SPLITS, _nan_bits, _ulps, beam_case, beam_reference,
                                       beam_source_rows, fill_indirection, in_registers)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

capi = None
FP32_BOUND = 5e-5  # "the same arithmetic up to summation order" (tests/test_gpu_fp32.py), x the size of the terms of a (row, head)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    global capi
    from fastertransformer4codefuse_amd import capi as _c
    capi = _c
    capi.require_gpu()
    yield


def sp():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    """a numpy array of any of the kernel's types on the device, bit for bit (NaN payloads included)"""
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize == 2:
        return torch.from_numpy(a.view(np.int16).copy()).cuda()
    if a.dtype.itemsize == 4:
        return torch.from_numpy(a.view(np.int32).copy()).cuda()
    return torch.from_numpy(a.copy()).cuda()


def _launch(c, nsplit, indir, kc, vc):
    """One launch on fresh device copies of the caches and of the sentinel ctx -> (ctx, k_cache, v_cache) as unsigned integers."""
    L = capi.lib()
    rows, nh, dh, s_max = c["rows"], c["nh"], c["dh"], c["s_max"]
    Kc, Vc, ctx = _dev(kc), _dev(vc), _dev(c["ctx0"])
    keep = [_dev(c["qkv"]), _dev(c["bias"]), _dev(c["seq_len"]), _dev(c["pad"]), _dev(c["masked"]), _dev(c["fin"]),
            None if indir is None else _dev(indir)]
    if c["fp32"]:
        ws, wsb = None, 0
    else:
        wsb = rows * nh * (nsplit or PICKED_SPLITS) * (dh + 2) * 8
        if not nsplit:  # the case is named for the split count the launcher picks: it must be that one
            assert L.ftcf_masked_multihead_attention_workspace(rows, nh, dh, s_max) == wsb, "the launcher picked another split count"
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    capi.check(L.ftcf_masked_multihead_attention_beams(
        capi.FP32 if c["fp32"] else capi.FP16, capi.vp(keep[0]), capi.vp(keep[1]), capi.vp(Kc), capi.vp(Vc), capi.vp(keep[2]),
        capi.vp(keep[3]), capi.vp(keep[4]), capi.vp(keep[5]), capi.vp(keep[6]), c["K"], c["max_input_len"], rows, nh, dh, c["rot"],
        s_max, c["step"], nsplit, capi.vp(ctx), capi.vp(ws), C.c_size_t(wsb), sp()))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().view(c["ut"]) for t in (ctx, Kc, Vc))


def _errors(c, ref, got):
    """worst context and appended-key error over the live rows against the float64 reference: fp16 in ulps of _ulps, fp32 as a
    fraction of the largest term size of the (row, head); the appended value must be bit exact"""
    ctx_r, k_r, v_r, c_mag, k_mag = ref
    ca, ka, va = got
    tl, ft = c["tl"], c["ft"]
    worst_c = worst_k = 0.0
    at = None
    for b in range(c["rows"]):
        if c["fin"][b]:
            continue
        g_c, g_k = ca[b].view(ft), ka[b, :, tl].view(ft)
        assert np.isfinite(g_c.astype(np.float64)).all(), ("ctx not finite: a row beyond the live length was consumed", b)
        if c["fp32"]:
            ec = np.abs(g_c.astype(np.float64) - ctx_r[b]) / c_mag[b].max(axis=1, keepdims=True)
            ek = np.abs(g_k.astype(np.float64) - k_r[b]) / k_mag[b].max(axis=1, keepdims=True)
        else:
            ec = _ulps(g_c, ctx_r[b], CTX_FLOOR * c_mag[b])
            ek = _ulps(g_k, k_r[b], k_mag[b])
        if ec.max() > worst_c:
            worst_c, at = float(ec.max()), (b, np.unravel_index(int(ec.argmax()), ec.shape))
        worst_k = max(worst_k, float(ek.max()))
        assert np.array_equal(va[b, :, tl], v_r[b].view(c["ut"])), ("appended v not bit exact", b)
    return worst_c, worst_k, at


def _check(name, nsplit, fp32=False, refill=False):
    kw, _ = BEAM_CASES[name]
    c = beam_case(fp32=fp32, **kw)
    rows, K, tl, s_max, dh, ut = c["rows"], c["K"], c["tl"], c["s_max"], c["dh"], c["ut"]
    ref = beam_reference(c)
    got = _launch(c, nsplit, c["indir"], c["kc"], c["vc"])
    ca, ka, va = got
    # 2. the form without beams on the gathered cache: the same bits; its own error is the yardstick of the bounds
    dk, dv = _nan_bits(np.random.RandomState(tl), c["kc"].shape, fp32), _nan_bits(np.random.RandomState(tl + 1), c["kc"].shape, fp32)
    for b in range(rows):
        src = beam_source_rows(c["indir"], K, c["max_input_len"], c["step"], b, tl)
        dk[b, :, :tl] = c["kc"][src, :, np.arange(tl), :].transpose(1, 0, 2)
        dv[b, :, :tl] = c["vc"][src, :, np.arange(tl), :].transpose(1, 0, 2)
    plain = _launch(c, nsplit, None, dk, dv)
    pc, pk, pv = _errors(c, ref, plain)[:2], plain[1], plain[2]
    worst_c, worst_k, at = _errors(c, ref, got)
    form = "fp32" if fp32 else ("registers" if in_registers(dh, s_max, nsplit or PICKED_SPLITS) else "looped")
    unit = "" if fp32 else " ulp"
    print(f"[{name} nsplit {nsplit} {form}: beams ctx {worst_c:.3g}{unit} k {worst_k:.3g}{unit}; "
          f"no beams ctx {pc[0]:.3g}{unit} k {pc[1]:.3g}{unit}] ", end="")
    # 1. against float64
    bound_c, bound_k = (FP32_BOUND, FP32_BOUND) if fp32 else (CTX_ULPS, K_ULPS)
    assert pc[0] <= bound_c and pc[1] <= bound_k, ("the form without beams", pc)
    assert worst_c <= bound_c, ("ctx (row, (head, dim))", worst_c, at)
    assert worst_k <= bound_k, ("appended k", worst_k)
    live = np.flatnonzero(c["fin"] == 0)
    assert np.array_equal(ca[live], plain[0][live]), "ctx differs from the form without beams"
    assert np.array_equal(ka[live, :, tl], pk[live, :, tl]) and np.array_equal(va[live, :, tl], pv[live, :, tl])
    # 3. nothing else written; 4. a finished row's ctx and cache row untouched
    ek, ev = c["kc"].copy(), c["vc"].copy()
    ek[live, :, tl], ev[live, :, tl] = ka[live, :, tl], va[live, :, tl]
    for what, g, want in (("k_cache", ka, ek), ("v_cache", va, ev)):
        bad = np.argwhere(g != want)
        assert bad.size == 0, (what, "stray writes (row, head, t, dim)", bad[:8].tolist())
    for b in np.flatnonzero(c["fin"]):
        assert np.array_equal(ca[b], c["ctx0"][b]), ("finished row's ctx written", b)
    # 5. repeatable
    again = _launch(c, nsplit, c["indir"], c["kc"], c["vc"])
    assert all(np.array_equal(x, y) for x, y in zip(got, again)), "a second launch gave other bits"
    # 6. entries of the indirection that this step does not use do not matter
    if refill:
        ind2 = fill_indirection(np.random.RandomState(99), rows, K, s_max, c["max_input_len"], (c["step"] - c["max_input_len"]) & 1,
                                keep=c["indir"], tl=tl)
        assert (ind2 != c["indir"]).any()
        other = _launch(c, nsplit, ind2, c["kc"], c["vc"])
        assert all(np.array_equal(x, y) for x, y in zip(got, other)), "an unused indirection entry changed the result"


_FP16 = [(n, s) for n, (_, splits) in BEAM_CASES.items() for s in splits]


@pytest.mark.parametrize("name,nsplit", _FP16, ids=[f"{n}-{s}" for n, s in _FP16])
def test_beam_attention_matches_float64_and_the_form_without_beams(name, nsplit):
    _check(name, nsplit, refill=name in ("A1", "B"))


@pytest.mark.parametrize("name", FP32_CASES)
def test_fp32_beam_attention_matches_float64_and_the_form_without_beams(name):
    _check(name, 0, fp32=True)


def test_bad_arguments_are_errors_not_launches():
    """nsplit out of range, a workspace too small, scores that do not fit the LDS, rows that are no multiple of beam_width: an error
    return with a message, nothing launched, and the next call works."""
    c = beam_case(**BEAM_CASES["F2"][0])
    L = capi.lib()
    t = {k: _dev(c[k]) for k in ("qkv", "bias", "kc", "vc", "seq_len", "pad", "masked", "fin", "indir", "ctx0")}
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")

    def call(nsplit=1, wsb=1 << 20, s_max=c["s_max"], K=c["K"], rows=c["rows"]):
        return L.ftcf_masked_multihead_attention_beams(
            capi.FP16, capi.vp(t["qkv"]), capi.vp(t["bias"]), capi.vp(t["kc"]), capi.vp(t["vc"]), capi.vp(t["seq_len"]), capi.vp(t["pad"]),
            capi.vp(t["masked"]), capi.vp(t["fin"]), capi.vp(t["indir"]), K, c["max_input_len"], rows, c["nh"], c["dh"], c["rot"], s_max,
            c["step"], nsplit, capi.vp(t["ctx0"]), capi.vp(ws), C.c_size_t(wsb), sp())

    need = c["rows"] * c["nh"] * 2 * (c["dh"] + 2) * 8
    for kw in (dict(nsplit=17), dict(nsplit=-1), dict(nsplit=2, wsb=need - 1), dict(s_max=20000), dict(K=2)):
        assert call(**kw) != 0 and L.ftcf_last_error(), kw
    torch.cuda.synchronize()
    assert np.array_equal(t["ctx0"].cpu().numpy().view(np.uint16), c["ctx0"]) and np.array_equal(t["kc"].cpu().numpy().view(np.uint16), c["kc"])
    capi.check(call(nsplit=2, wsb=need))
    torch.cuda.synchronize()
