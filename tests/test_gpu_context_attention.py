"""-m gpu: the prompt-phase attention at kernel level (include/ftcf.h ftcf_context_attention_range: k_qkv_bias_rotary_cache +
k_context_attention_mfma with a token range, a cache row multiplier and the key split; fp32: k32_qkv_bias_rotary_cache +
k32_context_attention) against the float64 reference of tests/context_attention_reference.py.

Every cache element the launch may not consume holds a NaN bit pattern and ctx starts as sentinel bits, so a read past the last
cached key is a NaN and a write outside the range is a changed bit: after each launch EVERY element of ctx, qkv and both caches is
either checked against the reference or required to keep its bits.  The bound of the context, CTX_FRAC x U, is a fraction of the
size of ONE weight's rounding (see the reference module), far below what one dropped or doubled key costs; the single-key probes
show that directly."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.context_attention_reference import (CASES, CHAIN, CTX_FRAC, FP32_BOUND, FP32_CASES, K_ULPS, PROBE_SETS, SPLITS, _ulps,
                                               case_and_reference, context_case, ctx_unit, probe_inputs, probe_list, probe_reference,
                                               reference_context)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

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


def _dev(a):
    """a numpy array of any of the kernel's types on the device, bit for bit (NaN payloads included)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize]).copy()).cuda()


def _initial(c, qkv=None, kc=None, vc=None):
    """what a launch starts from, as unsigned integers"""
    ut = c["ut"]
    return dict(qkv=(c["qkv"] if qkv is None else qkv).view(ut), kc=c["kc"] if kc is None else kc, vc=c["vc"] if vc is None else vc,
                ctx=c["ctx0"])


def _call(c, t, s_lo, s_hi, **over):
    a = dict(dtype=capi.FP32 if c["fp32"] else capi.FP16, B=c["B"], S=c["S"], nh=c["nh"], dh=c["dh"], rot=c["rot"], s_max=c["s_max"],
             crm=c["crm"], s_lo=s_lo, s_hi=s_hi)
    a.update(over)
    return capi.lib().ftcf_context_attention_range(a["dtype"], capi.vp(t["qkv"]), capi.vp(t["bias"]), capi.vp(t["lens"]),
                                                   capi.vp(t["kc"]), capi.vp(t["vc"]), a["B"], a["S"], a["nh"], a["dh"], a["rot"],
                                                   a["s_max"], a["crm"], a["s_lo"], a["s_hi"], capi.vp(t["ctx"]), sp())


def _tensors(c, init):
    t = {k: _dev(v) for k, v in init.items()}
    t["bias"], t["lens"] = _dev(c["bias"]), _dev(c["lens"])
    return t


def _read(c, t):
    torch.cuda.synchronize()
    return {k: t[k].cpu().numpy().view(c["ut"]).reshape(_shape(c, k)) for k in ("qkv", "kc", "vc", "ctx")}


def _shape(c, k):
    return {"qkv": c["qkv"].shape, "kc": c["kc"].shape, "vc": c["kc"].shape, "ctx": c["ctx0"].shape}[k]


def _launch(c, init, ranges=None):
    """The launches of `ranges` (default: the case's own) in succession on fresh device copies of init -> qkv, kc, vc, ctx as
    unsigned integers."""
    t = _tensors(c, init)
    for s_lo, s_hi in ranges or [(c["s_lo"], c["s_hi"])]:
        capi.check(_call(c, t, s_lo, s_hi))
    return _read(c, t)


def _verify(c, ref, got, init, s_lo, s_hi, bound=None):
    """Every element of what the launch of [s_lo, s_hi) left: checked against the reference, or the bits it started with.
    Returns the worst context error (fp16: as a fraction of U; fp32: of the largest term of the (row, head)) and where."""
    ft, ut, fp32, crm = c["ft"], c["ut"], c["fp32"], c["crm"]
    bound = (FP32_BOUND if fp32 else CTX_FRAC) if bound is None else bound
    exp = {k: v.copy() for k, v in init.items()}
    worst, at = 0.0, None
    for b in range(c["B"]):
        ln, row = int(c["lens"][b]), b * crm
        e = min(ln, s_hi)
        if e > s_lo:
            g = got["ctx"][b, s_lo:e].view(ft).astype(np.float64)
            assert np.isfinite(g).all(), ("ctx not finite: a cache row beyond the last cached key was consumed", b)
            r = ref["ctx64"][b]
            err = np.abs(g - r) / (ref["c_mag"][b].max(axis=-1, keepdims=True) if fp32 else ctx_unit(ref, b))
            if err.max() > worst:
                worst, at = float(err.max()), (b,) + tuple(int(i) for i in np.unravel_index(int(err.argmax()), err.shape))
            for what, g_x, r_x, mag in (("k", got["kc"][row, :, s_lo:e].view(ft).transpose(1, 0, 2), ref["k"][b], ref["k_mag"][b]),
                                        ("q", got["qkv"][b, s_lo:e, 0].view(ft), ref["q"][b], ref["q_mag"][b])):
                if fp32:
                    ek = np.abs(g_x.astype(np.float64) - r_x.astype(np.float64)) / mag.max(axis=-1, keepdims=True)
                    assert ek.max() <= FP32_BOUND, (what, b, float(ek.max()))
                else:
                    ek = _ulps(g_x, r_x, mag)
                    assert ek.max() <= K_ULPS, (what, b, float(ek.max()))
            assert np.array_equal(got["vc"][row, :, s_lo:e].transpose(1, 0, 2), ref["v"][b].view(ut)), ("v rows not bit exact", b)
            for k, idx in (("ctx", (b, slice(s_lo, e))), ("kc", (row, slice(None), slice(s_lo, e))), ("qkv", (b, slice(s_lo, e), 0))):
                exp[k][idx] = got[k][idx]
            exp["vc"][row, :, s_lo:e] = got["vc"][row, :, s_lo:e]
        z = max(ln, s_lo)
        if z < s_hi:  # padding inside the range: zeros
            exp["kc"][row, :, z:s_hi] = 0
            exp["vc"][row, :, z:s_hi] = 0
            exp["qkv"][b, z:s_hi, 0] = 0
    assert worst <= bound, ("ctx (sequence, row - s_lo, head, dim)", worst, at)
    for k in ("ctx", "qkv", "kc", "vc"):
        bad = np.argwhere(got[k] != exp[k])
        assert bad.size == 0, (k, "written or not written where it must not / must be", bad[:8].tolist())
    return worst, at


def _check(name, fp32, monkeypatch):
    c, ref = case_and_reference(name, fp32)
    init = _initial(c)
    runs = {}
    for split in ((None, "0") if (name in SPLITS and not fp32) else (None,)):
        if split is None:
            monkeypatch.delenv("FTCF_CTX_SPLIT", raising=False)
        else:
            monkeypatch.setenv("FTCF_CTX_SPLIT", split)
        got = _launch(c, init)
        worst, at = _verify(c, ref, got, init, c["s_lo"], c["s_hi"])
        print(f"[{name}{' fp32' if fp32 else ''} split {'on' if split is None else 'off'}: ctx {worst:.3g} at {at}] ", end="")
        again = _launch(c, init)
        assert all(np.array_equal(got[k], again[k]) for k in got), "a second launch gave other bits"
        runs[split] = got
    if len(runs) == 2:
        assert not np.array_equal(runs[None]["ctx"], runs["0"]["ctx"]), "the split did not run: the same bits with FTCF_CTX_SPLIT=0"
        for k in ("qkv", "kc", "vc"):
            assert np.array_equal(runs[None][k], runs["0"][k]), k


@pytest.mark.parametrize("name", list(CASES))
def test_context_attention_matches_float64_and_writes_nothing_else(name, monkeypatch):
    _check(name, False, monkeypatch)


@pytest.mark.parametrize("name", FP32_CASES)
def test_fp32_context_attention_matches_float64_and_writes_nothing_else(name, monkeypatch):
    _check(name, True, monkeypatch)


def test_chunk_chain_equals_the_whole_prompt(monkeypatch):
    """Three ranges in succession over a cache of NaN bits: the K/V they leave are the whole-prompt call's bit for bit, and every
    context row meets the bound against the whole-prompt reference (its keys below s_lo are what the earlier launches wrote)."""
    monkeypatch.delenv("FTCF_CTX_SPLIT", raising=False)
    name, ranges = CHAIN
    c = context_case(**dict(CASES[name], s_lo=0, s_hi=CASES[name]["S"]))
    ref, init = reference_context(c), _initial(c)
    whole = _launch(c, init)
    _verify(c, ref, whole, init, 0, c["S"])
    assert ranges[0][0] == 0 and ranges[-1][1] == c["S"] and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    chain = _launch(c, init, ranges)
    worst, at = _verify(c, ref, chain, init, 0, c["S"])
    print(f"[chain: ctx {worst:.3g} at {at}] ", end="")
    for k in ("kc", "vc", "qkv"):
        assert np.array_equal(chain[k], whole[k]), (k, "differs from the whole-prompt call's")


_base = {}


def _probe_base(name):
    if name not in _base:
        c, ref = case_and_reference(name)
        init = _initial(c)
        got = _launch(c, init)
        _verify(c, ref, got, init, c["s_lo"], c["s_hi"])
        _base[name] = got
    return _base[name]


_PROBES = [(n, kind, j) for n in PROBE_SETS for kind, j in probe_list(n)]


@pytest.mark.parametrize("name,kind,j", _PROBES, ids=[f"{n}-{k}{j}" for n, k, j in _PROBES])
def test_one_key_reaches_every_later_row_and_no_earlier_one(name, kind, j, monkeypatch):
    """The value (or key) of position j replaced: the rows before j keep their bits (no leak from the future); every row from j on
    whose reference moves by more than 4 U in every head (tests/test_context_attention_reference.py: all of them for a value)
    changes; and the change is the reference's.  Each launch is within CTX_FRAC x its own U of its reference, so the two
    differences agree within CTX_FRAC x (U_base + U_probe) = 2 CTX_FRAC x the mean of the two U."""
    monkeypatch.delenv("FTCF_CTX_SPLIT", raising=False)
    c, ref = case_and_reference(name)
    s_lo, s_hi = c["s_lo"], c["s_hi"]
    base = _probe_base(name)["ctx"][0, s_lo:s_hi]
    qkv, kc, vc = probe_inputs(c, kind, j)
    pref = probe_reference(name, kind, j)
    got = _launch(c, _initial(c, qkv, kc, vc))["ctx"][0, s_lo:s_hi]
    i0 = max(j - s_lo, 0)
    assert np.array_equal(got[:i0], base[:i0]), "a row before the changed position changed"
    ft = c["ft"]
    g_d = got.view(ft).astype(np.float64) - base.view(ft).astype(np.float64)
    assert np.isfinite(g_d).all()
    r_d = pref["ctx64"][0] - ref["ctx64"][0]
    u = 0.5 * (ctx_unit(ref, 0) + ctx_unit(pref, 0))
    moved = (np.abs(r_d) / ctx_unit(ref, 0)).max(axis=2).min(axis=1) > 4.0  # per row: every head has an element beyond 4 U
    assert not moved[:i0].any()
    same = np.array([np.array_equal(got[i], base[i]) for i in range(len(got))])
    assert not (same & moved).any(), ("rows (from s_lo) that did not see the change", np.flatnonzero(same & moved)[:8].tolist())
    err = np.abs(g_d - r_d) / u
    print(f"[{name} {kind}{j}: moved {int(moved.sum())} of {len(got) - i0}, difference off by {err.max():.3g} U] ", end="")
    assert err.max() <= 2 * CTX_FRAC, ("the change is not the reference's (row from s_lo, head, dim)",
                                       float(err.max()), np.unravel_index(int(err.argmax()), err.shape))


def test_bad_arguments_are_errors_not_launches():
    """rot odd / negative / above dh, an empty or overhanging range, S > s_max, an unsupported head size, B / nh / cache_row_mult
    below 1, a NULL tensor, fp32 with a range: an error return with a message, nothing launched, and the next call works."""
    c, _ = case_and_reference("R64-37-101")
    init = _initial(c)
    t = _tensors(c, init)
    L = capi.lib()
    bad = [dict(rot=15), dict(rot=-2), dict(rot=c["dh"] + 16), dict(s_lo=50, s_hi=50), dict(s_lo=60, s_hi=50), dict(s_lo=-1),
           dict(s_hi=c["S"] + 1), dict(S=c["s_max"] + 1, s_hi=c["s_max"] + 1), dict(dh=40), dict(dh=72), dict(B=0), dict(nh=0),
           dict(crm=0), dict(dtype=capi.FP32, s_lo=37, s_hi=101), dict(dtype=capi.FP32, s_lo=0, s_hi=101), dict(dtype=capi.BF16)]
    for kw in bad:
        assert _call(c, t, kw.pop("s_lo", c["s_lo"]), kw.pop("s_hi", c["s_hi"]), **kw) != 0 and L.ftcf_last_error(), kw
    for k in ("qkv", "bias", "lens", "kc", "vc", "ctx"):
        assert _call(c, dict(t, **{k: None}), c["s_lo"], c["s_hi"]) != 0 and L.ftcf_last_error(), k
    got = _read(c, t)
    assert all(np.array_equal(got[k], init[k]) for k in got), "a rejected call wrote something"
    capi.check(_call(c, t, c["s_lo"], c["s_hi"]))
    torch.cuda.synchronize()
