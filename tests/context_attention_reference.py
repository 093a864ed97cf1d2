"""Plain float64 numpy reference of the prompt-phase attention (include/ftcf.h ftcf_context_attention_range: k_qkv_bias_rotary_cache
+ k_context_attention_mfma, fp32: k32_qkv_bias_rotary_cache + k32_context_attention), its case table and its error measure, shared
by tests/test_context_attention_reference.py (CPU) and tests/test_gpu_context_attention.py (no GPU needed here).

The reference keeps the kernels' rounding points and nothing else: q, k, v = half(qkv + bias); NeoX rotary at position s (the index
in the right-padded row) as tests/attention_reference.py's _rotary, the rotated q and k rounded to half; the keys and values of
positions < s_lo taken from the cache AS GIVEN, those of [s_lo, s_hi) the freshly rounded ones; scores times float(half(1 /
sqrt(dh))) (the launcher rounds qk_scale to half: 1e-4 relative at dh 128); the causal mask key <= query < len; soft-max (with the
+1e-6 of the normaliser) and P.V in float64; the context rounded to half once.  The fp32 variant rounds to float32 where the fp16
one rounds to half and uses the unrounded scale.

Error of the context: the kernel rounds the unnormalised P to half before P.V but sums the normaliser unrounded, so every weight
carries a relative error of at most 2^-11, and the output is rounded once: |got - ctx64| <= U, U = 2^-11 (c_mag + |ctx64|), c_mag =
sum p |v| / den and ctx64 the reference's context BEFORE its own rounding (the fp32 exp and accumulation terms are two orders
smaller).  The error is measured against ctx64, not against the rounded ctx: two values rounded apart may sit a whole ulp from each
other, which is outside what the bound derives (against the rounded ctx the same runs give exactly 1.00 U wherever got and ctx fall
on either side of a rounding point at the bottom of a binade with |ctx| = c_mag).  Errors are reported as a fraction of U.  For
scale: at 520 keys one key moves an element by about c_mag / 520 ~ 4 U, at 200 keys or fewer by at least 10 U.
Measured on MI355X over every fp16 case of CASES, split on and off, the chunk chain included (profiles/context_attention_tests.md
has every case): worst 0.84 U, case H256-128 (dh 256,
rot 128, whole prompt), sequence 0, row 2 (three keys), head 0, dim 126.  Every case's worst sits in a row of two to seven keys
(0.54 .. 0.84); the launches that start at s_lo >= 37, whose rows all have 38 keys or more, stay at 0.14 .. 0.54.  That is the
finding behind CTX_FRAC: U is a worst-case bound, and a row of two or three keys -- one weight's rounding plus the output's, both
near their maximum somewhere among thousands of elements -- nearly attains it, as a worst-case bound should be attained; among many
keys the roundings average out.  1.5 x 0.84 = 1.26 is above the cap of 1.0, so CTX_FRAC is the cap: the bound is a hard one there
(no seed can pass it but for the fp32 terms, 3e-3 U), and it is the tightest that short rows allow.  It still sees one key: the
probes below move every later row by more than 4 U.
The q written back and the appended K rows: K_ULPS of tests/attention_reference.py at the size of the rotated pair; V rows: bit
exact; fp32: FP32_BOUND x the term size, as tests/test_gpu_beam_attention.py."""
import functools

import numpy as np

from tests.attention_reference import HEAD_SIZES, K_ULPS, _half, _nan_bits, _rotary, _sentinel, _single, _ulps  # noqa: F401

# worst context error as a fraction of U over every fp16 case on MI355X, and where; CTX_FRAC = min(1.5 x that, rounded up to two
# digits, the cap 1.0)
MEASURED = (0.84, "H256-128, sequence 0, row 2, head 0, dim 126")
CTX_FRAC = 1.0
FP32_BOUND = 5e-5
EPS = 2.0 ** -11


def key_tile(dh):
    return 32 if dh > 128 else 64


def split_count(dh, s_lo, s_hi):
    """Mirror of launch_context_attention's rule (FTCF_CTX_SPLIT unset): how many of the launch's query blocks, counted from the
    last one, are cut in two along their keys.  Query block n (0 = the last) is taken to see keys up to s_hi - 1 - 64 n."""
    kt = key_tile(dh)
    tmax = (s_hi - 1) // kt + 1
    if tmax < 8:
        return 0
    nqb, n2 = (s_hi - s_lo + 63) // 64, 0
    while n2 < nqb and (s_hi - 1 - 64 * n2) // kt + 1 > tmax // 2:
        n2 += 1
    return n2


def split_cut(dh, q_last):
    """first key of the second half of a split query block whose last cached key is q_last"""
    kt = key_tile(dh)
    return (q_last // kt + 1) // 2 * kt


def context_case(dh, rot, nh=2, B=1, S=0, s_max=0, lens=(), crm=1, s_lo=0, s_hi=None, seed=0, fp32=False):
    """The inputs of one launch.  qkv [B, S, 3, nh, dh] and bias [3, nh, dh]: randn and 0.1 randn, rounded (the qkv rows outside
    [s_lo, s_hi) too: finite, and not to be touched).  ctx0 [B, S, nh, dh]: sentinel bits.  Caches [B * crm, nh, s_max, dh] as
    unsigned integers: positions [0, min(s_lo, len)) of sequence b's row b * crm hold finite random values (an earlier chunk's K/V),
    every other element a NaN bit pattern: [s_lo, s_max), the rows crm skips, positions >= len below s_lo."""
    rng = np.random.RandomState(seed)
    ft, ut, rnd = (np.float32, np.uint32, _single) if fp32 else (np.float16, np.uint16, _half)
    s_hi = S if s_hi is None else s_hi
    lens = np.asarray(lens, dtype=np.int32)
    assert len(lens) == B and 1 <= int(lens.min()) and int(lens.max()) <= S <= s_max and 0 <= s_lo < s_hi <= S
    qkv = rnd(rng.randn(B, S, 3, nh, dh))
    bias = rnd(0.1 * rng.randn(3, nh, dh))
    kc = _nan_bits(rng, (B * crm, nh, s_max, dh), fp32)
    vc = _nan_bits(rng, (B * crm, nh, s_max, dh), fp32)
    for b in range(B):
        n = min(s_lo, int(lens[b]))
        kc[b * crm, :, :n] = rnd(rng.randn(nh, n, dh)).view(ut)
        vc[b * crm, :, :n] = rnd(rng.randn(nh, n, dh)).view(ut)
    ctx0 = _sentinel(rng, B * S * nh * dh).reshape(B, S, nh, dh).astype(ut)
    return dict(dh=dh, rot=rot, nh=nh, B=B, S=S, s_max=s_max, lens=lens, crm=crm, s_lo=s_lo, s_hi=s_hi, fp32=fp32, ft=ft, ut=ut,
                qkv=qkv, bias=bias, kc=kc, vc=vc, ctx0=ctx0)


def reference_context(c, qkv=None, kc=None, vc=None, s_lo=None, s_hi=None):
    """The launch of case c in float64 (qkv, caches, range: others than the case's own).  Per sequence b, over its rows
    [s_lo, e), e = min(len, s_hi) (None where there is none): ctx, q (rotated), k, v [e - s_lo, nh, dh] rounded to the kernel's
    type, ctx64 (the context before its one rounding: what the errors are measured against), and the magnitudes c_mag = sum p |v| /
    den, k_mag / q_mag = the size of the rotated pair."""
    fp32, nh, dh, rot, crm = c["fp32"], c["nh"], c["dh"], c["rot"], c["crm"]
    ft, rnd = c["ft"], (_single if fp32 else _half)
    qkv = c["qkv"] if qkv is None else qkv
    kc = (c["kc"] if kc is None else kc).view(ft)
    vc = (c["vc"] if vc is None else vc).view(ft)
    s_lo = c["s_lo"] if s_lo is None else s_lo
    s_hi = c["s_hi"] if s_hi is None else s_hi
    scale = 1.0 / np.sqrt(dh) if fp32 else float(np.float16(np.float32(1.0) / np.sqrt(np.float32(dh))))
    out = {k: [None] * c["B"] for k in ("ctx", "ctx64", "q", "k", "v", "c_mag", "k_mag", "q_mag")}
    for b in range(c["B"]):
        e = min(int(c["lens"][b]), s_hi)
        if e <= s_lo:
            continue
        x = rnd(qkv[b, s_lo:e].astype(np.float64) + c["bias"].astype(np.float64)[None])  # [n, 3, nh, dh]
        q, k, v = x[:, 0].copy(), x[:, 1].copy(), x[:, 2]
        for i in range(e - s_lo):
            q[i] = _rotary(x[i, 0], s_lo + i, rot, rnd)
            k[i] = _rotary(x[i, 1], s_lo + i, rot, rnd)
        keys = np.concatenate([kc[b * crm, :, :s_lo].astype(np.float64), k.astype(np.float64).transpose(1, 0, 2)], axis=1)  # [nh, e, dh]
        vals = np.concatenate([vc[b * crm, :, :s_lo].astype(np.float64), v.astype(np.float64).transpose(1, 0, 2)], axis=1)
        assert np.isfinite(keys).all() and np.isfinite(vals).all(), "the case holds a non-finite value where the reference reads"
        s = np.einsum("ihd,htd->hit", q.astype(np.float64), keys) * scale  # [nh, n, e]
        s[:, np.arange(e)[None, :] > (s_lo + np.arange(e - s_lo))[:, None]] = -np.inf
        p = np.exp(s - s.max(axis=2, keepdims=True))
        den = (p.sum(axis=2) + 1e-6).T[:, :, None]  # [n, nh, 1]
        out["ctx64"][b] = np.einsum("hit,htd->ihd", p, vals) / den
        out["ctx"][b] = rnd(out["ctx64"][b])
        out["c_mag"][b] = np.einsum("hit,htd->ihd", p, np.abs(vals)) / den
        out["q"][b], out["k"][b], out["v"][b] = q, k, v
        for name, j in (("q_mag", 0), ("k_mag", 1)):
            m = np.abs(x[:, j].astype(np.float64))
            m[..., :rot // 2] = m[..., rot // 2:rot] = m[..., :rot // 2] + m[..., rot // 2:rot]
            out[name][b] = m
    return out


def ctx_unit(ref, b):
    """U of every context element of sequence b's rows (+ 2^-25: half an ulp of a subnormal half, where the rounding is absolute)"""
    return EPS * (ref["c_mag"][b] + np.abs(ref["ctx64"][b])) + 2.0 ** -25


# ---------------------------------------------------------------------------------------------------------------------
# the case table: name -> context_case arguments; the smallest shapes that reach each form (KT: 64 keys at dh <= 128, 32 above;
# the key split needs (s_hi - 1) / KT + 1 >= 8)
# ---------------------------------------------------------------------------------------------------------------------
CASES = {}
_seed = iter(range(1000, 2000))
# head sizes, whole prompt: both rotary kernels (rot % 16 zero and not), the zero-padded d steps (48, 80, 144, ...), rot 0 and rot = dh
HEAD_CASES = HEAD_SIZES + [(64, 0), (64, 64), (128, 0), (128, 128)]
for _dh, _rot in HEAD_CASES:
    CASES[f"H{_dh}-{_rot}"] = dict(dh=_dh, rot=_rot, B=2, S=70, s_max=96, lens=(70, 37), seed=next(_seed))
# length edges, once with S == s_max
for _dh, _rot in ((128, 32), (64, 16)):
    for _sm in (130, 192):
        CASES[f"L{_dh}-{_sm}"] = dict(dh=_dh, rot=_rot, B=8, S=130, s_max=_sm, lens=(1, 16, 17, 63, 64, 65, 129, 130), seed=next(_seed))
# the cache row multiplier: K/V land in cache rows 0 and 3
CASES["M3"] = dict(dh=128, rot=32, B=2, S=70, s_max=96, lens=(70, 37), crm=3, seed=next(_seed))
# token ranges of one sequence, as the engine cuts them
RANGES = [(0, 1), (0, 64), (64, 200), (48, 49), (37, 101), (100, 163), (100, 200), (199, 200)]
for _dh, _rot in ((128, 32), (64, 16), (256, 128)):
    for _lo, _hi in RANGES:
        CASES[f"R{_dh}-{_lo}-{_hi}"] = dict(dh=_dh, rot=_rot, B=1, S=200, s_max=224, lens=(200,), s_lo=_lo, s_hi=_hi, seed=next(_seed))
# ragged: a row that ends inside the range; a row shorter than s_lo (its ctx keeps its bits, its cache rows in the range become zeros)
for _lo, _hi in ((100, 163), (150, 200)):
    CASES[f"RR-{_lo}-{_hi}"] = dict(dh=128, rot=32, B=2, S=200, s_max=224, lens=(200, 120), s_lo=_lo, s_hi=_hi, seed=next(_seed))
# the key split with a range ((449, 450): one token, one block, split at key 256; (400, 520): the probes' base)
for _lo, _hi in ((0, 520), (400, 460), (448, 520), (449, 450), (400, 520)):
    CASES[f"S-{_lo}-{_hi}"] = dict(dh=128, rot=32, B=1, S=520, s_max=544, lens=(520,), s_lo=_lo, s_hi=_hi, seed=next(_seed))
CASES["S-400-520"]["seed"] = 3148  # chosen for the probe condition (a condition on the inputs, decided by the reference alone)
CASES["SR-384-520"] =dict(dh=128, rot=32, B=3, S=520, s_max=544, lens=(520, 130, 421), s_lo=384, s_hi=520, seed=next(_seed))
for _lo, _hi in ((0, 260), (225, 260)):  # the key split at KT 32
    CASES[f"S256-{_lo}-{_hi}"] = dict(dh=256, rot=128, B=1, S=260, s_max=288, lens=(260,), s_lo=_lo, s_hi=_hi, seed=next(_seed))
FP32_CASES = ["H80-80", "H128-32", "H256-128", "L128-192", "M3"]  # whole prompt only
# the launches that split, with the number of split query blocks; every other case must not split
SPLITS = {"S-0-520": 5, "S-400-460": 1, "S-448-520": 2, "S-449-450": 1, "S-400-520": 2, "SR-384-520": 3, "S256-0-260": 3, "S256-225-260": 1}
CHAIN = ("R128-0-1", [(0, 48), (48, 163), (163, 200)])  # the chunk chain: the case whose shape it takes, its ranges
for _n, _kw in CASES.items():
    assert split_count(_kw["dh"], _kw.get("s_lo", 0), _kw.get("s_hi", _kw["S"])) == SPLITS.get(_n, 0), _n


@functools.lru_cache(maxsize=None)
def case_and_reference(name, fp32=False):
    """(case, reference) of a table entry, computed once and shared: read-only"""
    c = context_case(fp32=fp32, **CASES[name])
    return c, reference_context(c)


# ---------------------------------------------------------------------------------------------------------------------
# single-key probes: one V row (or K row) of one position replaced by 8 randn; decided by the reference alone
# ---------------------------------------------------------------------------------------------------------------------
PROBE_SETS = {"R128-100-200": None, "S-400-520": 256}  # base case -> cut (the split's first key of the second half; None: no split)


def probe_list(name):
    """[(kind, j)]: "v" at {0, 63, 64, s_lo - 1, s_lo, s_lo + 15, s_lo + 16, cut - 1, cut, s_hi - 1}, "k" at s_lo - 1 and cut"""
    kw, cut = CASES[name], PROBE_SETS[name]
    s_lo, s_hi = kw["s_lo"], kw["s_hi"]
    pos = [0, 63, 64, s_lo - 1, s_lo, s_lo + 15, s_lo + 16] + ([] if cut is None else [cut - 1, cut]) + [s_hi - 1]
    pos = sorted({j for j in pos if 0 <= j < s_hi})
    return [("v", j) for j in pos] + [("k", j) for j in ([s_lo - 1] + ([] if cut is None else [cut])) if 0 <= j < s_hi]


def probe_inputs(c, kind, j):
    """(qkv, kc, vc) of case c (one sequence) with the value (kind "v") or key (kind "k") of position j replaced by 8 randn,
    rounded: below s_lo the cache row, from s_lo on the v / k part of qkv row j"""
    rng = np.random.RandomState(7000 + 2 * j + (kind == "k"))
    new = _half(8 * rng.randn(c["nh"], c["dh"]))
    qkv, kc, vc = c["qkv"].copy(), c["kc"].copy(), c["vc"].copy()
    if j < c["s_lo"]:
        (vc if kind == "v" else kc)[0, :, j] = new.view(c["ut"])
    else:
        qkv[0, j, 2 if kind == "v" else 1] = new
    return qkv, kc, vc


@functools.lru_cache(maxsize=None)
def probe_reference(name, kind, j):
    c, _ = case_and_reference(name)
    qkv, kc, vc = probe_inputs(c, kind, j)
    return reference_context(c, qkv=qkv, kc=kc, vc=vc)
