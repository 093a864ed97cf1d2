"""Plain float64 numpy references of one decode-attention step, shared by the kernel-level attention tests (no GPU needed).

The references keep the kernels' rounding points and nothing else: q, k, v = half(qkv + bias); NeoX rotary with the angle in fp32
(pos / 10000^(2j/rot)), cos / sin and the rotation in float64, the rotated q and k rounded to half; scores, soft-max (with the
+1e-6 of the normaliser) and P.V in float64; the context rounded to half once.  The fp32 variant rounds to float32 where the
fp16 one rounds to half.

Errors are counted in half-precision ulps (see _ulps): the context at max(|ctx|, CTX_FLOOR x the size of the terms it averages),
the appended key at max(|k|, the size of the rotated pair).  CTX_ULPS / K_ULPS were measured on MI355X over every case of
tests/test_gpu_paged_attention.py: worst context error 4.00 ulp (a 49-key slot, dh 128, full rotary, P 48), worst appended-key
error 1.38 ulp (position 14,751, full rotary)."""
import numpy as np

CTX_FLOOR = 1 / 64
CTX_ULPS = 6
K_ULPS = 2


def _sentinel(rng, n):
    """n random fp16 bit patterns, all finite (bit 10 clear: the exponent is never all ones), as uint16."""
    return (rng.randint(0, 1 << 16, size=n).astype(np.uint16) & np.uint16(0xFBFF))


def _half(x):
    return np.asarray(x, dtype=np.float64).astype(np.float16)


def _single(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _rotary(x, pos, rot, rnd=_half):
    """NeoX rotary of vectors x [..., dh] at position pos, rounded as the kernel rounds it (rotary_coef / rotary_apply)."""
    if rot == 0:
        return x
    j = np.arange(rot // 2, dtype=np.float32)
    den = (10000.0 ** ((2 * j) / np.float32(rot)).astype(np.float64)).astype(np.float32)  # powf, correctly rounded
    ang = (np.float32(pos) / den).astype(np.float64)  # an fp32 quotient
    cs, sn = np.cos(ang), np.sin(ang)
    a, b = x[..., :rot // 2].astype(np.float64), x[..., rot // 2:rot].astype(np.float64)
    out = x.copy()
    out[..., :rot // 2] = rnd(cs * a - sn * b)
    out[..., rot // 2:rot] = rnd(cs * b + sn * a)
    return out


def _ulps(got, ref, mag):
    """|got - ref| (ref already rounded to half) in half-precision ulps at max(|ref|, mag).  The context: mag = CTX_FLOOR x the
    size of the terms it averages, so that an output that cancels to near zero is not counted at a subnormal ulp, while over
    thousands of keys (|ctx| ~ 0.01, a single key weighing 1 / len) one dropped key still costs tens of ulps.  The appended key:
    mag = the size of the rotated pair, the scale at which a rotation by an fp32 angle errs (the angle's own ulp is 1e-3 rad near
    position 15000)."""
    m = np.maximum(np.maximum(np.abs(ref.astype(np.float64)), mag), 2.0 ** -14).astype(np.float16)
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(m).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# beam search: the dense cache [rows, nh, s_max, dh] read through the cache indirection
# ---------------------------------------------------------------------------------------------------------------------
def beam_source_rows(indir, K, max_input_len, step, b, tl):
    """The cache rows that hold the keys of times [0, tl) of row b: (b / K) * K + indir[(step - max_input_len) & 1][b][t]
    (indir None: the row's own)."""
    if indir is None:
        return np.full(tl, b, dtype=np.int64)
    return b // K * K + indir[(step - max_input_len) & 1, b, :tl].astype(np.int64)


def reference_beam_step(qkv, bias, kc, vc, indir, K, max_input_len, seq_len, pad_count, masked, fin, nh, dh, rot, step, fp32=False):
    """One decode-attention step of beam search in float64.  qkv [rows, 3, nh, dh], bias [3, nh, dh], caches [rows, nh, s_max, dh],
    indir [2, rows, s_max] int32 or None, masked [rows, s_max] (1: probability 0), all in the kernel's type (half; fp32: float32).
    Row b: rotary at step - 1 - pad_count[b]; the key / value of time t < seq_len[b] from the row beam_source_rows() names, the
    current token from the row's own q, k, v.  Returns ctx, k_new, v_new [rows][nh, dh] (finished rows: None) and the magnitudes
    c_mag / k_mag of tests/test_gpu_paged_attention.py's reference_step."""
    rnd = _single if fp32 else _half
    rows = len(seq_len)
    x = rnd(qkv.astype(np.float64) + bias.astype(np.float64)[None])
    ctx, k_new, v_new, c_mag, k_mag = ([None] * rows for _ in range(5))
    for b in range(rows):
        if fin[b]:
            continue
        tl = int(seq_len[b])
        pos = step - 1 - int(pad_count[b])
        q = _rotary(x[b, 0], pos, rot, rnd)
        k = _rotary(x[b, 1], pos, rot, rnd)
        v = x[b, 2]
        t = np.arange(tl)
        src = beam_source_rows(indir, K, max_input_len, step, b, tl)
        keys = np.concatenate([kc[src, :, t, :].astype(np.float64), k[None].astype(np.float64)])  # [tl + 1, nh, dh]
        vals = np.concatenate([vc[src, :, t, :].astype(np.float64), v[None].astype(np.float64)])
        s = np.einsum("thd,hd->ht", keys, q.astype(np.float64)) / np.sqrt(dh)
        dead = np.concatenate([masked[b, :tl] != 0, [False]])
        s[:, dead] = -np.inf
        p = np.exp(s - s.max(axis=1, keepdims=True))
        den = (p.sum(axis=1) + 1e-6)[:, None]
        ctx[b], k_new[b], v_new[b] = rnd(np.einsum("ht,thd->hd", p, vals) / den), k, v
        c_mag[b] = np.einsum("ht,thd->hd", p, np.abs(vals)) / den
        xk = np.abs(x[b, 1].astype(np.float64))
        k_mag[b] = xk.copy()
        k_mag[b][:, :rot // 2] = k_mag[b][:, rot // 2:rot] = xk[:, :rot // 2] + xk[:, rot // 2:rot]
    return ctx, k_new, v_new, c_mag, k_mag


def _nan_bits(rng, shape, fp32):
    """random NaN bit patterns (either sign, a non-zero mantissa) of the cache's type, as unsigned integers"""
    if fp32:
        return (rng.randint(1, 1 << 23, size=shape).astype(np.uint32) | np.uint32(0x7F800000)
                | (rng.randint(0, 2, size=shape).astype(np.uint32) << np.uint32(31)))
    return (rng.randint(1, 1 << 10, size=shape).astype(np.uint16) | np.uint16(0x7C00)
            | (rng.randint(0, 2, size=shape).astype(np.uint16) << np.uint16(15)))


def fill_indirection(rng, rows, K, s_max, max_input_len, src_plane, keep=None, tl=0):
    """Both planes [2, rows, s_max], every entry in [0, K).  The source plane: 0 at t < max_input_len, uniform in [0, K) at every
    later t (those beyond the live length too: the kernel may dereference them); the other plane: (source + 1) % K.  keep: an
    earlier result whose source-plane entries at t < tl are kept (everything a step of length tl does not use is redrawn)."""
    ind = np.empty((2, rows, s_max), dtype=np.int32)
    src = rng.randint(0, K, size=(rows, s_max)).astype(np.int32)
    src[:, :max_input_len] = 0
    ind[src_plane] = src
    ind[1 - src_plane] = (src + 1) % K
    if keep is not None:
        ind[1 - src_plane] = rng.randint(0, K, size=(rows, s_max))
        ind[src_plane, :, :tl] = keep[src_plane, :, :tl]
    assert ind.min() >= 0 and ind.max() < K
    return ind


def beam_case(dh, rot, nh, batch, K, s_max, max_input_len, lens, tl, finished=(), seed=0, fp32=False):
    """The inputs of one beam-search decode-attention launch: rows = batch * K, every live row at seq_len = tl, step = tl + 1;
    entry e's prompt has lens[e] tokens, followed by max_input_len - lens[e] pad positions (pad_count; masked_tokens marks
    [lens[e], max_input_len)).
    Every cache row holds finite random values of its own at t < tl (a read from a wrong row is wrong but finite; masked positions
    too: the kernel multiplies their value by a zero weight) and NaN bit patterns at t >= tl (fetched speculatively, never to be
    consumed; position tl of a live row is overwritten by the append)."""
    rng = np.random.RandomState(seed)
    rows, step = batch * K, tl + 1
    ft = np.float32 if fp32 else np.float16
    ut = np.uint32 if fp32 else np.uint16
    rnd = _single if fp32 else _half
    lens = np.asarray(lens, dtype=np.int32)
    assert len(lens) == batch and int(lens.max()) <= max_input_len and tl < s_max
    kc = _nan_bits(rng, (rows, nh, s_max, dh), fp32)
    vc = _nan_bits(rng, (rows, nh, s_max, dh), fp32)
    kc[:, :, :tl] = rnd(rng.randn(rows, nh, tl, dh)).view(ut)
    vc[:, :, :tl] = rnd(rng.randn(rows, nh, tl, dh)).view(ut)
    pad = np.repeat(max_input_len - lens, K).astype(np.int32)
    masked = np.zeros((rows, s_max), dtype=np.uint8)
    for b in range(rows):
        masked[b, lens[b // K]:max_input_len] = 1
    fin = np.zeros(rows, dtype=np.uint8)
    fin[list(finished)] = 1
    return dict(dh=dh, rot=rot, nh=nh, batch=batch, K=K, rows=rows, s_max=s_max, max_input_len=max_input_len, tl=tl, step=step,
                fp32=fp32, ft=ft, ut=ut,
                qkv=rnd(rng.randn(rows, 3, nh, dh)), bias=rnd(0.1 * rng.randn(3, nh, dh)), kc=kc, vc=vc,
                seq_len=np.full(rows, tl, dtype=np.int32), pad=pad, masked=masked, fin=fin,
                indir=fill_indirection(rng, rows, K, s_max, max_input_len, (step - max_input_len) & 1),
                ctx0=(_sentinel(rng, rows * nh * dh).reshape(rows, nh, dh).astype(ut)))


def beam_reference(c, indir="own"):
    """reference_beam_step on a case of beam_case (indir: another indirection, None: none at all)"""
    ind = c["indir"] if isinstance(indir, str) else indir
    return reference_beam_step(c["qkv"], c["bias"], c["kc"].view(c["ft"]), c["vc"].view(c["ft"]), ind, c["K"], c["max_input_len"],
                               c["seq_len"], c["pad"], c["masked"], c["fin"], c["nh"], c["dh"], c["rot"], c["step"], fp32=c["fp32"])


# the head sizes of the decode attention with the rotary widths tests/test_gpu_kernels.py runs them at
HEAD_SIZES = [(32, 32), (48, 16), (64, 16), (80, 80), (96, 24), (128, 32), (144, 64), (160, 32), (192, 192), (224, 56), (256, 128)]

# name -> (beam_case arguments, split counts; 0: the launcher's own choice).  The smallest shapes that reach each form of the
# kernel: the all-in-registers form holds while roundup16(ceil(s_max / nsplit)) <= 2048 / LPK (LPK 4 / 8 / 16 / 32 lanes per key
# at dh <= 32 / <= 64 / <= 128 / > 128), the looped form beyond.
_A = dict(dh=128, rot=32, nh=2, batch=2, K=3, s_max=384, max_input_len=180, lens=(180, 143), tl=340, finished=(4,))
BEAM_CASES = {
    # registers; generated keys in splits 1..3; a ragged mask; b_first = 3; row 4 finished and still a parent of others
    "A1": (dict(_A, seed=1), (4,)),
    "A2": (dict(_A, tl=341, seed=2), (4,)),  # the other plane parity
    "B": (dict(_A, seed=3), (1,)),  # looped, chunk 384
    "C": (dict(_A, seed=4), (2,)),  # looped, two splits
    "D": (dict(_A, max_input_len=60, lens=(60, 23), tl=100, seed=5), (4,)),  # splits 2, 3 empty; the current token in split 1
    "E": (dict(_A, lens=(180, 180), tl=180, seed=6), (4, 1)),  # no generated key: every beam reads beam 0's row
    "F0": (dict(dh=64, rot=16, nh=2, batch=1, K=3, s_max=64, max_input_len=1, lens=(1,), tl=0, seed=7), (1,)),  # no cached key
    "F1": (dict(dh=64, rot=16, nh=2, batch=1, K=3, s_max=64, max_input_len=1, lens=(1,), tl=1, seed=8), (1,)),
    "F2": (dict(dh=64, rot=16, nh=2, batch=1, K=3, s_max=64, max_input_len=1, lens=(1,), tl=2, seed=9), (1,)),
    # many rows; the split count the launcher picks itself (PICKED_SPLITS, asserted by the GPU test)
    "G2x33": (dict(dh=64, rot=16, nh=1, batch=2, K=33, s_max=160, max_input_len=40, lens=(40, 40), tl=150, seed=10), (0,)),
    "G1x64": (dict(dh=64, rot=16, nh=1, batch=1, K=64, s_max=160, max_input_len=40, lens=(40,), tl=150, seed=11), (0,)),
    # looped with 16 splits
    "J": (dict(dh=256, rot=128, nh=1, batch=1, K=3, s_max=2100, max_input_len=1500, lens=(1500,), tl=2050, seed=12), (16,)),
}
for _dh, _rot in HEAD_SIZES:  # every head size looped (1) and in registers (16)
    BEAM_CASES[f"H{_dh}"] = (dict(dh=_dh, rot=_rot, nh=2, batch=1, K=3, s_max=640, max_input_len=300, lens=(300,), tl=600,
                                  seed=100 + _dh), (1, 16))
PICKED_SPLITS = 3  # of both G cases: min(ceil(640 / (rows x heads)), ceil(s_max / 64), 16)
FP32_CASES = ["A1", "E", "F0", "F1", "F2", "G2x33", "H80", "H256"]


def in_registers(dh, s_max, nsplit):
    """whether a launch of nsplit splits takes the all-in-registers form"""
    lpk = 4 if dh <= 32 else 8 if dh <= 64 else 16 if dh <= 128 else 32
    return (((s_max + nsplit - 1) // nsplit) + 15) // 16 * 16 <= 2048 // lpk
