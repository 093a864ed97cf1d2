"""-m gpu: the continuous batcher's paged K/V kernels at kernel level (include/ftcf.h ftcf_paged_attention,
ftcf_scatter_kv_to_pages, ftcf_gather_pages_to_kv) against a plain float64 numpy reference of one paged decode step.

The reference keeps the kernel's rounding points and nothing else: q, k, v = half(qkv + bias); NeoX rotary at position len[b]
with the angle in fp32 (pos / 10000^(2j/rot)), cos / sin and the rotation in float64, the rotated q and k rounded to half; scores,
soft-max (with the +1e-6 of the normaliser) and P.V in float64; the context rounded to half once.  Keys are gathered through
each slot's page table here in numpy.  Pools start as a sentinel pattern, so a write anywhere but the appended rows shows."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.attention_reference import CTX_FLOOR, CTX_ULPS, K_ULPS, _half, _rotary, _sentinel, _ulps
from tests.helpers import PAGED_LDS as LDS
from tests.helpers import longest_paged_len as longest
from tests.helpers import paged_smem_bytes as smem_bytes

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


def reference_step(qkv, bias, kpool, vpool, pt, lens, fin, nh, dh, rot, P):
    """One paged decode step in float64.  qkv [B, 3, nh, dh] fp16, bias [3, nh, dh] fp16, pools [pages, nh, P, dh] fp16.
    Returns ctx, k_new, v_new [B, nh, dh] fp16 (finished slots: None) and, for each of ctx and k_new, the magnitude of the terms
    that make it (sum_t p_t |v_t| / sum_t p_t; |a| + |b| of a rotated pair): the scale at which its error is measured."""
    B = len(lens)
    x = _half(qkv.astype(np.float64) + bias.astype(np.float64)[None])
    ctx, k_new, v_new, c_mag, k_mag = ([None] * B for _ in range(5))
    for b in range(B):
        if fin[b]:
            continue
        tl = int(lens[b])
        q = _rotary(x[b, 0], tl, rot)
        k = _rotary(x[b, 1], tl, rot)
        v = x[b, 2]
        t = np.arange(tl)
        keys = np.concatenate([kpool[pt[b, t // P], :, t % P, :].astype(np.float64), k[None].astype(np.float64)])  # [tl+1, nh, dh]
        vals = np.concatenate([vpool[pt[b, t // P], :, t % P, :].astype(np.float64), v[None].astype(np.float64)])
        s = np.einsum("thd,hd->ht", keys, q.astype(np.float64)) / np.sqrt(dh)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        den = (p.sum(axis=1) + 1e-6)[:, None]
        ctx[b], k_new[b], v_new[b] = _half(np.einsum("ht,thd->hd", p, vals) / den), k, v
        c_mag[b] = np.einsum("ht,thd->hd", p, np.abs(vals)) / den
        xk = np.abs(x[b, 1].astype(np.float64))
        k_mag[b] = xk.copy()
        k_mag[b][:, :rot // 2] = k_mag[b][:, rot // 2:rot] = xk[:, :rot // 2] + xk[:, rot // 2:rot]
    return ctx, k_new, v_new, c_mag, k_mag


def _layout(rng, lens, P, share, extra):
    """Page tables for slots of the given lengths (each holds ceil((len + 1) / P) pages: the appended token's page included),
    drawn from a random permutation of a pool `extra` pages larger than needed.  share: slots 0 and 1 share their first
    min(len0, len1) // P pages (read-only: both append further on).  Unused table entries point at a trap page nobody owns.
    -> (page_table [B, max_pages], num_pages, trap page)."""
    need = [(int(n) + 1 + P - 1) // P for n in lens]
    k = min(lens[0], lens[1]) // P if share else 0
    num_pages = sum(need) - k + 1 + extra
    perm = rng.permutation(num_pages)
    trap, free = int(perm[0]), list(perm[1:])
    max_pages = max(need)
    pt = np.full((len(lens), max_pages), trap, dtype=np.int32)
    for b, n in enumerate(need):
        for i in range(n):
            pt[b, i] = pt[0, i] if (b == 1 and i < k) else free.pop()
    return pt, num_pages, trap


def _run(qkv, bias, kpool, vpool, pt, lens, fin, nh, dh, rot, P, max_len, ctx):
    B, max_pages = pt.shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keep = [d(qkv.view(np.int16)).view(torch.float16), d(bias.view(np.int16)).view(torch.float16), d(pt), d(lens.astype(np.int32)),
            d(fin.astype(np.uint8))]
    capi.check(capi.lib().ftcf_paged_attention(
        capi.vp(keep[0]), capi.vp(keep[1]), capi.vp(kpool), capi.vp(vpool), capi.vp(keep[2]), capi.vp(keep[3]), capi.vp(keep[4]),
        B, nh, dh, rot, P, max_pages, max_len, capi.vp(ctx), sp()))
    torch.cuda.synchronize()


def _case(dh, rot, P, nh, lens, max_len=None, seed=0, share=True, fin_len=None, plant=False):
    """Runs one launch (twice) and checks it against reference_step.  plant: in every live slot of two or more cached keys, the
    last cached key and the first key of a page halfway through are made to score ln(len) against the slot's rotated q (each
    then weighs about a quarter of the soft-max at any length): a kernel that drops or misplaces either one is off by far more
    than the bound, however long the context."""
    rng = np.random.RandomState(seed)
    lens = [int(n) for n in lens]
    fin = [0] * len(lens)
    if fin_len is not None:  # a finished slot with cached pages of its own
        lens.append(fin_len)
        fin.append(1)
    lens, fin = np.array(lens, dtype=np.int32), np.array(fin, dtype=np.uint8)
    B = len(lens)
    pt, num_pages, trap = _layout(rng, lens, P, share, extra=max(3, len(lens)))
    if max_len is None:
        max_len = pt.shape[1] * P
    assert smem_bytes(dh, pt.shape[1], max_len) <= LDS and int(lens.max()) < max_len
    # pools: sentinel everywhere, then the cached rows of every slot (shared pages written once, by slot 0)
    kb = _sentinel(rng, num_pages * nh * P * dh).reshape(num_pages, nh, P, dh)
    vb = _sentinel(rng, num_pages * nh * P * dh).reshape(num_pages, nh, P, dh)
    for b in range(B):
        for t0 in range(0, int(lens[b]), P):
            n = min(P, int(lens[b]) - t0)
            pg = pt[b, t0 // P]
            if b == 1 and share and t0 + P <= min(lens[0], lens[1]):
                continue
            kb[pg, :, :n] = _half(rng.randn(nh, n, dh)).view(np.uint16)
            vb[pg, :, :n] = _half(rng.randn(nh, n, dh)).view(np.uint16)
    qkv = _half(rng.randn(B, 3, nh, dh))
    bias = _half(0.1 * rng.randn(3, nh, dh))
    ctx_s = _sentinel(rng, B * nh * dh).reshape(B, nh, dh)
    if plant:
        x = _half(qkv.astype(np.float64) + bias.astype(np.float64)[None])
        for b in range(B):
            tl = int(lens[b])
            if fin[b] or tl < 2:
                continue
            q = _rotary(x[b, 0], tl, rot).astype(np.float64)  # [nh, dh]
            k = _half(q * (np.log(tl) * np.sqrt(dh) / (q * q).sum(axis=1, keepdims=True)))
            for t in (tl - 1, P * ((tl - 1) // P // 2)):
                kb[pt[b, t // P], :, t % P] = k.view(np.uint16)
    ref, k_new, v_new, c_mag, k_mag = reference_step(qkv, bias, kb.view(np.float16), vb.view(np.float16), pt, lens, fin, nh, dh, rot, P)

    dev = lambda a: torch.from_numpy(a.view(np.int16).copy()).cuda()
    Kp, Vp, ctx = dev(kb), dev(vb), dev(ctx_s)
    _run(qkv, bias, Kp, Vp, pt, lens, fin, nh, dh, rot, P, max_len, ctx)
    ka, va, ca = (t.cpu().numpy().view(np.uint16) for t in (Kp, Vp, ctx))

    ek, ev = kb.copy(), vb.copy()  # what the pools must hold now: the sentinel / cached rows + one appended row per live slot
    worst_c = worst_k = 0.0
    at_c = at_k = None
    per_slot = {}  # len -> worst ctx error of that slot
    for b in range(B):
        if fin[b]:
            assert np.array_equal(ca[b], ctx_s[b]), ("finished slot's ctx written", b)
            continue
        tl = int(lens[b])
        pg, r = pt[b, tl // P], tl % P
        ec = _ulps(ca[b].view(np.float16), ref[b], CTX_FLOOR * c_mag[b])
        ek_ = _ulps(ka[pg, :, r].view(np.float16), k_new[b], k_mag[b])
        per_slot[tl] = max(per_slot.get(tl, 0.0), float(ec.max()))
        if ec.max() > worst_c:
            worst_c, at_c = float(ec.max()), (b, tl, np.unravel_index(int(ec.argmax()), ec.shape))
        if ek_.max() > worst_k:
            worst_k, at_k = float(ek_.max()), (b, tl)
        assert np.array_equal(va[pg, :, r], v_new[b].view(np.uint16)), ("appended v not bit exact", b, tl)
        ek[pg, :, r] = ka[pg, :, r]
        ev[pg, :, r] = va[pg, :, r]
    slots = "" if B > 6 else " (by length: " + ", ".join(f"{n}: {e:.2f}" for n, e in sorted(per_slot.items())) + ")"
    print(f"[dh {dh} rot {rot} P {P} nh {nh}: ctx {worst_c:.2f} ulp{slots}, k {worst_k:.2f} ulp] ", end="")
    assert worst_c <= CTX_ULPS, ("ctx (slot, len, (head, dim))", worst_c, at_c)
    assert worst_k <= K_ULPS, ("appended k (slot, len)", worst_k, at_k)
    for name, got, want in (("k_pool", ka, ek), ("v_pool", va, ev)):
        bad = np.argwhere(got != want)
        assert bad.size == 0, (name, "stray writes (page, head, row, dim)", bad[:8].tolist())
    # a second launch over what the first one left: the same bits
    _run(qkv, bias, Kp, Vp, pt, lens, fin, nh, dh, rot, P, max_len, ctx)
    assert np.array_equal(ctx.cpu().numpy().view(np.uint16), ca)
    assert np.array_equal(Kp.cpu().numpy().view(np.uint16), ka) and np.array_equal(Vp.cpu().numpy().view(np.uint16), va)


def _edges(dh, P):
    S = 16 if dh == 128 else 32  # keys per iteration of the score loop (4 waves x 64 / (dh / 8) lanes per key)
    return [P + 1, 2 * P + 3, 0, 1, P - 1, P, S - 1, S, S + 1]


# every page size at both head sizes, the rotary width cycling through none / partial / all: the short edges in one launch
_SHORT = [(128, 128, 8), (128, 0, 16), (128, 32, 24), (128, 128, 48), (128, 32, 64), (128, 0, 256),
          (64, 64, 8), (64, 16, 16), (64, 0, 24), (64, 16, 48), (64, 64, 64), (64, 16, 256)]


@pytest.mark.parametrize("dh,rot,P", _SHORT)
def test_paged_attention_at_page_and_loop_edges(dh, rot, P):
    """Lengths 0, 1, P - 1, P, P + 1, the score loop's stride and its neighbours, mixed in one launch; two slots sharing their
    first page(s); one finished slot."""
    _case(dh, rot, P, 5, _edges(dh, P), seed=P + dh + rot, fin_len=P + 3)


@pytest.mark.parametrize("dh,rot,P,lens", [(128, 32, 24, [4096, 1003, 5]), (128, 0, 256, [1000, 4096, 300]),
                                           (64, 64, 48, [4096, 997, 33]), (64, 16, 8, [1001, 4096, 64])])
def test_paged_attention_at_long_contexts(dh, rot, P, lens):
    _case(dh, rot, P, 3, lens, seed=len(lens) + P, fin_len=2 * P, plant=True)


@pytest.mark.parametrize("dh,rot,P", [(128, 128, 16), (128, 32, 48), (64, 16, 24), (64, 64, 256)])
def test_paged_attention_at_the_longest_length_the_batcher_accepts(dh, rot, P):
    """len = max_len - 1, max_len the batcher's limit for (dh, P) (~14,700 tokens at dh 128 with 16-token pages): the score array
    fills the LDS the launcher grants it."""
    L = longest(dh, P)
    assert smem_bytes(dh, L // P + 1, L + P) > LDS  # one page more is refused by the batcher
    _case(dh, rot, P, 2, [L - 1, L // 2 + 7], max_len=L, seed=L, plant=True)


@pytest.mark.parametrize("dh,rot,P", [(128, 32, 16), (64, 16, 24)])
def test_paged_attention_with_many_slots_and_heads(dh, rot, P):
    """64 slots of random lengths up to 200 and 40 heads in one launch."""
    rng = np.random.RandomState(dh + P)
    lens = rng.randint(0, 201, size=63).tolist()
    _case(dh, rot, P, 40, lens, seed=dh * P, fin_len=17)


def test_paged_attention_reads_and_writes_pages_above_2_to_the_31_elements():
    """A pool of 8200 pages of nh 8 x P 256 x dh 128 (2.15e9 elements, 4.3 GB per pool): slot 0 lives in pages 8192..8199, whose
    offsets are all >= 2^31 elements (64-bit page offsets); slot 1 in low pages.  Pages nobody owns are checked on the device."""
    nh, dh, P, rot, num_pages = 8, 128, 256, 32, 8200
    page = nh * P * dh
    assert 8192 * page == 2 ** 31
    rng = np.random.RandomState(31)
    lens = np.array([1900, 300], dtype=np.int32)
    fin = np.zeros(2, dtype=np.uint8)
    hi = 8192 + rng.permutation(8)
    lo = np.array([5, 3], dtype=np.int32)
    pt = np.stack([hi, np.concatenate([lo, [4] * 6])]).astype(np.int32)  # (slot 1's unused entries: a page nobody writes)
    used = sorted(set(hi.tolist()) | {5, 3})
    S = 0x2A5A  # sentinel (a finite half)
    Kp = torch.full((num_pages, nh, P, dh), S, dtype=torch.int16, device="cuda")
    Vp = torch.full((num_pages, nh, P, dh), S, dtype=torch.int16, device="cuda")
    kb = np.full((len(used), nh, P, dh), S, dtype=np.uint16)  # host copies of the used pages
    vb = kb.copy()
    pos = {pg: i for i, pg in enumerate(used)}
    for b in range(2):
        for t0 in range(0, int(lens[b]), P):
            n = min(P, int(lens[b]) - t0)
            i = pos[int(pt[b, t0 // P])]
            kb[i, :, :n] = _half(rng.randn(nh, n, dh)).view(np.uint16)
            vb[i, :, :n] = _half(rng.randn(nh, n, dh)).view(np.uint16)
    idx = torch.tensor(used, dtype=torch.long, device="cuda")
    Kp[idx] = torch.from_numpy(kb.view(np.int16)).cuda()
    Vp[idx] = torch.from_numpy(vb.view(np.int16)).cuda()
    qkv = _half(rng.randn(2, 3, nh, dh))
    bias = _half(0.1 * rng.randn(3, nh, dh))
    # the reference sees the used pages under their own ids (a sparse view of the pool)
    remap = np.vectorize(lambda g: pos.get(int(g), 0))(pt).astype(np.int32)
    ref, k_new, v_new, c_mag, k_mag = reference_step(qkv, bias, kb.view(np.float16), vb.view(np.float16), remap, lens, fin, nh, dh, rot, P)
    ctx = torch.zeros((2, nh, dh), dtype=torch.int16, device="cuda")
    _run(qkv, bias, Kp, Vp, pt, lens, fin, nh, dh, rot, P, pt.shape[1] * P, ctx)
    ca = ctx.cpu().numpy().view(np.uint16)
    ka, va = Kp[idx].cpu().numpy().view(np.uint16), Vp[idx].cpu().numpy().view(np.uint16)
    for b in range(2):
        tl = int(lens[b])
        i, r = pos[int(pt[b, tl // P])], tl % P
        e = _ulps(ca[b].view(np.float16), ref[b], CTX_FLOOR * c_mag[b])
        e_k = _ulps(ka[i, :, r].view(np.float16), k_new[b], k_mag[b])
        print(f"[pages above 2^31, slot {b} len {tl}: ctx {e.max():.2f} ulp, k {e_k.max():.2f} ulp] ", end="")
        assert e.max() <= CTX_ULPS, ("ctx", b, float(e.max()))
        assert e_k.max() <= K_ULPS, ("appended k", b)
        assert np.array_equal(va[i, :, r], v_new[b].view(np.uint16)), ("appended v", b)
        kb[i, :, r], vb[i, :, r] = ka[i, :, r], va[i, :, r]
    assert np.array_equal(ka, kb) and np.array_equal(va, vb), "stray writes inside the used pages"
    mask = torch.ones(num_pages, dtype=torch.bool, device="cuda")
    mask[idx] = False
    for pool in (Kp, Vp):
        for p0 in range(0, num_pages, 1024):  # pages nobody owns still hold the sentinel (in slices: no 2e9-element temporary)
            ch = pool[p0:p0 + 1024].view(min(1024, num_pages - p0), -1)
            dirty = ch.ne(S).any(dim=1) & mask[p0:p0 + 1024]
            assert not bool(dirty.any()), ("stray write in pages", (torch.nonzero(dirty).flatten() + p0).tolist()[:8])
    del Kp, Vp
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dh,rot,P,lens,s_max", [
    (128, 32, 8, [0, 1, 15, 16, 17, 95], 96),    # dense: all in registers (<= 128 keys)
    (128, 32, 8, [127, 128, 129, 300], 304),     # dense: the looped form
    (128, 32, 8, [600], 608),                    # ... past one 512-key step of its two rounds in flight
    (64, 16, 24, [0, 31, 32, 33, 255], 256),     # dense: all in registers (<= 256 keys)
    (64, 16, 24, [257, 700], 704)])              # dense: the looped form
def test_paged_attention_equals_dense_attention_bit_for_bit(dh, rot, P, lens, s_max):
    """One launch of ftcf_paged_attention and one of ftcf_masked_multihead_attention_beams (fp16, no indirection, one split, no
    mask) over the same keys and values: both are mmha_partial, so ctx and the appended K / V rows are identical bits and neither
    cache changes anywhere else.  Pages are permuted, unused table entries name a trap page; the dense cache [B, nh, s_max, dh]
    holds exactly the rows the pages hold and a sentinel elsewhere; pad_count puts the dense row's rotary position at len[b]."""
    nh = 2
    rng = np.random.RandomState(dh + s_max)
    lens = np.array(lens, dtype=np.int32)
    B = len(lens)
    fin = np.zeros(B, dtype=np.uint8)
    pt, num_pages, trap = _layout(rng, lens, P, False, extra=3)
    max_len = pt.shape[1] * P
    assert smem_bytes(dh, pt.shape[1], max_len) <= LDS and int(lens.max()) < min(max_len, s_max)
    kb = _sentinel(rng, num_pages * nh * P * dh).reshape(num_pages, nh, P, dh)
    vb = _sentinel(rng, num_pages * nh * P * dh).reshape(num_pages, nh, P, dh)
    kd = _sentinel(rng, B * nh * s_max * dh).reshape(B, nh, s_max, dh)
    vd = _sentinel(rng, B * nh * s_max * dh).reshape(B, nh, s_max, dh)
    for b in range(B):
        n = int(lens[b])
        t = np.arange(n)
        kd[b, :, :n] = _half(rng.randn(nh, n, dh)).view(np.uint16)
        vd[b, :, :n] = _half(rng.randn(nh, n, dh)).view(np.uint16)
        kb[pt[b, t // P], :, t % P] = kd[b, :, :n].transpose(1, 0, 2)
        vb[pt[b, t // P], :, t % P] = vd[b, :, :n].transpose(1, 0, 2)
    qkv = _half(rng.randn(B, 3, nh, dh))
    bias = _half(0.1 * rng.randn(3, nh, dh))
    ctx0 = _sentinel(rng, B * nh * dh).reshape(B, nh, dh)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).cuda()

    Kp, Vp, ctx_p = dev(kb), dev(vb), dev(ctx0)
    _run(qkv, bias, Kp, Vp, pt, lens, fin, nh, dh, rot, P, max_len, ctx_p)

    Kd, Vd, ctx_d = dev(kd), dev(vd), dev(ctx0)
    step = s_max + 1
    keep = [dev(qkv), dev(bias), torch.from_numpy(lens).cuda(), torch.from_numpy((step - 1 - lens).astype(np.int32)).cuda(),
            torch.from_numpy(fin).cuda()]
    wsb = B * nh * (dh + 2) * 8
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    capi.check(capi.lib().ftcf_masked_multihead_attention_beams(
        capi.FP16, capi.vp(keep[0]), capi.vp(keep[1]), capi.vp(Kd), capi.vp(Vd), capi.vp(keep[2]), capi.vp(keep[3]), capi.vp(None),
        capi.vp(keep[4]), capi.vp(None), 1, 0, B, nh, dh, rot, s_max, step, 1, capi.vp(ctx_d), capi.vp(ws), C.c_size_t(wsb), sp()))
    torch.cuda.synchronize()

    u16 = lambda t: t.cpu().numpy().view(np.uint16)
    cp, kp, vp, cd, kda, vda = (u16(t) for t in (ctx_p, Kp, Vp, ctx_d, Kd, Vd))
    assert np.array_equal(cp, cd), ("ctx differs (slot, head, dim)", np.argwhere(cp != cd)[:8].tolist())
    assert (cp != ctx0).any(axis=2).all(), "a (slot, head) whose ctx was not written"
    for b in range(B):
        n = int(lens[b])
        pg, r = pt[b, n // P], n % P
        assert np.array_equal(kp[pg, :, r], kda[b, :, n]), ("appended k differs", b, n)
        assert np.array_equal(vp[pg, :, r], vda[b, :, n]), ("appended v differs", b, n)
        kb[pg, :, r], vb[pg, :, r] = kp[pg, :, r], vp[pg, :, r]  # what the caches must hold now: one appended row per slot
        kd[b, :, n], vd[b, :, n] = kda[b, :, n], vda[b, :, n]
    for name, got, want in (("k_pool", kp, kb), ("v_pool", vp, vb), ("k_cache", kda, kd), ("v_cache", vda, vd)):
        bad = np.argwhere(got != want)
        assert bad.size == 0, (name, "stray writes", bad[:8].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# scatter (a prompt's dense K/V -> its pages) and gather (the prefix cache: pages -> the dense cache), bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _scatter(kc, vc, Kp, Vp, pages, L, nh, dh, s_max, S, P, pool_layer, row_layer):
    return capi.lib().ftcf_scatter_kv_to_pages(capi.vp(kc), capi.vp(vc), capi.vp(Kp), capi.vp(Vp), capi.vp(pages), L, nh, dh, s_max, S,
                                               P, C.c_size_t(pool_layer), C.c_size_t(row_layer), sp())


def _gather(kc, vc, Kp, Vp, pages, L, nh, dh, s_max, T, P, pool_layer, row_layer):
    return capi.lib().ftcf_gather_pages_to_kv(capi.vp(kc), capi.vp(vc), capi.vp(Kp), capi.vp(Vp), capi.vp(pages), L, nh, dh, s_max, T,
                                              P, C.c_size_t(pool_layer), C.c_size_t(row_layer), sp())


@pytest.mark.parametrize("L,nh,dh,P,s_max,S,row", [(1, 3, 128, 8, 100, 77, 1), (2, 5, 64, 24, 130, 101, 2), (3, 2, 128, 48, 200, 193, 1),
                                                   (3, 4, 64, 16, 64, 63, 2), (2, 2, 128, 256, 600, 513, 1)])
def test_scatter_and_gather_are_exact_inverses(L, nh, dh, P, s_max, S, row):
    """A 3-row, L-layer dense cache, row != 0, permuted pages: scatter of S tokens (S % P != 0) is numpy indexing bit for bit and
    writes nothing past token S - 1; gather of the whole pages [0, T) into another row returns them bit for bit and changes nothing
    else, in the pool or in the cache; a T that is not a multiple of P is refused and the library stays usable."""
    assert S % P != 0 and S <= s_max
    rng = np.random.RandomState(L * 100 + S)
    rows = 3
    npg = (S + P - 1) // P
    num_pages = npg + 5
    pages = rng.permutation(num_pages)[:npg].astype(np.int32)
    src = _sentinel(rng, L * rows * nh * s_max * dh).reshape(L, rows, nh, s_max, dh)
    srv = _sentinel(rng, src.size).reshape(src.shape)
    pk = _sentinel(rng, L * num_pages * nh * P * dh).reshape(L, num_pages, nh, P, dh)
    pv = _sentinel(rng, pk.size).reshape(pk.shape)
    dev = lambda a: torch.from_numpy(a.view(np.int16).copy()).cuda()
    Kc, Vc, Kp, Vp, Pg = dev(src), dev(srv), dev(pk), dev(pv), torch.from_numpy(pages).cuda()
    pool_layer, row_layer = num_pages * nh * P * dh, rows * nh * s_max * dh
    capi.check(_scatter(Kc[0, row], Vc[0, row], Kp, Vp, Pg, L, nh, dh, s_max, S, P, pool_layer, row_layer))
    torch.cuda.synchronize()
    ek, ev = pk.copy(), pv.copy()
    t = np.arange(S)
    for l in range(L):
        ek[l, pages[t // P], :, t % P] = src[l, row, :, :S].transpose(1, 0, 2)
        ev[l, pages[t // P], :, t % P] = srv[l, row, :, :S].transpose(1, 0, 2)
    assert np.array_equal(Kp.cpu().numpy().view(np.uint16), ek) and np.array_equal(Vp.cpu().numpy().view(np.uint16), ev)
    assert np.array_equal(Kc.cpu().numpy().view(np.uint16), src) and np.array_equal(Vc.cpu().numpy().view(np.uint16), srv)

    # gather the whole pages back into another row of a second cache full of sentinels
    T = (S // P) * P
    dst_r = (row + 1) % rows
    dk = _sentinel(rng, src.size).reshape(src.shape)
    dv = _sentinel(rng, src.size).reshape(src.shape)
    Dk, Dv = dev(dk), dev(dv)
    capi.check(_gather(Dk[0, dst_r], Dv[0, dst_r], Kp, Vp, Pg, L, nh, dh, s_max, T, P, pool_layer, row_layer))
    torch.cuda.synchronize()
    wk, wv = dk.copy(), dv.copy()
    wk[:, dst_r, :, :T] = src[:, row, :, :T]
    wv[:, dst_r, :, :T] = srv[:, row, :, :T]
    assert np.array_equal(Dk.cpu().numpy().view(np.uint16), wk) and np.array_equal(Dv.cpu().numpy().view(np.uint16), wv)
    assert np.array_equal(Kp.cpu().numpy().view(np.uint16), ek) and np.array_equal(Vp.cpu().numpy().view(np.uint16), ev)

    # refused: T not a multiple of P, T past s_max; nothing written, and the next call works
    for bad_t in (T + 1, s_max + P):
        code = _gather(Dk[0, 0], Dv[0, 0], Kp, Vp, Pg, L, nh, dh, s_max, bad_t, P, pool_layer, row_layer)
        assert code != 0 and b"gather_pages_to_kv" in capi.lib().ftcf_last_error(), (bad_t, code)
    torch.cuda.synchronize()
    assert np.array_equal(Dk.cpu().numpy().view(np.uint16), wk) and np.array_equal(Dv.cpu().numpy().view(np.uint16), wv)
    Dk.copy_(dev(dk))
    Dv.copy_(dev(dv))
    capi.check(_gather(Dk[0, dst_r], Dv[0, dst_r], Kp, Vp, Pg, L, nh, dh, s_max, T, P, pool_layer, row_layer))
    torch.cuda.synchronize()
    assert np.array_equal(Dk.cpu().numpy().view(np.uint16), wk) and np.array_equal(Dv.cpu().numpy().view(np.uint16), wv)
