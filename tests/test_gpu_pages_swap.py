"""-m gpu: the two kernels of the batcher's swap space alone, through the C ABI (ftcf_pages_pack / ftcf_pages_unpack,
csrc/kernels_attn.hip): whole pages of every layer of both pools <-> a contiguous staging buffer [n][2][L][page_elems].
fp16 pools with recognisable contents, scattered non-monotonic page lists and a single page, three geometries (fewer 16-byte
pieces per page and layer than one workgroup has threads; a count that is no multiple of 256; size_per_head 128).  Every
comparison is bit exact, on the uint16 view; everything that must not be written holds canaries."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
NUM_PAGES, STAGE_PAGES = 8, 4
GEOMETRIES = [(2, 2, 8, 64), (3, 3, 8, 64), (2, 2, 16, 128)]  # L, nh, P, dh: 128 / 192 / 512 pieces per page and layer
LISTS = [([5, 0, 3], [1, 6, 2]), ([4], [7])]
CANARY_STAGE, CANARY_POOL = 0xBEEF, 0xC0DE


@pytest.fixture(scope="module")
def capi():
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return capi


def _dev(a):
    return torch.from_numpy(a.view(np.int16)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint16)


def _pools(L, nh, P, dh):
    """[L][NUM_PAGES][nh][P][dh]: every element of K and of V names its place (two different odd multipliers mod 65521)"""
    n = L * NUM_PAGES * nh * P * dh
    i = np.arange(n, dtype=np.int64)
    shape = (L, NUM_PAGES, nh, P, dh)
    return ((i * 7 + 13) % 65521).astype(np.uint16).reshape(shape), ((i * 11 + 5) % 65521).astype(np.uint16).reshape(shape)


def _gather(K, V, pages):
    """the staging layout [n][2][L][page_elems] of a page list, in numpy"""
    L = K.shape[0]
    return np.stack([np.stack([np.stack([pool[l, pg].reshape(-1) for l in range(L)]) for pool in (K, V)]) for pg in pages])


@pytest.mark.parametrize("src,dst", LISTS)
@pytest.mark.parametrize("L,nh,P,dh", GEOMETRIES)
def test_pack_is_a_gather_and_unpack_its_inverse(capi, L, nh, P, dh, src, dst):
    lib = capi.lib()
    K, V = _pools(L, nh, P, dh)
    page_elems, n = nh * P * dh, len(src)
    layer_elems = C.c_size_t(NUM_PAGES * page_elems)
    dK, dV = _dev(K), _dev(V)
    stage = _dev(np.full((STAGE_PAGES, 2, L, page_elems), CANARY_STAGE, np.uint16))
    d_src, d_dst = torch.tensor(src, dtype=torch.int32).cuda(), torch.tensor(dst, dtype=torch.int32).cuda()
    capi.check(lib.ftcf_pages_pack(capi.vp(stage), capi.vp(dK), capi.vp(dV), capi.vp(d_src), n, L, nh, dh, P, layer_elems, None))
    torch.cuda.synchronize()
    got = _host(stage)
    np.testing.assert_array_equal(got[:n], _gather(K, V, src))
    assert (got[n:] == CANARY_STAGE).all()  # nothing beyond n pages
    np.testing.assert_array_equal(_host(dK), K)  # the pools are only read
    np.testing.assert_array_equal(_host(dV), V)
    # into another list of other pools: the target pages are the source pages, every other page keeps its canary
    tK, tV = (_dev(np.full(K.shape, CANARY_POOL, np.uint16)) for _ in range(2))
    capi.check(lib.ftcf_pages_unpack(capi.vp(stage), capi.vp(tK), capi.vp(tV), capi.vp(d_dst), n, L, nh, dh, P, layer_elems, None))
    torch.cuda.synchronize()
    for pool, ref in ((_host(tK), K), (_host(tV), V)):
        for s, d in zip(src, dst):
            np.testing.assert_array_equal(pool[:, d], ref[:, s])
        others = [pg for pg in range(NUM_PAGES) if pg not in dst]
        assert (pool[:, others] == CANARY_POOL).all()
    np.testing.assert_array_equal(_host(stage)[:n], _gather(K, V, src))  # the staging buffer is only read


def test_unpack_within_the_same_pools_and_no_pages(capi):
    """a swap in the batcher goes out of and back into ONE pair of pools: the pages of another list, nobody else's"""
    lib = capi.lib()
    L, nh, P, dh = 2, 2, 8, 64
    K, V = _pools(L, nh, P, dh)
    page_elems = nh * P * dh
    layer_elems = C.c_size_t(NUM_PAGES * page_elems)
    dK, dV = _dev(K), _dev(V)
    stage = _dev(np.full((STAGE_PAGES, 2, L, page_elems), CANARY_STAGE, np.uint16))
    src, dst = [6, 1], [0, 7]
    d_src, d_dst = torch.tensor(src, dtype=torch.int32).cuda(), torch.tensor(dst, dtype=torch.int32).cuda()
    capi.check(lib.ftcf_pages_pack(capi.vp(stage), capi.vp(dK), capi.vp(dV), capi.vp(d_src), 0, L, nh, dh, P, layer_elems, None))
    torch.cuda.synchronize()
    assert (_host(stage) == CANARY_STAGE).all()  # n = 0: nothing happens
    capi.check(lib.ftcf_pages_pack(capi.vp(stage), capi.vp(dK), capi.vp(dV), capi.vp(d_src), 2, L, nh, dh, P, layer_elems, None))
    capi.check(lib.ftcf_pages_unpack(capi.vp(stage), capi.vp(dK), capi.vp(dV), capi.vp(d_dst), 2, L, nh, dh, P, layer_elems, None))
    torch.cuda.synchronize()
    for pool, ref in ((_host(dK), K), (_host(dV), V)):
        want = ref.copy()
        want[:, 0], want[:, 7] = ref[:, 6], ref[:, 1]
        np.testing.assert_array_equal(pool, want)
    assert lib.ftcf_pages_pack(capi.vp(stage), capi.vp(dK), capi.vp(dV), capi.vp(d_src), 1, L, nh, 12, P, layer_elems, None) == -1  # dh % 8
