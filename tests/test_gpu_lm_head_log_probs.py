"""-m gpu: ftcf_lm_head_log_probs (csrc/kernels_logprob.hip), the fused LM head -> log-probability kernel behind
context_log_probs, against float64 log_softmax of the oracle's LM-head logits (ParallelGpt.cc:403-470 + logprob_kernels.cu:36-100
compute the same from written-out logits)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ATOL = 2e-3


@pytest.fixture(scope="module")
def torch_capi():
    import torch
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return torch, capi


def _inputs(m, n, k, seed):
    rng = np.random.RandomState(seed)
    A = rng.standard_normal((m, k)).astype(np.float16)
    A[::5] *= np.float16(4.0)  # some peaked rows
    W = (rng.standard_normal((n, k)) * 0.02).astype(np.float16)
    t = rng.randint(0, n, size=m).astype(np.int32)
    t[::7] = -1  # rows without a target give 0
    t[1 % m] = n - 1  # the last, partial column tile
    t[2 % m] = 0
    return A, W, t


def _run(torch, capi, A, W, t, lse=True):
    m, k = A.shape
    n = W.shape[0]
    dA, dW = torch.from_numpy(A).cuda(), torch.from_numpy(W).cuda()
    dt = torch.from_numpy(t).cuda()
    lp = torch.full((m,), float("nan"), dtype=torch.float32, device="cuda")
    ls = torch.full((m,), float("nan"), dtype=torch.float32, device="cuda") if lse else None
    capi.check(capi.lib().ftcf_lm_head_log_probs(capi.vp(dA), capi.vp(dW), capi.vp(dt), capi.vp(lp), capi.vp(ls), C.c_int(m),
                                                 C.c_int(n), C.c_int(k), C.c_void_p(None)))
    torch.cuda.synchronize()
    return lp.cpu().numpy(), (ls.cpu().numpy() if lse else None)


def _rows(m):
    if m <= 64:
        return np.arange(m)
    # the CPU reference of a 100864-column head is slow: every row of the first and last tiles, tile edges, a spread
    sel = set(range(0, 8)) | {63, 64, 65, m - 1, m - 2} | set(range(0, m, max(1, m // 32)))
    return np.array(sorted(r for r in sel if r < m))


def _check(A, W, t, lp, ls):
    sel = _rows(A.shape[0])
    logits = orc.lm_head(A[sel].astype(np.float32), W.astype(np.float32)).astype(np.float64)
    mx = logits.max(axis=1, keepdims=True)
    ref_lse = (mx + np.log(np.exp(logits - mx).sum(axis=1, keepdims=True)))[:, 0]
    ts = t[sel]
    ref = np.where(ts >= 0, logits[np.arange(len(sel)), np.maximum(ts, 0)] - ref_lse, 0.0)
    assert np.all(lp[sel][ts < 0] == 0.0)
    np.testing.assert_allclose(lp[sel], ref, atol=ATOL, rtol=0)
    np.testing.assert_allclose(ls[sel], ref_lse, atol=ATOL, rtol=1e-6)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(ls))


@pytest.mark.parametrize("m", [1, 16, 17, 256])
def test_13b_head_matches_float64_log_softmax(torch_capi, m):
    torch, capi = torch_capi
    A, W, t = _inputs(m, 100864, 5120, seed=m)
    lp, ls = _run(torch, capi, A, W, t)
    _check(A, W, t, lp, ls)


@pytest.mark.parametrize("m,n,k", [(1024, 8192, 5120), (70, 50280, 2560), (33, 1000, 256), (5, 517, 200)])
def test_other_shapes_match_float64_log_softmax(torch_capi, m, n, k):
    """Many m-blocks (1024 rows), an odd vocabulary (50280 = 392.8 column tiles), k not a multiple of the 128-wide k chunk."""
    torch, capi = torch_capi
    A, W, t = _inputs(m, n, k, seed=n + m)
    lp, ls = _run(torch, capi, A, W, t)
    _check(A, W, t, lp, ls)


def test_two_runs_are_bit_identical(torch_capi):
    torch, capi = torch_capi
    A, W, t = _inputs(300, 100864, 5120, seed=3)
    lp0, ls0 = _run(torch, capi, A, W, t)
    lp1, ls1 = _run(torch, capi, A, W, t)
    assert lp0.tobytes() == lp1.tobytes() and ls0.tobytes() == ls1.tobytes()
    lp2, _ = _run(torch, capi, A, W, t, lse=False)  # (row_logsumexp NULL)
    assert lp2.tobytes() == lp0.tobytes()
