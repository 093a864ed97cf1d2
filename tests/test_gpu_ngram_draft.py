"""-m gpu: speculative decoding's prompt-lookup drafting kernel (include/ftcf.h ftcf_ngram_draft) against a restatement of its
definition in Python."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

capi = None


@pytest.fixture(scope="module", autouse=True)
def _lib():
    global capi
    from fastertransformer4codefuse_amd import capi as _c
    capi = _c
    capi.require_gpu()
    yield


def draft_ref(t, K, N):
    """For g = min(N, n - 1) down to 1: the largest s <= n - g - 1 with t[s:s+g] == t[n-g:n]; the first g that has one wins."""
    n = len(t)
    for g in range(min(N, n - 1), 0, -1):
        for s in range(n - g - 1, -1, -1):
            if t[s:s + g] == t[n - g:n]:
                return t[s + g:min(s + g + K, n)]
    return []


def draft_gpu(t, K, N):
    tok = torch.tensor(t, dtype=torch.int32, device="cuda")
    out = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    capi.check(capi.lib().ftcf_ngram_draft(capi.vp(tok), len(t), K, N, capi.vp(out), capi.vp(cnt),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    n = int(cnt.item())
    o = out.cpu().tolist()
    assert 0 <= n <= K and all(v == -7 for v in o[n:]), (n, o)  # nothing written beyond the count
    return o[:n]


def test_random_sequences_on_a_small_alphabet():
    rng = np.random.RandomState(0)
    seen = set()
    for _ in range(3000):
        n = int(rng.choice([1, 2, 3, 5, 17, 64, 255, 256, 257, 700]))
        t = rng.randint(0, 4, size=n).tolist()
        K, N = int(rng.randint(1, 16)), int(rng.randint(1, 9))
        want = draft_ref(t, K, N)
        assert draft_gpu(t, K, N) == want, (t, K, N)
        seen.add(len(want))
    assert {0, 1, 2, 15} <= seen  # no match, short continuations and full drafts all occurred


def test_edges():
    assert draft_gpu([5], 4, 3) == []  # n = 1
    assert draft_gpu([1, 2, 3, 4], 4, 3) == []  # no match
    assert draft_gpu([7, 8, 9, 7], 4, 3) == [8, 9, 7]  # continuation shorter than K: cut at n
    assert draft_gpu([1, 2, 5, 1, 2, 6, 1, 2], 1, 2) == [6]  # several matches: the most recent one
    assert draft_gpu([1, 2, 5, 9, 2, 6, 1, 2], 2, 8) == [5, 9]  # the longest g wins over a more recent shorter match
    # g capped by N: with N = 1 only the last token is matched (-> its most recent earlier occurrence)
    assert draft_gpu([1, 2, 5, 9, 2, 6, 1, 2], 2, 1) == [6, 1]
    # a long history: the match sits beyond the first pass of the workgroup's 256 threads
    t = list(range(10, 610)) + [3, 4, 5] + list(range(700, 1000)) + [3, 4]
    assert draft_gpu(t, 5, 3) == [5, 700, 701, 702, 703]
    for bad in ((0, 3), (16, 3), (4, 0), (4, 9)):
        tok = torch.tensor([1, 2, 1], dtype=torch.int32, device="cuda")
        out = torch.zeros(16, dtype=torch.int32, device="cuda")
        assert capi.lib().ftcf_ngram_draft(capi.vp(tok), 3, bad[0], bad[1], capi.vp(out), capi.vp(out), None) != 0
