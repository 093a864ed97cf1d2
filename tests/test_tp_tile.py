"""CPU: the shard / tile construction behind tests/test_gpu_tp_product_grid.py.  `_tile(shard, tp, r)` must be a TP = 1 model
every rank-r' shard of which is rank r's shard again, bit for bit -- otherwise the TP = 1 reference of a fake-peer rank is
not the model that rank runs."""
import argparse

import pytest
import torch

import bench
from tests.gpu_helpers import _periodic, _shard, _tile


@pytest.fixture(scope="module")
def small():
    # the smallest widths whose TP 8 shards still cut whole int8 tiles (hl, il multiples of 64)
    a = argparse.Namespace(layers=2, heads=8, head_dim=64, inter=1024, vocab=96, rotary=32, dtype="int8")
    return _periodic((a,) + bench.synth_weights(a, 1, torch.device("cpu")), 8)


def _same(x, y, what):
    assert len(x) == len(y), what
    for i, (u, v) in enumerate(zip(x, y)):
        assert u.dtype == v.dtype and u.shape == v.shape and torch.equal(u, v), (what, i)


@pytest.mark.parametrize("tp", [2, 4, 8])
def test_shards_of_the_tiled_model_are_the_shard(small, tp):
    a = small[0]
    for r in sorted({0, 1, tp - 1}):
        shard = _shard(small, tp, r)
        tiled = _tile((a,) + shard, tp, r)
        for part, full in zip(tiled[1:], small[1:]):  # the tiled model has the TP = 1 model's sizes
            assert [t.numel() for t in part] == [t.numel() for t in full]
        for r2 in range(tp):
            for what, x, y in zip(("weights", "int8", "scales"), _shard(tiled, tp, r2), shard):
                _same(x, y, (tp, r, r2, what))


@pytest.mark.parametrize("tp", [2, 4, 8])
def test_tiled_model_repeats_the_shard(small, tp):
    """The tiled model is not the original: its other slices are copies of rank r's (a tiling that returned the input model
    unchanged would pass the round trip above for r = r' only)."""
    a = small[0]
    L, H, V = a.layers, a.heads * a.head_dim, a.vocab
    r = tp - 1
    _, w, q8, sc = _tile((a,) + _shard(small, tp, r), tp, r)
    hl = H // tp
    for l in range(L):
        qkv = small[1][3 * L + l].view(3, tp, hl)[:, r]
        assert torch.equal(w[3 * L + l].view(3, tp, hl), qkv[:, None].expand(3, tp, hl))
        assert torch.equal(w[9 * L + l], ((small[1][9 * L + l].float() / tp).half().float() * tp).half())
        out = small[2][L + l].view(H // 16, tp, hl // 64, 1024)[:, r]
        assert torch.equal(q8[L + l].view(H // 16, tp, hl // 64, 1024), out[:, None].expand(-1, tp, -1, -1))
        assert torch.equal(sc[L + l], small[3][L + l])
    lm = small[1][12 * L + 3].view(tp, V // tp, H)
    assert torch.equal(w[12 * L + 3].view(tp, V // tp, H), lm[r:r + 1].expand(tp, -1, -1))
