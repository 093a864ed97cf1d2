"""-m gpu: one rank of a tensor-parallel job at its REAL launch grid (all compute units, the default layout of the one- / two-row
persistent kernel's out-proj / FFN2 stage) against a TP = 1 model.  With fake peers (FTCF_FAKE_TP, a one-rank communicator)
the rank plays every peer with its own shard: its outputs are those of a TP = N job whose every rank holds shard `rank`, i.e.
of the TP = 1 model `_tile(shard)` whose every head group, FFN column block and vocabulary slice is a copy of that shard's.
The local-group emulation (test_gpu_fullsize.py, test_gpu_tp_local.py) gives a rank CUs / TP workgroups and at TP 8 leaves the
persistent kernel; this is the grid a rank runs on an N-GPU node."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

from tests.gpu_helpers import _close, _periodic, _run, _shard, _tile

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, OUT = 37, 5  # a prompt that is not a multiple of 16, a few tokens


@pytest.fixture(scope="module")
def model():
    """13B width (H 5120, 40 x 128 heads, inter 20480, V 100864, rotary 32, int8), 8 layers: the grid and the run tables
    depend on the width only.  Embedding and LM head repeat with period V / 8, so every vocabulary slice of TP 2 / 4 / 8 is
    the same and a token's copies feed the same next step."""
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    sys.path.insert(0, ROOT)
    import bench
    a = argparse.Namespace(layers=8, heads=40, head_dim=128, inter=20480, vocab=100864, rotary=32, dtype="int8")
    return _periodic((a,) + bench.synth_weights(a, 1, torch.device("cuda", 0)), 8)


def _op(a, w, q8, sc, group, tp, rank):
    from fastertransformer4codefuse_amd.gptneox_op import GptNeoXOp
    return GptNeoXOp(group, rank, a.heads, a.head_dim, a.inter, a.layers, a.vocab, a.rotary, 0, 2, tp, 1, 1, 2048, True,
                     w, q8, sc)


def _inputs(rows, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 100864, (rows, S), generator=g, dtype=torch.int32)
    lens = torch.tensor([S - 8 * (b % 2) - (b % 5) for b in range(rows)], dtype=torch.int32)  # ragged from two rows on
    for b in range(rows):
        ids[b, lens[b]:] = 0
    return ids.cuda(), lens.cuda()


def _check(model, monkeypatch, tp, rank, rows, env, path, layout):
    a = model[0]
    V, vl = a.vocab, a.vocab // tp
    ids, lens = _inputs(rows, 100 * tp + 10 * rows + rank)
    shard = _shard(model, tp, rank)
    ref = _op(*_tile((a,) + shard, tp, rank), None, 1, 0)  # TP = 1, default environment
    t1, l1 = _run(ref, ids, OUT, V, lens)
    del ref
    with monkeypatch.context() as m:
        m.setenv("FTCF_FAKE_TP", "1")
        for k, v in env.items():
            m.setenv(k, v)
        op = _op(a, *shard, object(), tp, rank)  # (any non-None group: the op only hands it to the communicator set-up)
        t, l = _run(op, ids, OUT, V, lens)
        t2, l2 = _run(op, ids, OUT, V, lens)
        st = op.stats()
        del op
    torch.cuda.empty_cache()
    what = f"tp{tp} rank{rank} rows{rows} {env}"
    assert st["decode_path"] == path, (what, st["decode_path"])
    if layout is not None:
        assert st["persist_layout"] == layout, (what, st["persist_layout"])
    assert np.array_equal(t, t2) and np.array_equal(l, l2), (what, "repeat not bit-identical")
    assert np.array_equal(t[:, :S], t1[:, :S]), what
    # a vocabulary slice's copies tie: the two models may pick different copies of one token
    _close(t1 % vl, l1, t % vl, l, S, 5e-3, what)


# the default layout of the out-proj / FFN2 stage on a rank's shard: own groups at TP 2 / 4, K pieces at TP 8
_DEFAULT_LAYOUT = {2: 1, 4: 1, 8: 0}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("rank_end", [0, 1], ids=["rank0", "last_rank"])
@pytest.mark.parametrize("rows", [1, 2], ids=["rows1", "rows2"])
@pytest.mark.parametrize("tp", [2, 4, 8], ids=["tp2", "tp4", "tp8"])
def test_fake_peer_rank_on_the_product_grid_follows_the_tiled_model(model, monkeypatch, tp, rows, rank_end):
    _check(model, monkeypatch, tp, rank_end * (tp - 1), rows, {}, 1, _DEFAULT_LAYOUT[tp])


@pytest.mark.timeout(600)
@pytest.mark.parametrize("own", [0, 1], ids=["kpieces", "own"])
@pytest.mark.parametrize("tp", [2, 4], ids=["tp2", "tp4"])
def test_fake_peer_rank_with_forced_layout_follows_the_tiled_model(model, monkeypatch, tp, own):
    """Both layouts of the out-proj / FFN2 stage on the product grid (the default picks the own groups at TP 2 / 4)."""
    _check(model, monkeypatch, tp, tp - 1, 1, {"FTCF_PERSIST_OWN": str(own)}, 1, own)


@pytest.mark.timeout(900)
def test_fake_peer_rank_tp8_bs16_follows_the_tiled_model(model, monkeypatch):
    """16 rows at TP 8: the general path, its per-layer all-reduces and the vocabulary-split LM head."""
    _check(model, monkeypatch, 8, 5, 16, {}, 2, None)
