"""-m gpu: the continuous batcher's prefix cache (ftcf_batcher_create_ex / ContinuousBatcher(..., prefix_cache=True)).

A request whose prompt starts with full page blocks an earlier admission has computed takes their pages, k_gather_pages_to_kv
copies them into the engine's cache and the prompt phase runs from the first uncached token.  The bar is that of the chunked
admission: every stream equals what the CPU oracle / the engine generates for the request alone (token exact on the tiny model,
up to near ties on the mid model), and the pool's pages are all accounted for (free list + cached pages)."""
import numpy as np
import pytest

from tests.helpers import load_tiny, random_model

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
MID = dict(head_num=8, size_per_head=64, inter_size=2048, num_layer=3, vocab_size=2048, rotary_dim=16, start_id=0, end_id=2)


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


@pytest.fixture(scope="module")
def tiny(gh):
    from oracle import oracle as orc
    from tests.helpers import weight_list_to_layers
    cfg, w, z = load_tiny()
    layers, glob = weight_list_to_layers(cfg, w)
    return cfg, w, z, orc.Model(dict(cfg, fp16=1), layers, glob), gh.make_op(cfg, w)


def _oracle(model, prompt, n_new, end_id, **kw):
    from tests.test_gpu_batcher import _oracle_alone
    return _oracle_alone(model, prompt, n_new, end_id, **kw)


def _run(cb, reqs, arrivals=None, **kw):
    """reqs: [(prompt, max_new)], submitted at the iterations of `arrivals` ({iteration: [index]}; default: one after the other,
    each once the previous has finished) -> ({index: tokens}, per-iteration lists of request indices)."""
    got, ids, per_step = {}, {}, []
    if arrivals is None:
        for k, (p, n) in enumerate(reqs):
            rid = cb.submit(p, n, **kw)
            for tok in cb.run_all()[rid]:
                got.setdefault(k, []).append(tok)
        return got, per_step
    pending, it = dict(arrivals), 0
    while pending or cb.busy():
        for k in pending.pop(it, []):
            ids[cb.submit(reqs[k][0], reqs[k][1], **kw)] = k
        evs = cb.step()
        per_step.append([ids[rid] for rid, _, _ in evs])
        for rid, tok, _ in evs:
            got.setdefault(ids[rid], []).append(tok)
        it += 1
        assert it < 5000
    return got, per_step


def _accounted(cb, num_pages):
    st, px = cb.status(), cb.prefix_stats()
    assert st["free_pages"] + px["cached_pages"] == num_pages, (st, px)
    cb.clear_prefix_cache()
    assert cb.status()["free_pages"] == num_pages and cb.prefix_stats()["cached_pages"] == 0


def test_a_shared_prefix_is_served_from_the_cache(gh, tiny):
    """B shares 19 tokens with the finished request A; 8-token pages: two blocks (16 tokens) come from the cache."""
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z, model, op = tiny
    V, end_id = cfg["vocab_size"], cfg["end_id"]
    rng = np.random.RandomState(31)
    a = rng.randint(3, V, size=26).tolist()
    b = a[:19] + rng.randint(3, V, size=7).tolist()
    cb = ContinuousBatcher(op, max_batch=2, page_tokens=8, num_pages=24, max_seq_len=64, prefix_cache=True)
    got_a, _ = _run(cb, [(a, 6)])
    s0 = cb.prefix_stats()
    assert s0["enabled"] == 1 and s0["hit_tokens"] == 0 and s0["cached_pages"] == 3 and s0["computed_tokens"] == len(a)
    got_b, _ = _run(cb, [(b, 9)])
    s1 = cb.prefix_stats()
    assert s1["hit_tokens"] - s0["hit_tokens"] == 16
    assert s1["computed_tokens"] - s0["computed_tokens"] == len(b) - 16
    assert s1["prompt_tokens"] - s0["prompt_tokens"] == len(b) and s1["lookups"] == 2
    assert got_a[0] == _oracle(model, a, 6, end_id, top_k=1)
    assert got_b[0] == _oracle(model, b, 9, end_id, top_k=1)
    _accounted(cb, 24)


@pytest.mark.parametrize("S", [24, 21])
def test_the_same_prompt_twice(gh, tiny, S):
    """The hit is floor((S - 1) / P) pages whether S is a multiple of P or not (the last prompt token is always computed)."""
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z, model, op = tiny
    V, end_id = cfg["vocab_size"], cfg["end_id"]
    p = np.random.RandomState(S).randint(3, V, size=S).tolist()
    cb = ContinuousBatcher(op, max_batch=2, page_tokens=8, num_pages=16, max_seq_len=48, prefix_cache=True)
    got, _ = _run(cb, [(p, 10), (p, 10)])
    st = cb.prefix_stats()
    assert st["hit_tokens"] == (S - 1) // 8 * 8 and st["computed_tokens"] == 2 * S - st["hit_tokens"]
    assert got[0] == got[1] == _oracle(model, p, 10, end_id, top_k=1)
    _accounted(cb, 16)


def test_a_system_prompt_shared_by_requests_arriving_over_time(gh, tiny):
    """Several requests with a common 20-token system prompt and private tails run at once on the shared pages."""
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z, model, op = tiny
    V, end_id = cfg["vocab_size"], cfg["end_id"]
    rng = np.random.RandomState(5)
    system = rng.randint(3, V, size=20).tolist()
    reqs = [(system + rng.randint(3, V, size=int(rng.randint(1, 12))).tolist(), int(rng.randint(3, 12))) for _ in range(8)]
    ref = [_oracle(model, p, n, end_id, top_k=1) for p, n in reqs]
    cb = ContinuousBatcher(op, max_batch=4, page_tokens=8, num_pages=40, max_seq_len=64, prefix_cache=True)
    got, _ = _run(cb, reqs, arrivals={0: [0], 2: [1], 3: [2, 3], 5: [4], 6: [5], 9: [6, 7]})
    for k in range(len(reqs)):
        assert got[k] == ref[k], (k, got[k], ref[k])
    st = cb.prefix_stats()
    assert st["hit_tokens"] >= 16 * 5 and st["lookups"] == len(reqs)
    _accounted(cb, 40)


def test_a_tight_pool_evicts_lru_leaves_and_never_a_pinned_page(gh, tiny):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z, model, op = tiny
    V, end_id = cfg["vocab_size"], cfg["end_id"]
    rng = np.random.RandomState(25)  # (every reference trajectory keeps a top-2 margin above 5e-3 of max|logit| in the oracle)
    x = rng.randint(3, V, size=17).tolist()
    y = x[:16] + rng.randint(3, V, size=9).tolist()
    zz = rng.randint(3, V, size=30).tolist()
    wv = rng.randint(3, V, size=40).tolist()
    cb = ContinuousBatcher(op, max_batch=2, page_tokens=8, num_pages=10, max_seq_len=64, prefix_cache=True)
    got = {}
    got["x"] = _run(cb, [(x, 3)])[0][0]  # caches x's 2 blocks
    # y takes x's two blocks (pinned) and 4 new pages; z needs 5 pages: 4 are free and nothing is evictable -> z waits for y
    ry = cb.submit(y, 20)
    for rid, tok, _ in cb.step():
        got.setdefault("y", []).append(tok)
    cb.submit(zz, 4)
    while cb.prefix_stats()["lookups"] < 3:
        st, px = cb.status(), cb.prefix_stats()
        assert st["waiting"] == 1 and px["evictable_pages"] == 0 and px["cached_pages"] == 3, (st, px)
        for rid, tok, _ in cb.step():
            got.setdefault("y" if rid == ry else "z", []).append(tok)
    assert cb.prefix_stats()["evictions"] == 0
    while cb.busy():
        for rid, tok, _ in cb.step():
            got.setdefault("y" if rid == ry else "z", []).append(tok)
    # w needs 6 pages with 4 free: the two least recently used leaves go (y's third block, then x's second)
    got["w"] = _run(cb, [(wv, 8)])[0][0]
    px = cb.prefix_stats()
    assert px["evictions"] == 2, px
    assert cb.status()["free_pages"] + px["cached_pages"] == 10
    # y again: only x's first block is left of its prefix -> a partial hit of 8 tokens; then x: 16 again (y re-inserted them)
    h0 = px["hit_tokens"]
    got["y2"] = _run(cb, [(y, 20)])[0][0]
    assert cb.prefix_stats()["hit_tokens"] - h0 == 8
    got["x2"] = _run(cb, [(x, 3)])[0][0]
    assert cb.prefix_stats()["hit_tokens"] - h0 == 24
    ref = {"x": _oracle(model, x, 3, end_id, top_k=1), "y": _oracle(model, y, 20, end_id, top_k=1),
           "z": _oracle(model, zz, 4, end_id, top_k=1), "w": _oracle(model, wv, 8, end_id, top_k=1)}
    ref["y2"], ref["x2"] = ref["y"], ref["x"]
    for k in ref:
        assert got[k] == ref[k], (k, got[k], ref[k])
    _accounted(cb, 10)


def test_a_hit_is_admitted_in_chunks_from_the_hit_offset(gh, tiny, monkeypatch):
    """FTCF_BATCHER_PREFILL_CHUNK=4 and a slot running: B's 16 cached tokens are skipped, its 11-token tail is prefilled as
    4 + 4 + 3 with a decode step of the running request after the first two chunks."""
    monkeypatch.setenv("FTCF_BATCHER_PREFILL_CHUNK", "4")
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z, model, op = tiny
    V, end_id = cfg["vocab_size"], cfg["end_id"]
    rng = np.random.RandomState(17)
    a = rng.randint(3, V, size=19).tolist()
    b = a[:16] + rng.randint(3, V, size=11).tolist()
    pb = z["prompt_b"].tolist()
    cb = ContinuousBatcher(op, max_batch=3, page_tokens=8, num_pages=24, max_seq_len=64, prefix_cache=True)
    got_a, _ = _run(cb, [(a, 4)])
    got, per_step = _run(cb, [(pb, 12), (b, 6)], arrivals={0: [0], 1: [1]})
    assert per_step[1] == [0, 0, 0, 1], per_step[:3]
    assert cb.prefix_stats()["hit_tokens"] == 16
    assert got_a[0] == _oracle(model, a, 4, end_id, top_k=1)
    assert got[0] == _oracle(model, pb, 12, end_id, top_k=1)
    assert got[1] == _oracle(model, b, 6, end_id, top_k=1)
    _accounted(cb, 24)


def test_sampling_penalty_and_stop_words_are_the_same_with_and_without_the_cache(gh, tiny):
    """A seeded top-k request with a repetition penalty and stop words: the same tokens cold and with a hit; a greedy request
    with a strong penalty follows the oracle, whose penalty sees the whole prompt, cached prefix included."""
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z, model, op = tiny
    V, end_id = cfg["vocab_size"], cfg["end_id"]
    rng = np.random.RandomState(23)
    prefix = rng.randint(3, V, size=24).tolist()
    p1 = prefix + rng.randint(3, V, size=5).tolist()
    p2 = prefix + rng.randint(3, V, size=3).tolist()
    free = _oracle(model, p2, 10, end_id, top_k=1)
    stop = [[free[6]]]
    kw = dict(top_k=8, temperature=0.9, seed=99, repetition_penalty=1.4, stop_words=[[7, 8], [free[7], free[8]]])
    out = {}
    for on in (False, True):
        cb = ContinuousBatcher(op, max_batch=2, page_tokens=8, num_pages=24, max_seq_len=64, prefix_cache=on)
        r0 = cb.submit(p1, 4)
        cb.run_all()
        r1 = cb.submit(p2, 10, **kw)
        r2 = cb.submit(p2, 10, top_k=1, repetition_penalty=2.5, stop_words=stop)
        res = cb.run_all()
        out[on] = (res[r1], res[r2])
        assert r0 < r1
        assert cb.prefix_stats()["hit_tokens"] == (2 * 24 if on else 0)  # (r2 is admitted alone after r1: it hits too)
    assert out[True][0] == out[False][0]
    ref = _oracle(model, p2, 10, end_id, top_k=1, repetition_penalty=2.5, stop_words=stop)
    assert out[True][1] == out[False][1] == ref


@pytest.mark.parametrize("int8_mode", [0, 1])
def test_mid_model_hits_follow_the_engine(gh, int8_mode):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    from tests.test_gpu_batcher import _alone
    cfg = MID
    w = random_model(cfg, seed=17)
    V, end_id = cfg["vocab_size"], cfg["end_id"]
    op = gh.make_op(cfg, w, int8_mode=int8_mode)
    rng = np.random.RandomState(41)
    system = rng.randint(3, V, size=50).tolist()
    reqs = [(system + rng.randint(3, V, size=int(rng.randint(1, 30))).tolist(), int(rng.randint(2, 12))) for _ in range(6)]
    cb = ContinuousBatcher(op, max_batch=4, page_tokens=16, num_pages=48, max_seq_len=96, prefix_cache=True)
    got, _ = _run(cb, reqs, arrivals={0: [0], 3: [1, 2], 4: [3], 6: [4, 5]})
    assert cb.prefix_stats()["hit_tokens"] >= 3 * 48
    for i, (p, n) in enumerate(reqs):
        alone, logits = _alone(gh, op, p, n, V, end_id)
        for t, (a, b) in enumerate(zip(got[i], alone)):
            if a != b:  # (test_gpu_batcher.py's convention: only a near tie may flip a token)
                top2 = np.sort(logits[t])[-2:]
                assert top2[1] - top2[0] <= 1e-2 * np.abs(logits[t]).max(), (i, t)
                break
        else:
            assert len(got[i]) == len(alone)
    _accounted(cb, 48)


def test_cancelling_a_request_on_shared_pages(gh, tiny):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z, model, op = tiny
    V, end_id = cfg["vocab_size"], cfg["end_id"]
    rng = np.random.RandomState(4)
    base = rng.randint(3, V, size=20).tolist()
    b = base[:17] + rng.randint(3, V, size=4).tolist()
    c = base[:18] + rng.randint(3, V, size=6).tolist()
    cb = ContinuousBatcher(op, max_batch=2, page_tokens=8, num_pages=16, max_seq_len=48, prefix_cache=True)
    _run(cb, [(base, 2)])
    got, it, rb, rc = {}, 0, None, None
    rb = cb.submit(b, 15)
    rc = cb.submit(c, 12)
    while cb.busy():
        for rid, tok, _ in cb.step():
            got.setdefault(rid, []).append(tok)
        it += 1
        if it == 4:
            assert cb.cancel(rb)
            assert cb.prefix_stats()["cached_pages"] == 3  # (base's two blocks and c's third)
    assert cb.prefix_stats()["hit_tokens"] == 32
    assert got[rc] == _oracle(model, c, 12, end_id, top_k=1)
    assert len(got[rb]) < 15
    # the cache is intact: the prefix is served again and exact
    again, _ = _run(cb, [(b, 5)])
    assert again[0] == _oracle(model, b, 5, end_id, top_k=1) and cb.prefix_stats()["hit_tokens"] == 48
    _accounted(cb, 16)


def test_a_beam_request_neither_reads_nor_populates_the_cache(gh, tiny):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    from tests.test_gpu_batcher import _beam_alone
    cfg, w, z, model, op = tiny
    V = cfg["vocab_size"]
    p = np.random.RandomState(6).randint(3, V, size=21).tolist()
    cb = ContinuousBatcher(op, max_batch=4, page_tokens=8, num_pages=32, max_seq_len=48, prefix_cache=True)
    _run(cb, [(p, 3)])
    s0 = cb.prefix_stats()
    bid = cb.submit_beam(p, 7, 3)
    cb.run_all()
    ids, lens, cum = cb.beam_result(bid)
    ref = _beam_alone(gh, op, p, 7, V, 3)
    assert np.array_equal(ids, ref[0]) and np.array_equal(lens, ref[1])
    np.testing.assert_allclose(cum, ref[2], rtol=1e-3, atol=1e-3)
    assert cb.prefix_stats() == s0
    _accounted(cb, 32)


def test_the_cache_is_refused_where_reuse_is_impossible(gh):
    import threading
    import torch
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    from fastertransformer4codefuse_amd.gptneox_op import LocalTensorParallelGroup
    from tests.helpers import shard_weights
    cfg, w, z = load_tiny()
    op = gh.make_op(cfg, w)
    assert ContinuousBatcher(op, max_batch=2, page_tokens=8, num_pages=8, max_seq_len=32).prefix_stats() == dict(
        enabled=0, cached_pages=0, evictable_pages=0, lookups=0, prompt_tokens=0, hit_tokens=0, computed_tokens=0, evictions=0)
    op32 = gh.make_op(cfg, w, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="prefix cache"):
        ContinuousBatcher(op32, max_batch=2, page_tokens=8, num_pages=8, max_seq_len=32, prefix_cache=True)
    group = LocalTensorParallelGroup()
    errs = [None, None]

    def worker(r):
        try:
            opr = gh.make_op(cfg, shard_weights(cfg, w, 2, r), tp=2, rank=r, comm=group)
            try:
                ContinuousBatcher(opr, max_batch=2, page_tokens=8, num_pages=8, max_seq_len=32, prefix_cache=True)
            except RuntimeError as e:
                errs[r] = str(e)
        except Exception as e:  # (the group itself must come up)
            errs[r] = "setup: " + repr(e)

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert all(e is not None and "prefix cache" in e and not e.startswith("setup") for e in errs), errs
