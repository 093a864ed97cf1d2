"""-m gpu: n samples of one prompt from ONE prompt phase (ContinuousBatcher.submit_n / ftcf_batcher_submit_n).

The promise is the batcher's usual one: sibling i of a fork request produces exactly the tokens the plain submission of the same
prompt and options with seed + i produces ALONE in a fresh batcher of the same geometry -- token for token, no tolerance --
while the prompt runs through the model once (fork_stats()["prompt_tokens_computed"]) and its full pages are held once
(status()["free_pages"] right after the admission).  Greedy siblings also equal the CPU oracle.  First-token log-probabilities
and top-N pairs are compared with the tolerance of the batcher's log-probability tests (2e-3 + 2e-3 relative)."""
import math

import numpy as np
import pytest

from tests.helpers import load_tiny

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
P = 8
GEOM = dict(max_batch=4, page_tokens=P, num_pages=40, max_seq_len=64)
TOL = 2e-3
TOPK = dict(top_k=8, temperature=0.9)
TOPP = dict(top_p=0.9)
_ALONE = {}  # (int8_mode, geometry, prompt, n_new, options) -> the stream of the plain request alone: computed once, shared


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


@pytest.fixture(scope="module")
def tiny(gh):
    cfg, w, z = load_tiny()
    return cfg, w, z, {m: gh.make_op(cfg, w, int8_mode=m) for m in (0, 1)}


def _cb(op, **kw):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    return ContinuousBatcher(op, **dict(GEOM, **kw))


def _key(v):
    return tuple(sorted((k, _key(x)) for k, x in v.items())) if isinstance(v, dict) else (
        tuple(_key(x) for x in v) if isinstance(v, (list, tuple)) else v)


def _alone(ops, m, prompt, n_new, geom=None, mask=None, **kw):
    """The reference: the plain request alone in a fresh batcher of the same geometry (mask: set while it waits)."""
    key = (m, _key(geom or {}), tuple(prompt), n_new, _key(kw), _key(mask) if mask is not None else None)
    if key not in _ALONE:
        cb = _cb(ops[m], **(geom or {}))
        rid = cb.submit(prompt, n_new, **kw)
        if mask is not None:
            cb.set_token_mask(rid, mask)
        _ALONE[key] = cb.run_all()[rid]
        assert cb.status()["free_pages"] + cb.prefix_stats()["cached_pages"] == dict(GEOM, **(geom or {}))["num_pages"]
    return _ALONE[key]


def _prompt(V, S, seed=0):
    return np.random.RandomState(1000 * seed + S).randint(3, V, size=S).tolist()


def _pages(S, n_new, n):
    shared = S // P
    own = (S + n_new + P - 1) // P - shared
    return shared, own


@pytest.mark.parametrize("sampling", [TOPK, TOPP], ids=["top_k", "top_p"])
@pytest.mark.parametrize("S", [7, 8, 9, 16, 17])
@pytest.mark.parametrize("int8_mode", [0, 1])
def test_every_sibling_equals_the_plain_request_of_seed_plus_i_alone(tiny, int8_mode, S, sampling):
    """Tails of P - 1, 0, 1, 0, 1 rows; n = 2, 3 and max_batch; the prompt is computed once and its full pages are held once."""
    cfg, w, z, ops = tiny
    V, n_new, seed = cfg["vocab_size"], 10, 40 + S
    prompt = _prompt(V, S)
    for n in (2, 3, 4):
        cb = _cb(ops[int8_mode])
        ids = cb.submit_n(prompt, n_new, n, seed=seed, **sampling)
        assert ids == list(range(ids[0], ids[0] + n)) and cb.status()["waiting"] == 1
        got = {}
        first = cb.step()
        assert [e[0] for e in first] == ids  # n events, in sibling order
        shared, own = _pages(S, n_new, n)
        assert cb.status()["free_pages"] == GEOM["num_pages"] - (shared + n * own)
        assert cb.fork_stats() == dict(requests=1, siblings=n, shared_pages=(n - 1) * shared, prompt_tokens_computed=S)
        for rid, tok, _ in first:
            got.setdefault(rid, []).append(tok)
        for rid, toks in cb.run_all().items():
            got.setdefault(rid, []).extend(toks)
        for i, rid in enumerate(ids):
            want = _alone(ops, int8_mode, prompt, n_new, seed=seed + i, **sampling)
            assert got[rid] == want, (n, i, got[rid], want)
        assert cb.status() == {"waiting": 0, "running": 0, "free_pages": GEOM["num_pages"]}
        assert cb.fork_stats()["prompt_tokens_computed"] == S


@pytest.mark.parametrize("S", [9, 16])
def test_three_greedy_siblings_are_one_stream_and_the_oracles(tiny, S):
    from oracle import oracle as orc
    from tests.helpers import weight_list_to_layers
    from tests.test_gpu_batcher import _oracle_alone
    cfg, w, z, ops = tiny
    layers, glob = weight_list_to_layers(cfg, w)
    model = orc.Model(dict(cfg, fp16=1), layers, glob)
    prompt = z["prompt"].tolist()[:S] if len(z["prompt"]) >= S else _prompt(cfg["vocab_size"], S, 3)
    cb = _cb(ops[0])
    ids = cb.submit_n(prompt, 8, 3)
    out = cb.run_all()
    ref = _oracle_alone(model, prompt, 8, cfg["end_id"], top_k=1)
    assert out[ids[0]] == out[ids[1]] == out[ids[2]] == ref
    assert out[ids[0]] == _alone(ops, 0, prompt, 8)
    assert cb.status()["free_pages"] == GEOM["num_pages"]


def test_one_sample_is_the_plain_request(tiny):
    cfg, w, z, ops = tiny
    prompt = _prompt(cfg["vocab_size"], 11, 1)
    cb = _cb(ops[0])
    ids = cb.submit_n(prompt, 6, 1, seed=5, **TOPK)
    assert len(ids) == 1 and cb.run_all()[ids[0]] == _alone(ops, 0, prompt, 6, seed=5, **TOPK)
    assert cb.fork_stats() == dict(requests=0, siblings=0, shared_pages=0, prompt_tokens_computed=0)


def test_masks_set_on_waiting_siblings_govern_their_first_tokens(tiny):
    """Siblings 0 and 2 get masks of their own while the fork waits; sibling 1 has none: the rows differ in their processed logits."""
    cfg, w, z, ops = tiny
    V = cfg["vocab_size"]
    prompt = _prompt(V, 13, 2)
    masks = {0: [5], 1: None, 2: [11, 12, 13, 14, 15, 16, 17, 18]}
    cb = _cb(ops[0])
    ids = cb.submit_n(prompt, 7, 3, seed=9, **TOPK)
    for i, m in masks.items():
        if m is not None:
            cb.set_token_mask(ids[i], m)
    first = {rid: tok for rid, tok, _ in cb.step()}
    assert first[ids[0]] == 5 and first[ids[2]] in masks[2]
    out = cb.run_all()
    for i, rid in enumerate(ids):
        want = _alone(ops, 0, prompt, 7, seed=9 + i, mask=masks[i], **TOPK)
        assert [first[rid]] + out.get(rid, []) == want, (i, want)
        if masks[i] is not None:
            assert set(want) <= set(masks[i]) | {cfg["end_id"]}


def test_logit_bias_and_repetition_penalty_apply_to_every_sibling(tiny):
    cfg, w, z, ops = tiny
    V = cfg["vocab_size"]
    prompt = _prompt(V, 15, 4)
    free = _alone(ops, 0, prompt, 8)
    up = next(t for t in range(3, V) if t not in free)
    kw = dict(repetition_penalty=1.4, logit_bias={free[0]: -np.inf, free[1]: -np.inf, up: 3.0}, presence_penalty=0.5, **TOPK)
    cb = _cb(ops[0])
    ids = cb.submit_n(prompt, 8, 3, seed=21, **kw)
    out = cb.run_all()
    for i, rid in enumerate(ids):
        assert out[rid] == _alone(ops, 0, prompt, 8, seed=21 + i, **kw), i
        assert free[0] not in out[rid] and free[1] not in out[rid]


def test_a_stop_word_ends_one_sibling_while_the_others_go_on(tiny):
    cfg, w, z, ops = tiny
    V = cfg["vocab_size"]
    prompt = _prompt(V, 12, 5)
    free = [_alone(ops, 0, prompt, 12, seed=60 + i, **TOPK) for i in range(3)]
    # a token sibling 1 emits before its end that sibling 0 never emits
    stop = next(t for t in free[1][:-2] if t not in free[0] and t != cfg["end_id"])
    cb = _cb(ops[0])
    ids = cb.submit_n(prompt, 12, 3, seed=60, stop_words=[[stop]], **TOPK)
    out = cb.run_all()
    want = [_alone(ops, 0, prompt, 12, seed=60 + i, stop_words=[[stop]], **TOPK) for i in range(3)]
    assert [out[r] for r in ids] == want
    assert want[1][-1] == stop and len(want[1]) < len(free[1]) and want[0] == free[0]
    assert cb.status()["free_pages"] == GEOM["num_pages"]


def test_cancelling_a_running_sibling_leaves_the_shared_pages_to_the_rest(tiny):
    cfg, w, z, ops = tiny
    prompt = _prompt(cfg["vocab_size"], 17, 6)
    n_new = 12
    shared, own = _pages(17, n_new, 3)
    cb = _cb(ops[0])
    ids = cb.submit_n(prompt, n_new, 3, seed=70, **TOPK)
    got = {}
    for it in range(3):
        for rid, tok, _ in cb.step():
            got.setdefault(rid, []).append(tok)
    before = cb.status()["free_pages"]
    assert cb.cancel(ids[1]) and not cb.cancel(ids[1])
    assert cb.status()["free_pages"] == before + own  # (its own pages only: the prompt's stay with the others)
    for rid, toks in cb.run_all().items():
        got.setdefault(rid, []).extend(toks)
    assert len(got[ids[1]]) == 3
    for i in (0, 2):
        assert got[ids[i]] == _alone(ops, 0, prompt, n_new, seed=70 + i, **TOPK), i
    assert cb.status()["free_pages"] == GEOM["num_pages"]


def test_cancelling_waiting_siblings_shrinks_the_fork(tiny):
    cfg, w, z, ops = tiny
    prompt = _prompt(cfg["vocab_size"], 9, 7)
    cb = _cb(ops[0])
    ids = cb.submit_n(prompt, 6, 4, seed=80, **TOPK)
    assert cb.cancel(ids[0]) and cb.cancel(ids[2]) and not cb.cancel(ids[2]) and cb.status()["waiting"] == 1
    out = cb.run_all()
    assert sorted(out) == [ids[1], ids[3]]
    for i in (1, 3):  # (a sibling keeps its index: its seed is seed + i whoever left)
        assert out[ids[i]] == _alone(ops, 0, prompt, 6, seed=80 + i, **TOPK), i
    assert cb.fork_stats()["siblings"] == 2
    ids = cb.submit_n(prompt, 6, 2)
    assert cb.cancel(ids[0]) and cb.cancel(ids[1]) and cb.status()["waiting"] == 0 and not cb.busy()


@pytest.mark.parametrize("cache", [False, True])
def test_a_sibling_that_ends_with_its_first_token_releases_cleanly(tiny, cache):
    cfg, w, z, ops = tiny
    end_id = cfg["end_id"]
    prompt = _prompt(cfg["vocab_size"], 16, 8)
    cb = _cb(ops[0], prefix_cache=cache)
    ids = cb.submit_n(prompt, 6, 3, seed=90, **TOPK)
    cb.set_token_mask(ids[0], [end_id])
    first = cb.step()
    assert first[0] == (ids[0], end_id, True) and [e[0] for e in first] == ids
    shared, own = _pages(16, 6, 3)
    assert cb.status()["free_pages"] == GEOM["num_pages"] - (shared + 2 * own)
    out = cb.run_all()
    for i in (1, 2):
        want = _alone(ops, 0, prompt, 6, seed=90 + i, geom=dict(prefix_cache=cache), **TOPK)
        assert [first[i][1]] + out.get(ids[i], []) == want, i
    assert cb.status()["free_pages"] + cb.prefix_stats()["cached_pages"] == GEOM["num_pages"]
    assert cb.prefix_stats()["cached_pages"] == (shared if cache else 0)


def test_fork_requests_read_and_populate_the_prefix_cache(tiny):
    cfg, w, z, ops = tiny
    V = cfg["vocab_size"]
    rng = np.random.RandomState(12)
    a = rng.randint(3, V, size=20).tolist()
    f = a[:17] + rng.randint(3, V, size=9).tolist()  # 26 tokens: 2 of its 3 full blocks are a's
    c = f[:24] + rng.randint(3, V, size=5).tolist()  # the third block is the fork's own
    geom = dict(prefix_cache=True)
    cb = _cb(ops[0], **geom)
    cb.submit(a, 3)
    cb.run_all()
    h0 = cb.prefix_stats()["hit_tokens"]
    ids = cb.submit_n(f, 8, 3, seed=33, **TOPK)
    first = cb.step()
    assert cb.prefix_stats()["hit_tokens"] - h0 == 16
    assert cb.fork_stats() == dict(requests=1, siblings=3, shared_pages=2 * 3, prompt_tokens_computed=len(f) - 16)
    out = cb.run_all()
    for i, rid in enumerate(ids):
        assert [first[i][1]] + out.get(rid, []) == _alone(ops, 0, f, 8, geom=geom, seed=33 + i, **TOPK), i
    h1 = cb.prefix_stats()["hit_tokens"]
    rc = cb.submit(c, 5)
    assert cb.run_all()[rc] == _alone(ops, 0, c, 5, geom=geom)
    assert cb.prefix_stats()["hit_tokens"] - h1 == 24  # (the block the fork inserted among them)
    st, px = cb.status(), cb.prefix_stats()
    assert st["free_pages"] + px["cached_pages"] == GEOM["num_pages"], (st, px)
    cb.clear_prefix_cache()
    assert cb.status()["free_pages"] == GEOM["num_pages"]


def test_overcommit_swaps_a_sibling_out_and_every_stream_stays_exact(tiny):
    """4 siblings of 9 + 40 tokens need 1 + 4 * 6 pages at full length; the pool has 14: the latest sibling leaves and comes back."""
    cfg, w, z, ops = tiny
    prompt = _prompt(cfg["vocab_size"], 9, 9)
    geom = dict(num_pages=14, overcommit=True)
    cb = _cb(ops[0], **geom)
    ids = cb.submit_n(prompt, 40, 4, seed=50, **TOPK)
    first = cb.step()
    assert cb.status()["free_pages"] == 14 - (1 + 4 * 1)  # (overcommit: every sibling owns one page)
    out = cb.run_all()
    pe = cb.preempt_stats()
    assert pe["preemptions"] > 0 and pe["resumes"] == pe["preemptions"] and pe["swapped_requests"] == 0, pe
    for i, rid in enumerate(ids):
        assert [first[i][1]] + out.get(rid, []) == _alone(ops, 0, prompt, 40, geom=geom, seed=50 + i, **TOPK), i
    assert cb.status()["free_pages"] == 14 and cb.preempt_stats()["swap_pages_used"] == 0


def test_a_fork_arriving_while_others_run_is_admitted_in_chunks(tiny, monkeypatch):
    """FTCF_BATCHER_PREFILL_CHUNK=4 and a slot running: the 17-token prompt is prefilled as 4 + 4 + 4 + 4 + 1 with a decode step
    of the running request after each of the first four chunks; the fork happens when the last chunk is in."""
    monkeypatch.setenv("FTCF_BATCHER_PREFILL_CHUNK", "4")
    cfg, w, z, ops = tiny
    pb = z["prompt_b"].tolist()
    prompt = _prompt(cfg["vocab_size"], 17, 10)
    cb = _cb(ops[0])
    r0 = cb.submit(pb, 12)
    got = {}
    per_step = []
    ids = None
    while cb.busy():
        evs = cb.step()
        per_step.append([e[0] for e in evs])
        for rid, tok, _ in evs:
            got.setdefault(rid, []).append(tok)
        if ids is None:
            ids = cb.submit_n(prompt, 6, 2, seed=44, **TOPK)
    assert per_step[1] == [r0] * 5 + ids, per_step[:3]
    assert cb.fork_stats()["prompt_tokens_computed"] == 17
    monkeypatch.delenv("FTCF_BATCHER_PREFILL_CHUNK")
    assert got[r0] == _alone(ops, 0, pb, 12)
    for i, rid in enumerate(ids):
        assert got[rid] == _alone(ops, 0, prompt, 6, seed=44 + i, **TOPK), i
    assert cb.status()["free_pages"] == GEOM["num_pages"]


def test_first_token_log_probs_and_top_pairs_on_the_admitting_iteration(tiny):
    cfg, w, z, ops = tiny
    prompt = _prompt(cfg["vocab_size"], 14, 11)
    close = lambda a, b: abs(a - b) <= TOL + TOL * abs(b)
    cb = _cb(ops[0])
    ids = cb.submit_n(prompt, 4, 3, seed=15, **TOPK)
    evs = cb.step_ex()
    assert [e[0] for e in evs] == ids
    for i, (rid, tok, fin, lp) in enumerate(evs):
        ref = _cb(ops[0])
        ref.submit(prompt, 4, seed=15 + i, **TOPK)
        (_, rtok, rfin, rlp), = ref.step_ex()
        assert (tok, fin) == (rtok, rfin) and math.isfinite(lp) and close(lp, rlp), (i, lp, rlp)
    cb.run_all()
    ids = cb.submit_n(prompt, 4, 3, seed=15, **TOPK)
    evs = cb.step(top_logprobs=3)
    assert [e[0] for e in evs] == ids
    for i, (rid, tok, fin, lp, top_ids, top_lps) in enumerate(evs):
        ref = _cb(ops[0])
        ref.submit(prompt, 4, seed=15 + i, **TOPK)
        (_, rtok, rfin, rlp, rids, rlps), = ref.step(top_logprobs=3)
        assert (tok, fin, top_ids) == (rtok, rfin, rids) and close(lp, rlp), (i, top_ids, rids)
        assert all(close(a, b) for a, b in zip(top_lps, rlps)), (i, top_lps, rlps)


def test_what_cannot_run_is_refused_and_queues_nothing(tiny):
    from fastertransformer4codefuse_amd.capi import FtcfError
    cfg, w, z, ops = tiny
    prompt = _prompt(cfg["vocab_size"], 9, 12)
    cb = _cb(ops[0], num_pages=12)
    # n < 1, n > max_batch; siblings of 9 + 40 tokens share 1 page and own 6 each: 4 need 25 pages and 2 need 13, the pool has 12
    for n, n_new in ((0, 4), (5, 4), (-1, 4), (4, 40), (2, 40)):
        with pytest.raises(FtcfError) as e:
            cb.submit_n(prompt, n_new, n)
        assert e.value.code == -1, (n, e.value)
        assert cb.status() == {"waiting": 0, "running": 0, "free_pages": 12}
    ids = cb.submit_n(prompt, 4, 2)
    assert ids == [1, 2]  # (the refused calls took no ids)
    out = cb.run_all()
    assert out[1] == out[2] == _alone(ops, 0, prompt, 4, geom=dict(num_pages=12))
