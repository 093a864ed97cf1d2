"""-m gpu: ContinuousBatcher.step_ex / ftcf_batcher_step_ex -- every event's token carries its log-probability, the value the
engine alone returns as output_log_probs for the same request (paged vs dense attention: values within 2e-3 + 2e-3 relative, tokens exact),
with the prefix cache, for sampled requests, for chunked admissions; a beam request's event carries NaN."""
import math

import numpy as np
import pytest

from tests.helpers import load_tiny

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
TOL = 2e-3


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


@pytest.fixture(scope="module")
def tiny(gh):
    cfg, w, z = load_tiny()
    return cfg, w, z, gh.make_op(cfg, w)


def _alone(op, prompt, n_new, V, top_k=1, top_p=0.0, temperature=1.0, seed=0):
    """The engine alone: (tokens up to and including the end / the last, their output_log_probs)."""
    from tests.test_gpu_log_probs import run
    p = np.asarray(prompt, dtype=np.int32)
    r = run(op, p[None, :], [len(p)], n_new, V, debug=False, olp=True, top_k=top_k, top_p=top_p, temperature=temperature,
            random_seed=seed)
    n = int(r["sequence_lengths"][0]) - len(p)
    return r["output_ids"][0, len(p):len(p) + n].tolist(), r["output_log_probs"][0, :n]


def _drain(cb, reqs, **kw):
    """Submit all, drain with step_ex; {index: ([tokens], [log_probs])}."""
    ids = {cb.submit(p, n, **kw): k for k, (p, n) in enumerate(reqs)}
    got = {}
    it = 0
    while cb.busy():
        for rid, tok, _fin, lp in cb.step_ex():
            t, l = got.setdefault(ids[rid], ([], []))
            t.append(tok)
            l.append(lp)
        it += 1
        assert it < 5000
    return got


def _check(op, got, reqs, V, **kw):
    for k, (p, n) in enumerate(reqs):
        toks, lps = got[k]
        want_t, want_l = _alone(op, p, n, V, **kw)
        assert toks == want_t, (k, toks, want_t)
        assert all(math.isfinite(v) for v in lps)
        np.testing.assert_allclose(np.array(lps, dtype=np.float32), want_l, atol=TOL, rtol=TOL)


def _prompts(V, seed, lens):
    rng = np.random.RandomState(seed)
    return [rng.randint(3, V, size=L).tolist() for L in lens]


def test_greedy_step_ex_matches_the_engine_alone(tiny):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z, op = tiny
    V = cfg["vocab_size"]
    reqs = [(z["prompt"].tolist(), 8), (z["prompt_b"].tolist(), 6)] + [(p, 7) for p in _prompts(V, 1, [5, 20, 9])]
    cb = ContinuousBatcher(op, 4, 16, 64, 64)
    got = _drain(cb, reqs)
    _check(op, got, reqs, V)
    # step() of the same batcher is unchanged: the same tokens without log-probabilities
    ids = {cb.submit(p, n): k for k, (p, n) in enumerate(reqs)}
    plain = {}
    while cb.busy():
        for rid, tok, _ in cb.step():
            plain.setdefault(ids[rid], []).append(tok)
    assert all(plain[k] == got[k][0] for k in plain)


def test_sampled_requests_and_prefix_cache(tiny):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z, op = tiny
    V = cfg["vocab_size"]
    base = _prompts(V, 2, [40])[0]
    reqs = [(base + t, 6) for t in _prompts(V, 3, [3, 5, 2])]
    cb = ContinuousBatcher(op, 4, 16, 64, 80, prefix_cache=True)
    for k, (p, n) in enumerate(reqs):  # one after the other: the later ones hit the first one's pages
        got = _drain(cb, [(p, n)], top_k=4, temperature=0.8, seed=100 + k)
        _check(op, {0: got[0]}, [(p, n)], V, top_k=4, temperature=0.8, seed=100 + k)
    assert cb.prefix_stats()["hit_tokens"] > 0
    got = _drain(cb, reqs)  # greedy, with hits
    _check(op, got, reqs, V)


def test_chunked_admission(tiny, monkeypatch):
    """FTCF_BATCHER_PREFILL_CHUNK=8 and a slot running: the long prompt is prefilled in chunks with decode steps in between."""
    monkeypatch.setenv("FTCF_BATCHER_PREFILL_CHUNK", "8")
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z, op = tiny
    V = cfg["vocab_size"]
    short, long_ = _prompts(V, 4, [4, 37])
    cb = ContinuousBatcher(op, 4, 16, 64, 64)
    got = {}
    ids = {cb.submit(short, 12): 0}
    for rid, tok, _f, lp in cb.step_ex():  # the short one is running now
        got.setdefault(ids[rid], ([], []))[0].append(tok)
        got[ids[rid]][1].append(lp)
    ids[cb.submit(long_, 5)] = 1
    while cb.busy():
        for rid, tok, _f, lp in cb.step_ex():
            t, l = got.setdefault(ids[rid], ([], []))
            t.append(tok)
            l.append(lp)
    _check(op, got, [(short, 12), (long_, 5)], V)


def test_beam_event_carries_nan(tiny):
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg, w, z, op = tiny
    cb = ContinuousBatcher(op, 4, 16, 64, 64)
    rb = cb.submit_beam(z["prompt"].tolist(), 4, 2)
    rg = cb.submit(z["prompt_b"].tolist(), 4)
    evs = []
    while cb.busy():
        evs += cb.step_ex()
    beam = [e for e in evs if e[0] == rb]
    assert len(beam) == 1 and beam[0][1] == -1 and math.isnan(beam[0][3])
    assert all(math.isfinite(e[3]) for e in evs if e[0] == rg)
