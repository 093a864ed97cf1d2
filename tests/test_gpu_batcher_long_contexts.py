"""-m gpu: the continuous batcher at long contexts and at page sizes that are not powers of two.  Every request's tokens and
step_ex log-probabilities are what the engine alone returns for it (within TOL of tests/test_gpu_batcher_log_probs.py or FRAC of
the logit range, see below; a token may only flip at a near tie of the engine's logits, after which the histories part), in each decode form of the batcher:

- the rows kernel over pages (at most 16 slots, page_tokens a multiple of its key block: 16 keys at size_per_head 128, 32 at 64);
- the per-GEMM launches with k_mmha_paged (FTCF_BATCHER_ROWS=0);
- more than 16 slots running (k_mmha_paged).

Prompts sit at page edges (P - 1, P, P + 1, 2P), one is 2011 tokens long and one fills the longest max_seq_len the batcher accepts
for the geometry (the LDS rule of k_mmha_paged: ~15,000 tokens); the two long ones arrive while the others run, so they are admitted
in chunks between decode steps.  Every request decodes 2P + 2 tokens: across at least two page boundaries.

The rows kernel over pages runs here with int8 weights (MID at P 48, SMALL64 at P 32); fp16 MID runs at P 24, on k_mmha_paged.

_alone and _check are this file's own, not those of test_gpu_batcher_log_probs.py: a flip needs the engine's logits to be judged
a near tie, and the bound needs the step's logit range (FRAC below); the tokens and the TOL comparison are as there."""
import numpy as np
import pytest

from tests.helpers import longest_paged_len as longest
from tests.helpers import random_model
from tests.test_gpu_batcher_log_probs import TOL
from tests.test_gpu_log_probs import run
from tests.test_gpu_rows import MID, SMALL64

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


def _alone(op, prompt, n_new, V):
    """The engine alone, greedy: (tokens up to and including the end, their output_log_probs, the logits of every step)."""
    p = np.asarray(prompt, dtype=np.int32)
    r = run(op, p[None, :], [len(p)], n_new, V, debug=True, olp=True, top_k=1)
    n = int(r["sequence_lengths"][0]) - len(p)
    return r["output_ids"][0, len(p):len(p) + n].tolist(), r["output_log_probs"][0, :n], r["logits"][:n, 0]


# Between the batcher and the engine alone only the summation order differs (other kernels), and on these random models that
# moves a decode step's log-probs by more than TOL (the tiny model's bound): a log-prob must then be within FRAC of the step's
# logit range (|logit| reaches 30..45 here).  Measured on MI355X: worst |difference| / max |logit| 7.6e-4 over every case below
# (a rows kernel that appends a page-start token into the previous page: 5.0e-3).
FRAC = 1.5e-3


def _check(k, toks, lps, ref):
    """Tokens equal and log-probs within TOL (or FRAC of the logit range) up to a flip; a flip must be a near tie of the engine's
    logits (the batcher's token within that bound of the maximum), and its log-prob the engine's log-softmax of that token.
    -> the worst |difference| / max |logit|."""
    want_t, want_l, logits = ref
    lps = np.array(lps, dtype=np.float64)
    n = min(len(toks), len(want_t))
    flip = next((s for s in range(n) if toks[s] != want_t[s]), None)
    upto = n if flip is None else flip
    assert flip is not None or toks == want_t, (k, len(toks), len(want_t))
    scale = np.abs(logits[:n]).max(axis=1).astype(np.float64)
    bound = np.maximum(TOL + TOL * np.abs(want_l[:n]), FRAC * scale)
    d = np.abs(lps[:upto] - want_l[:upto])
    assert np.all(d <= bound[:upto]), (k, int(np.argmax(d - bound[:upto])), float(d.max()), float((d / scale[:upto]).max()))
    if flip is not None:
        lg = logits[flip].astype(np.float64)
        lse = lg.max() + np.log(np.exp(lg - lg.max()).sum())
        gap = lg.max() - lg[toks[flip]]
        assert gap <= 2 * bound[flip], (k, flip, "token flip without a near tie", gap)
        assert abs(lps[flip] - (lg[toks[flip]] - lse)) <= bound[flip], (k, flip, lps[flip])
    return float((d / scale[:upto]).max()) if upto else 0.0


def _serve(op, cb, reqs, late):
    """reqs[k] = (prompt, max_new); the indices in `late` are submitted after the first step, with the others running.
    -> ({index: (tokens, log_probs)}, decode paths of the steps that decoded, most slots running at once)."""
    ids, got, paths, most = {}, {}, set(), 0
    for k, (p, n) in enumerate(reqs):
        if k not in late:
            ids[cb.submit(p, n)] = k
    it = 0
    while cb.busy():
        evs = cb.step_ex()
        decoded = False
        for rid, tok, _fin, lp in evs:
            t, l = got.setdefault(ids[rid], ([], []))
            decoded |= len(t) > 0  # (a second token: the step ran a decode step)
            t.append(tok)
            l.append(lp)
        if decoded:
            paths.add(op.stats()["decode_path"])
        most = max(most, cb.status()["running"])
        if it == 0:
            for k in late:
                ids[cb.submit(*reqs[k])] = k
        it += 1
        assert it < 5000
    return got, paths, most


CASES = [("mid", 1, 48), ("mid", 0, 24), ("small64", 0, 48), ("small64", 1, 32)]


@pytest.mark.parametrize("model,int8_mode,P", CASES)
def test_long_prompts_and_odd_page_sizes_follow_the_engine_alone(gh, monkeypatch, model, int8_mode, P):
    """MID (size_per_head 128) in int8 and fp16, SMALL64 (size_per_head 64); page_tokens 48 (the rows kernel at 128, k_mmha_paged at
    64), 24 (k_mmha_paged) and 32 (the rows kernel at 64)."""
    from fastertransformer4codefuse_amd import capi
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    cfg = dict(MID if model == "mid" else SMALL64)
    dh, V = cfg["size_per_head"], cfg["vocab_size"]
    w = random_model(cfg, seed=11 + P + int8_mode, std=0.04)
    op = gh.make_op(cfg, w, int8_mode=int8_mode)
    max_seq = longest(dh, P)
    # creation: the LDS limit is accepted, one page more is refused
    with pytest.raises(capi.FtcfError, match="max_seq_len too large"):
        ContinuousBatcher(op, 4, P, 16, max_seq + P)
    m = 2 * P + 2
    rng = np.random.RandomState(P + dh)
    reqs = [(rng.randint(3, V, size=n).tolist(), m) for n in (P - 1, P, P + 1, 2 * P, 2011, max_seq - m)]
    late = (4, 5)
    refs = [_alone(op, p, n, V) for p, n in reqs]
    assert len(refs[5][0]) >= 1
    rows_form = P % (16 if dh == 128 else 32) == 0
    forms = (["rows"] if rows_form else []) + ["general", "wide"]
    worst = 0.0
    for form in forms:
        if form == "general":
            monkeypatch.setenv("FTCF_BATCHER_ROWS", "0")
        else:
            monkeypatch.delenv("FTCF_BATCHER_ROWS", raising=False)
        form_reqs = reqs + (reqs[:4] * 4 if form == "wide" else [])  # wide: 16 more copies of the short requests (same references)
        mb = 20 if form == "wide" else 8
        pages = sum((len(p) + n + P - 1) // P for p, n in form_reqs) + 8
        cb = ContinuousBatcher(op, mb, P, pages, max_seq)
        free0 = cb.status()["free_pages"]
        got, paths, most = _serve(op, cb, form_reqs, late)
        if form == "rows":
            assert 3 in paths, paths  # the rows kernel read the pages
        else:
            assert 2 in paths and 3 not in paths, paths  # the per-GEMM launches and k_mmha_paged
        if form == "wide":
            assert most > 16, most
        for k, (p, n) in enumerate(form_reqs):
            toks, lps = got[k]
            worst = max(worst, _check((form, k, len(p)), toks, lps, refs[k if k < 6 else (k - 6) % 4]))
        assert cb.status() == {"waiting": 0, "running": 0, "free_pages": free0}  # every slot's pages are back
        del cb
    print(f"{model} int8 {int8_mode} P {P}: worst |d log-prob| / max |logit| {worst:.2e}")
