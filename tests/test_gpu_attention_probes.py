"""-m gpu: every cached key of every decode-attention path is live, and no other key is (tests/attention_probe_cases.py).

The decode step has four hand-written attention implementations that index the K/V cache on their own: mmha_partial
(attn_device.hip.h: per-stage launches, general path), PsAttn (persist_device.hip.h: the one- / two-row persistent kernel, split
chunks, short and long register form), RwAt<DH, false> (rows_device.hip.h: 16- / 32-key blocks dealt over the streamer waves, a ring
that runs on from pair to pair, shared leftover pairs, the padding-key mask) and RwAt<DH, true> (the same stream over the batcher's
page tables).  The engine tests bound the logits by LOGIT_FRAC = 5e-3 of the oracle's range -- too coarse to see ONE key.  Here one
prompt token of a ONE-attention-layer model is replaced and the request repeated on the same engine:
  * `live`: the logits of every decode step of that row are NOT bit-identical to the base run's, and the change is the oracle's:
    max |d_gpu - d_oracle| <= LOGIT_FRAC * range (d = probed - base logits of the step; a heavy key weighted wrongly);
  * `pad`, `other_row`: logits of every step and all tokens of the observed rows are bit-identical to the base run's.
Every path here is run-to-run reproducible (every sum has a fixed order), which the base request run twice checks first.
Steps count while the histories of all four runs (GPU and oracle, base and probed) agree; what is lost is capped (MAX_LOST).
test_attention_probe_reference.py shows on the CPU that the oracle has the property on every case."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import attention_probe_cases as apc
from tests.attention_probe_cases import LOGIT_FRAC

pytestmark = pytest.mark.gpu

CASES = apc.cases()
KNOBS = ("FTCF_MMHA_WGS", "FTCF_PERSIST", "FTCF_STAGE_MAX_ROWS", "FTCF_PERSIST_NB", "FTCF_PERSIST_OWN", "FTCF_ROWS", "FTCF_ROWS_NB", "FTCF_BATCHER_ROWS",
         "FTCF_BATCHER_PREFILL_CHUNK")
TOP = 20  # pairs per step the batcher returns (it has no logits output): the N most likely tokens and their log-probabilities


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


def _engine(gh, monkeypatch, case):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    return gh.make_op(case.cfg, case.weights(), int8_mode=case.int8_mode)  # (the engine reads the switches when it is created)


def _collect(gh, monkeypatch, case):
    """the base request twice and every probed request on one engine; for a case whose switches the library reads once per process,
    in a child process (tests/attention_probe_worker.py)"""
    from tests import attention_probe_worker as worker
    if not case.child:
        return worker.collect(gh, _engine(gh, monkeypatch, case), case)
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(case.env)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "probes.npz")
        subprocess.run([sys.executable, "-m", "tests.attention_probe_worker", case.name, out], env=env, check=True, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        z = np.load(out)
        get = lambda k: dict(logits=z[k + ".logits"], output_ids=z[k + ".output_ids"])
        return dict(base=get("base"), again=get("again"), paths=z["paths"].tolist(),
                    probed={(r, p): get(f"p{r}_{p}") for _, r, p in case.forwards()})


def _agree(case, b, *runs):
    """decode steps (>= 1) of row b up to which the generated tokens of all runs are equal (and none is end_id)"""
    n, steps = int(case.lens[b]), []
    gen = [r["output_ids"][b, n:n + case.out_len] for r in runs]
    for t in range(1, case.out_len):
        if any(g[t - 1] != gen[0][t - 1] for g in gen) or gen[0][t - 1] == case.cfg["end_id"]:
            break
        steps.append(t)
    return steps


def _check_caps(case, pairs, got, live, live_lost, worst, fig):
    lost = 1.0 - got / max(pairs, 1)
    print(f"{case.name}: path {case.path}, {len(case.probes)} probes in {fig['forwards']} requests, lost {lost:.3f} of the (probe, step) "
          f"pairs, {live_lost} of {live} live probes without their first decode step; smallest oracle live change "
          f"{fig['min_live']:.2e} of range, largest |d_gpu - d_oracle| {worst:.2e} of range")
    assert lost <= apc.MAX_LOST and live_lost <= apc.MAX_LOST * live, (lost, live_lost, live)


@pytest.mark.parametrize("case", [c for c in CASES if c.path != "batcher"], ids=lambda c: c.name)
def test_engine_decode_paths_read_every_live_key_and_no_other(gh, monkeypatch, case):
    from tests.test_gpu_rows import _follows  # the engine tests' rule: logits within LOGIT_FRAC of the oracle's range, flips near ties
    res = _collect(gh, monkeypatch, case)
    base, again = res["base"], res["again"]
    assert all(p == case.path for p in res["paths"]), res["paths"]
    assert np.array_equal(base["logits"], again["logits"]) and np.array_equal(base["output_ids"], again["output_ids"])
    o_base, o_runs, _, fig = apc.reference(case)
    _follows(base, o_base, case.lens, case.out_len)
    pairs = got = live = live_lost = 0
    worst = 0.0
    for kinds, row, pos in case.forwards():
        probed = res["probed"][(row, pos)]
        o_probed = o_runs[(row, pos)]
        for kind in kinds:
            for b in case.observed(row, kind):
                pairs += case.out_len - 1
                if kind == "live":
                    steps = _agree(case, b, base, probed, o_base, o_probed)
                    live += 1
                    live_lost += not steps
                    for t in steps:
                        assert not np.array_equal(probed["logits"][t, b], base["logits"][t, b]), ("a dead key", row, pos, t)
                        d_gpu = probed["logits"][t, b] - base["logits"][t, b]
                        d_orc = o_probed["logits"][t, b] - o_base["logits"][t, b]
                        err = float(np.abs(d_gpu - d_orc).max()) / apc.logit_range(o_base["logits"][t, b])
                        worst = max(worst, err)
                        assert err <= LOGIT_FRAC, ("a key weighted wrongly", row, pos, t, err)
                    got += len(steps)
                else:
                    n = int(case.lens[b])
                    assert np.array_equal(probed["logits"][:, b], base["logits"][:, b]), (kind, row, pos, b)
                    assert np.array_equal(probed["output_ids"][b, n:], base["output_ids"][b, n:]), (kind, row, pos, b)
                    got += case.out_len - 1
    _check_caps(case, pairs, got, live, live_lost, worst, fig)


def _batcher_run(cb, op, case, ids):
    """All requests of the case submitted together; per request the events' (token, top ids, top log-probabilities)."""
    rid = {cb.submit(ids[b, :case.lens[b]].tolist(), case.out_len): b for b in range(case.B)}
    ev = {b: [] for b in range(case.B)}
    it = 0
    while cb.busy():
        for r, tok, fin, lp, top_ids, top_lps in cb.step(top_logprobs=TOP):
            ev[rid[r]].append((tok, np.asarray(top_ids, np.int32), np.asarray(top_lps, np.float32)))
        if it == 2:
            assert op.stats()["decode_path"] == 3  # the rows kernel ran the decode step's layers
        it += 1
        assert it < 1000
    out = dict(output_ids=np.full((case.B, case.S + case.out_len), -1, np.int32), events=ev)
    for b in range(case.B):
        n = int(case.lens[b])
        toks = [e[0] for e in ev[b]]
        out["output_ids"][b, n:n + len(toks)] = toks
    return out


def _log_softmax(x):
    x = x.astype(np.float64)
    m = x.max()
    return x - (m + np.log(np.exp(x - m).sum()))


@pytest.mark.parametrize("case", [c for c in CASES if c.path == "batcher"], ids=lambda c: c.name)
def test_batcher_rows_kernel_reads_every_live_key_of_its_pages_and_no_other(gh, monkeypatch, case):
    """The same probes through the continuous batcher (prefix cache off: no probe is served from shared pages).  It returns
    log-probabilities, not logits: the TOP most likely tokens of each step.  A log-probability is a logit minus the row's
    log-sum-exp, and a change of the logits by at most e moves the log-sum-exp by at most e: the logit bounds apply doubled."""
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    op = _engine(gh, monkeypatch, case)
    P = case.page_tokens
    per_req = (case.S + case.out_len + P - 1) // P
    cb = ContinuousBatcher(op, max_batch=case.B, page_tokens=P, num_pages=case.B * per_req + 2, max_seq_len=per_req * P)
    base = _batcher_run(cb, op, case, case.ids)
    again = _batcher_run(cb, op, case, case.ids)
    for b in range(case.B):
        assert len(base["events"][b]) == len(again["events"][b]) >= 1
        for e, f in zip(base["events"][b], again["events"][b]):
            assert e[0] == f[0] and np.array_equal(e[1], f[1]) and np.array_equal(e[2], f[2])
    o_base, o_runs, _, fig = apc.reference(case)
    for b in range(case.B):  # the base run against the oracle (the rule of tests/test_gpu_rows.py _follows, on log-probabilities)
        n = int(case.lens[b])
        for t, (tok, ids, lps) in enumerate(base["events"][b]):
            ref = o_base["logits"][t, b]
            scale = apc.logit_range(ref)
            assert np.abs(lps - _log_softmax(ref)[ids]).max() <= 2 * LOGIT_FRAC * scale, (b, t)
            if tok != o_base["output_ids"][b, n + t]:
                top2 = np.sort(ref)[-2:]
                assert top2[1] - top2[0] < 2 * LOGIT_FRAC * scale, "token flip without a near tie"
                break
    pairs = got = live = live_lost = 0
    worst = 0.0
    for kinds, row, pos in case.forwards():
        probed = _batcher_run(cb, op, case, case.probed_ids(row, pos))
        o_probed = o_runs[(row, pos)]
        for kind in kinds:
            assert kind != "pad"  # (a request of the batcher has no padding)
            for b in case.observed(row, kind):
                pairs += case.out_len - 1
                eb, ep = base["events"][b], probed["events"][b]
                if kind == "live":
                    steps = [t for t in _agree(case, b, base, probed, o_base, o_probed) if t < min(len(eb), len(ep))]
                    live += 1
                    live_lost += not steps
                    for t in steps:
                        assert not (np.array_equal(eb[t][1], ep[t][1]) and np.array_equal(eb[t][2], ep[t][2])), ("a dead key", row, pos, t)
                        common = np.intersect1d(eb[t][1], ep[t][1])
                        assert len(common) >= TOP // 2
                        lp = lambda e: np.array([e[2][list(e[1]).index(i)] for i in common], np.float64)
                        d_gpu = lp(ep[t]) - lp(eb[t])
                        d_orc = _log_softmax(o_probed["logits"][t, b])[common] - _log_softmax(o_base["logits"][t, b])[common]
                        err = float(np.abs(d_gpu - d_orc).max()) / apc.logit_range(o_base["logits"][t, b])
                        worst = max(worst, err)
                        assert err <= 2 * LOGIT_FRAC, ("a key weighted wrongly", row, pos, t, err)
                    got += len(steps)
                else:
                    assert len(eb) == len(ep)
                    for e, f in zip(eb, ep):
                        assert e[0] == f[0] and np.array_equal(e[1], f[1]) and np.array_equal(e[2], f[2]), (kind, row, pos, b)
                    got += case.out_len - 1
    _check_caps(case, pairs, got, live, live_lost, worst, fig)
    assert cb.status()["running"] == 0 and cb.status()["waiting"] == 0
