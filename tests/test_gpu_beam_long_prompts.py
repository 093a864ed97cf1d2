"""-m gpu: beam search on prompts longer than one KV split of the decode attention, step by step against the oracle.

The other beam tests keep max_input_len + output_len <= 64 (one split, the all-in-registers form) and compare tokens and cumulative
log-probabilities.  Here the requests of tests/beam_long_prompt_cases.py (3 to 6 splits, indirected loads in every split, one
request in the looped form, one with half of its keys generated, dh 64 and 128, fp16 and int8 weights, a narrow request after a wide
one on the same engine) are compared LOGIT by logit: the GPU's logits and the oracle's are both replayed through the oracle's
beam-search layer; a step of a batch entry is comparable while everything the two searches selected before it -- tokens and parents
of its K slots -- agrees, and on a comparable step every slot that was not finished before it has
max |gpu - oracle| <= LOGIT_FRAC x max |oracle| over its logits.  The GPU's own tokens stay exact under the replay of its logits.
So that the test cannot pass empty: three quarters of all (request, entry, step) triples are compared, in every request the
first three steps with generated keys are, and in every request some compared step follows a reordering of the beams."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine library: see tests/test_gpu_engine.py)

from tests import beam_long_prompt_cases as cases
from tests.beam_long_prompt_cases import LOGIT_FRAC, REQUESTS

pytestmark = pytest.mark.gpu

_oracle = {}


@pytest.fixture(scope="module")
def gh():
    from tests import gpu_helpers
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    return gpu_helpers


def _oracle_run(name):
    if name not in _oracle:
        _oracle[name] = cases.oracle_run(name)
    return _oracle[name]


def _comparable(tg, to, rows, steps):
    """the number of leading steps of a batch entry before which the two searches selected the same tokens and parents"""
    n = 0
    for t in range(steps):
        if t > 0 and not (np.array_equal(tg["ids"][t - 1][rows], to["ids"][t - 1][rows])
                          and np.array_equal(tg["parents"][t - 1][rows], to["parents"][t - 1][rows])):
            break  # their rows no longer hold the same histories
        n += 1
    return n


def _compare(label, name, gpu):
    r = REQUESTS[name]
    B, K, out = r["B"], r["K"], r["out"]
    o = _oracle_run(name)
    g_ids, tg = cases.replay(name, gpu["logits"])
    _, to = cases.replay(name, o["logits"])
    assert gpu["output_ids"].tolist() == g_ids.tolist()  # exact given the GPU's own logits
    steps = min(len(tg["ids"]), len(to["ids"]))
    compared, worst, reordered = 0, 0.0, False
    for e in range(B):
        rows = np.arange(e * K, (e + 1) * K)
        n = _comparable(tg, to, rows, steps)
        for t in range(n):
            assert np.array_equal(tg["finished"][t][rows], to["finished"][t][rows])
            for s in rows[to["finished"][t][rows] == 0]:
                err = float(np.abs(gpu["logits"][t, s] - o["logits"][t, s]).max() / np.abs(o["logits"][t, s]).max())
                worst = max(worst, err)
                assert err <= LOGIT_FRAC, (label, "entry", e, "step", t, "slot", int(s), err)
            # the keys step t read were gathered through the parents of the steps before it.  Step 0 does not count: it expands
            # beam 0 only (every parent is 0), and the key it appends is the same in every beam
            reordered |= bool((to["parents"][1:t][:, rows] % K != np.arange(K)).any())
        assert n >= 4, (label, "entry", e, "the first three steps with generated keys (1, 2, 3) are not all compared", n)
        compared += n
    assert reordered, (label, "no compared step follows a reordering of the beams")
    print(f"[{label}: {compared} of {B * out} steps compared, worst logit error {worst:.2e}] ", end="")
    return compared, B * out, worst


def _engine_run(gh, name, op=None):
    from tests.beam_long_prompt_worker import run
    return run(gh, name, op)


def _child_run(name, **env):
    """the request in a fresh child process with the given switches (read once per process): one run with a timeout, no exec"""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "run.npz")
        subprocess.run([sys.executable, "-m", "tests.beam_long_prompt_worker", name, out], env=dict(os.environ, **env), check=True,
                       timeout=300, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        z = np.load(out)
        return {k: z[k] for k in z.files}


def _wide_then_narrow(gh):
    wide, op = _engine_run(gh, "a")
    first = _compare("f (wide)", "a", wide)
    second = _compare("f (narrow)", "f2", _engine_run(gh, "f2", op)[0])
    return first[0] + second[0], first[1] + second[1], max(first[2], second[2])


@pytest.fixture(scope="module")
def results(gh):
    """every request run once: label -> (steps compared, steps in all, worst logit error), or the exception that ended it"""
    runs = [(name, lambda name=name: _compare(name, name, _engine_run(gh, name)[0])) for name in ("a", "b", "d", "e_fp16", "e_int8")]
    runs.append(("c", lambda: _compare("c", "b", _child_run("b", FTCF_MMHA_WGS="1"))))
    runs.append(("f", lambda: _wide_then_narrow(gh)))
    res = {}
    for label, run in runs:
        try:
            res[label] = run()
        except Exception as e:  # shown by the test of that request, and by test_enough_steps_were_compared
            res[label] = e
    return res


def _result(results, label):
    if isinstance(results[label], Exception):
        raise results[label]
    return results[label]


@pytest.mark.parametrize("name", ["a", "b", "d", "e_fp16", "e_int8"])
def test_long_prompt_beams_follow_the_oracle_logit_by_logit(results, name):
    _result(results, name)


def test_looped_form_in_a_child_process(results):
    """request b with FTCF_MMHA_WGS=1: one split of 338 keys, the looped form with the indirection"""
    _result(results, "c")


def test_narrow_request_after_a_wide_one_on_the_same_engine(results):
    """K = 4 then K = 2 on one engine: the indirection entries the wider request left behind must not reach the narrow one"""
    _result(results, "f")


def test_enough_steps_were_compared(results):
    """three quarters of all (request, entry, step) triples, over the requests above"""
    got = [_result(results, label) for label in results]
    compared, total = sum(v[0] for v in got), sum(v[1] for v in got)
    print(f"[{compared} of {total} triples compared, worst logit error {max(v[2] for v in got):.2e}] ", end="")
    assert 4 * compared >= 3 * total, (compared, total, dict(zip(results, got)))
