"""CPU: every crafted decode-step case (tests/decode_cases.py) is well-posed -- the oracle's fp32 step and the float64
statement of the layer (tests/decode_reference.py) agree on it, at a pinned seed whose draws keep clear of every boundary of
the walk -- before a GPU sees it.  Tokens, finished, sequence lengths and draw counters are exact; log-probabilities use the
tolerance of test_gpu_sampling_vocab.py."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import decode_cases as dc
from tests import decode_reference as ref

CASES = dc.sampling_cases()
LP_TOL = dc.LP_TOL


def test_every_case_has_a_pinned_seed():
    assert sorted(dc.SEEDS) == sorted(c.name for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_matches_float64_statement(case):
    seed = dc.SEEDS[case.name]
    want = case.reference(seed)
    margin = float(np.min(want["margin"]))
    assert margin > ref.MARGIN, f"pinned seed {seed}: margin {margin:.3e}"
    assert case.find_seed() == seed, "the pinned seed is not the first one from the case's base that clears the margin"
    got = dc.oracle_step(case, seed)
    np.testing.assert_array_equal(got["output_ids"], want["output_ids"])
    np.testing.assert_array_equal(got["finished"], want["finished"])
    np.testing.assert_array_equal(got["seq_len"], want["seq_len"])
    np.testing.assert_array_equal(got["draw_counter"], want["draw_counter"])
    if case.return_cum_log_probs or case.output_log_probs:
        np.testing.assert_allclose(got["cum_log_probs"], want["cum_log_probs"], **LP_TOL)
        # the step's own term (what output_log_probs receives), not only the running sum
        np.testing.assert_allclose(got["cum_log_probs"].astype(np.float64) - case.cum_log_probs, want["step_log_probs"], rtol=1e-4, atol=2e-4)
    else:
        np.testing.assert_array_equal(got["cum_log_probs"], case.cum_log_probs)


def test_uniform_is_the_oracles_draw_stream():
    lib = orc.lib()
    import ctypes as C
    lib.orc_uniform.restype = C.c_float
    for seed, draw in ((0, 0), (1, 0), (12345678901234567, 3), (2 ** 64 - 1, 2 ** 40 + 7), (977, 1)):
        assert ref.uniform(seed, draw) == float(lib.orc_uniform(C.c_uint64(seed), C.c_uint64(0), C.c_uint64(draw)))


BEAM_CASES = dc.beam_cases()
SCORE_TOL = dc.SCORE_TOL


@pytest.mark.parametrize("case", BEAM_CASES, ids=lambda c: c.name)
def test_oracle_beam_step_matches_float64_statement(case):
    want = case.reference()
    assert want["margin"] > ref.MARGIN, f"two different scores {want['margin']:.3e} apart decide a place"
    got = dc.oracle_beam_step(case)
    for key in ("output_ids", "parent_ids", "finished", "seq_len", "tgt_indir"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    np.testing.assert_allclose(got["cum_log_probs"], want["cum_log_probs"], **SCORE_TOL)
