"""CPU (-m "not gpu"): the float64 statement of top_logprobs (tests/top_logprobs_reference.py) is well-posed on every case of
tests/decode_cases.py at N = 1, 5 and 20, so that tests/test_gpu_top_logprobs_step.py can hold the kernels to exact ids.

(a) Exact ties are ordered by id, masked entries follow every other entry by id, V < N pads with (-1, -inf).
(b) Rows of the top-p layer are found as fp32 probabilities: two different neighbouring values among the first N + 1
    unmasked entries that are closer than LP_TOL's atol cannot be told apart there.  Such positions are excused (they may
    swap in the GPU test).
(c) On such rows the first N + 1 unmasked entries must lie above exp(-80), below which an fp32 probability is 0; a case that
    breaks this is left out for its top-p rows: ONE_HOT (a logit 80 above the rest of the row).
Excused positions plus the positions of left-out rows must stay under 1 % of the compared positions: the case list is one the
reference alone can be held to."""
import numpy as np

from tests import decode_cases as dc
from tests import top_logprobs_reference as tlp

CASES = dc.sampling_cases()
LEFT_OUT = {"one_hot_p0.9"}  # (c): every other entry of the row is a probability of 0 in fp32


def test_reference_is_well_posed_on_every_case():
    compared = excused = left_out = ties = 0
    broke_c = set()
    for case in CASES:
        for N in tlp.NS:
            for b, r in enumerate(case_rows(case, N)):
                if r is None:
                    continue
                ids, vals, row = r["ids"], r["log_probs"], r["row"]
                n = min(N, case.V)
                assert (ids[n:] == -1).all() and np.isneginf(vals[n:]).all()
                assert len(set(ids[:n].tolist())) == n and (ids[:n] >= 0).all() and (ids[:n] < case.V).all()
                live = np.isfinite(vals[:n])
                assert not live[np.argmin(live):].any() if not live.all() else True, "a masked entry before a live one"
                for j in range(n - 1):
                    if live[j] and live[j + 1]:
                        assert row[ids[j]] >= row[ids[j + 1]] and vals[j] >= vals[j + 1]
                        if row[ids[j]] == row[ids[j + 1]]:  # (a): -0.0 == +0.0 is such a tie
                            ties += 1
                            assert ids[j] < ids[j + 1], (case.name, N, b, j)
                    elif not live[j]:
                        assert ids[j] < ids[j + 1], "masked entries by id"
                # nothing outside the list beats its last live entry
                if live.any():
                    last = int(np.nonzero(live)[0][-1])
                    rest = np.ones(case.V, bool)
                    rest[ids[:n]] = False
                    rest &= row > -tlp.ref.FLT_MAX
                    if rest.any():
                        assert last == n - 1 and row[rest].max() <= row[ids[last]]
                        better = np.nonzero(rest & (row == row[ids[last]]))[0]
                        assert better.size == 0 or better.min() > ids[last]
                if r["topp"] and not r["well_posed"]:
                    broke_c.add(case.name)
                    left_out += n
                    continue
                compared += n
                excused += int(r["excused"][:n].sum())
                if not r["topp"]:
                    assert not r["excused"].any()
    print(f"compared {compared} positions, excused {excused}, left out {left_out}, exact ties between neighbours {ties}")
    assert broke_c == LEFT_OUT, broke_c
    assert ties > 1000, "the tie rule is not exercised"
    assert excused + left_out < 0.01 * compared, (excused, left_out, compared)


def case_rows(case, N):
    return tlp.case_top_n(case, N, atol=dc.LP_TOL["atol"])


def test_reference_known_answers():
    row = np.array([0.5, -np.inf, 2.0, 2.0, -tlp.ref.FLT_MAX, -0.0, 0.0], np.float64)
    r = tlp.top_n(row, 8)
    assert r["ids"].tolist() == [2, 3, 0, 5, 6, 1, 4, -1]
    den = 2 * np.exp(0.0) + np.exp(-1.5) + 2 * np.exp(-2.0) + 1e-6
    np.testing.assert_allclose(r["log_probs"][:5], np.array([0.0, 0.0, -1.5, -2.0, -2.0]) - np.log(den), rtol=1e-12)
    assert np.isneginf(r["log_probs"][5:]).all()
    # a top-p row: 1.0 and 1.0 + 1e-4 are closer than the tolerance and may swap; the entry below exp(-80) makes it ill-posed
    r = tlp.top_n(np.array([1.0, 3.0, 1.0001, -5.0]), 2, topp=True)
    assert r["ids"].tolist() == [1, 2] and r["excused"].tolist() == [False, True] and r["clusters"][1] == [2, 0] and r["well_posed"]
    assert not tlp.top_n(np.array([1.0, 100.0, 1.5]), 1, topp=True)["well_posed"]
