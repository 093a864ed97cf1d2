"""CPU: the oracle itself has the single-key property that test_gpu_attention_probes.py asks of every decode path
(tests/attention_probe_cases.py): on every case a replaced live prompt token changes every decode step of its row, by at least
MIN_LIVE of the logit range at the first one; a replaced padding token or another row's token changes nothing, bit for bit; and
few enough histories part (MAX_LOST) for the GPU tests to be about keys and not about token flips."""
import numpy as np
import pytest

from tests import attention_probe_cases as apc

CASES = apc.cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_oracle_has_the_single_key_property(case):
    base, runs, reports, fig = apc.reference(case)
    print(case.name, fig)
    assert 1 <= fig["forwards"] <= apc.MAX_FORWARDS
    kinds = {k for _, _, k in case.probes}
    assert "live" in kinds and (case.B == 1 or "other_row" in kinds)
    for (row, pos, kind), rep in reports:
        run = runs[(row, pos)]
        if kind == "live":
            assert pos < case.lens[row]
            steps = rep[row]
            assert all(d > 0.0 for _, d in steps), (row, pos, steps)
            if steps:  # (a probe without its first decode step is counted by fig["live_lost"])
                assert steps[0][0] == 1 and steps[0][1] >= apc.MIN_LIVE * apc.logit_range(base["logits"][1, row]), (row, pos, steps[0])
        else:
            assert (case.lens[row] <= pos < case.S) if kind == "pad" else pos < case.lens[row]
            for b in case.observed(row, kind):
                assert np.array_equal(run["logits"][:, b], base["logits"][:, b]), (kind, row, pos, b)
                n = int(case.lens[b])
                assert np.array_equal(run["output_ids"][b, n:], base["output_ids"][b, n:]), (kind, row, pos, b)
    assert fig["lost"] <= apc.MAX_LOST and fig["live_lost"] <= apc.MAX_LOST, fig
    assert fig["min_gap"] >= apc.MIN_GAP, fig  # the engine's base run cannot part from the oracle's


def test_a_last_prompt_key_probe_survives_on_every_path_and_head_size():
    """The last prompt key is the newest cached key of the first decode step: the only probe that sees a key loop that stops one key
    early.  Its replacement usually changes the row's first generated token (through the residual stream) and the probe is lost; the
    pinned picks keep at least one of them per decode path and size_per_head."""
    alive = {}
    for case in CASES:
        _, _, reports, _ = apc.reference(case)
        for (row, pos, kind), rep in reports:
            if kind == "live" and pos == case.lens[row] - 1:
                key = (case.path, case.dh)
                alive[key] = alive.get(key, 0) + bool(rep[row])
    assert len(alive) == 10 and all(n >= 1 for n in alive.values()), alive


def test_probe_report_counts_decode_steps_while_the_histories_agree():
    case = [c for c in CASES if c.name == "persist2_dh64_i0_ragged"][0]
    V, out, n = case.cfg["vocab_size"], case.out_len, case.lens
    base = dict(output_ids=np.zeros((2, case.S + out), np.int32), logits=np.zeros((out, 2, V), np.float32))
    for b in range(2):
        base["output_ids"][b, n[b]:n[b] + out] = 10 + np.arange(out)
    probed = dict(output_ids=base["output_ids"].copy(), logits=base["logits"].copy())
    probed["logits"][:, 0, 5] = 0.25
    probed["output_ids"][0, n[0] + 3] = 99  # row 0 parts with its 4th generated token: steps 1..3 count, step 4 and later do not
    rep = apc.probe_report(base, probed, case, (0, 2, "live"))
    assert rep == {0: [(1, 0.25), (2, 0.25), (3, 0.25)]}
    rep = apc.probe_report(base, probed, case, (0, 2, "other_row"))
    assert rep == {1: [(t, 0.0) for t in range(1, out)]}
    assert sorted(apc.probe_report(base, probed, case, (1, 20, "pad"))) == [0, 1]
    base["output_ids"][1, n[1] + 1] = probed["output_ids"][1, n[1] + 1] = case.cfg["end_id"]  # nothing behind an end token
    assert apc.probe_report(base, probed, case, (0, 2, "other_row")) == {1: [(1, 0.0)]}
    lost, live_lost = apc.lost_fraction([((0, 2, "live"), {0: []}), ((0, 3, "live"), {0: [(1, 0.5)] * (out - 1)})], case)
    assert (lost, live_lost) == (0.5, 0.5)


def test_probe_positions_follow_the_rule():
    by_name = {c.name: c for c in CASES}
    short = by_name["persist1_dh64_i0_chunk32"]  # up to 64 keys: every position
    assert [(r, p) for r, p, k in short.probes if k == "live"] == [(0, p) for p in range(28)]
    ragged = by_name["persist2_dh64_i0_ragged"]
    assert {(r, p) for r, p, k in ragged.probes if k == "pad"} <= {(1, p) for p in range(27, 40)}
    assert {(r, p) for r, p, k in ragged.probes if k == "other_row"} == {(r, p) for r, p, k in ragged.probes if k == "live"}
    long = by_name["launches1_dh64_300keys"]  # both ends, both sides of every multiple of 64 and of 16 (as far as 64 requests go)
    pos = {p for _, p, k in long.probes if k == "live"}
    assert {0, 1, 298, 299} <= pos and all({m - 1, m} <= pos for m in range(64, 300, 64))
    assert sum({m - 1, m} <= pos for m in range(16, 300, 16)) >= 12 and len(pos) <= apc.MAX_FORWARDS
    for c in CASES:
        for (r, p), tok in c._new.items():
            assert 3 <= tok < c.cfg["vocab_size"] and tok != c.ids[r, p]
    assert apc.persist_chunk(1, 4, 64, 20) == (2, 16, False) and apc.persist_chunk(1, 4, 128, 36) == (2, 32, False)
    assert apc.persist_chunk(1, 4, 64, 20, 6) == (1, 32, False) and apc.persist_chunk(2, 4, 128, 267, 10) == (1, 272, True)
    assert apc.persist_chunk(1, 4, 128, 1552, 24) == (6, 272, True)
