"""CPU: bench.py's options.  A plain run does only what its headline figure needs; --full adds the end-to-end request, the
profiled roofline run with its PMC child and the CPU baseline, and the --no-* / --profile-steps options trim a --full run."""
import sys

import bench


def _parse(monkeypatch, *extra):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", *extra])
    return bench.parse()


def test_plain_run_skips_the_legs_beyond_the_headline(monkeypatch):
    a = _parse(monkeypatch)
    assert not a.full
    assert a.no_e2e and a.no_cpu_baseline and a.no_pmc and a.profile_steps == 0
    assert (a.steps, a.warmup) == (20, 5)


def test_full_run_keeps_every_leg(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not (a.no_e2e or a.no_cpu_baseline or a.no_pmc) and a.profile_steps == 48
    b = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--profile-steps", "0")
    assert b.no_cpu_baseline and b.profile_steps == 0 and not (b.no_e2e or b.no_pmc)
