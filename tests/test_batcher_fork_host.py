"""The host share of the batcher's fork requests (n samples of one prompt from one prompt phase: ftcf_batcher_submit_n,
fastertransformer4codefuse_amd/csrc/batcher_sched.h) is plain C++: tools/check_batcher_fork.cc drives the scheduler
with random mixes of plain, beam and fork requests, under reservation and overcommit, with the prefix cache on and off, fake prompt
phases that fail at seeded points, and checks the page accounting, the ids and the rollbacks after every operation.  It runs twice,
once plain and once as a stand-alone program under the address and undefined-behaviour sanitizers.  The rest is the CPU-only
surface of the feature: the entry points are declared with their signatures, exported, and the Python batcher has them."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

from fastertransformer4codefuse_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastertransformer4codefuse_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
GEOMETRIES = 6


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    out = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", *flags, "-I" + CSRC, os.path.join(ROOT, "tools", "check_batcher_fork.cc"),
                          "-o", exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    return run.stdout


def _check_lines(stdout):
    lines = [l for l in stdout.splitlines() if ": ok," in l]
    assert len(lines) == GEOMETRIES, stdout
    kinds = set()
    for l in lines:
        m = re.search(r"fork admitted (\d+) failed (\d+) \(tail 0 / 1 / P-1: (\d+) / (\d+) / (\d+), with a hit (\d+)\), siblings (\d+), "
                      r"shared pages saved (\d+), siblings cancelled waiting (\d+), ended with the first token (\d+), refused (\d+), "
                      r"other admitted (\d+) failed (\d+), preemptions (\d+)", l)
        assert m, l
        ok, bad, t0, t1, tp, hits, sibs, saved, cancelled, ended, refused, others, others_bad, pre = map(int, m.groups())
        # fork admissions both succeeded and failed in this geometry, with every kind of tail, among other admissions
        assert ok > 0 and bad > 0 and t0 > 0 and t1 > 0 and tp > 0, l
        assert sibs > ok and saved > 0 and cancelled > 0 and ended > 0 and refused > 0 and others > 0 and others_bad > 0, l
        assert (hits > 0) == ("cache" in l) and (pre > 0) == ("overcommit" in l), l
        kinds.add(("cache" in l, "overcommit" in l))
    assert len(kinds) == 4, kinds  # reservation and overcommit, each with the cache on and off


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_fork_invariants_under_random_operations(tmp_path):
    _check_lines(_build_and_run(tmp_path, "check_batcher_fork", ["-O1"]))


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_fork_invariants_under_the_sanitizers(tmp_path):
    """the same host program (its own main, nothing preloaded) with -fsanitize=address,undefined"""
    _check_lines(_build_and_run(tmp_path, "check_batcher_fork_san",
                                ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def _declaration(hdr, name):
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_entry_points_are_declared_with_their_signatures_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ftcf.h")).read()
    assert _declaration(hdr, "ftcf_batcher_submit_n") == _declaration(hdr, "ftcf_batcher_submit_opts")[:-1] + [
        "int n_samples", "long* request_ids"]
    assert _declaration(hdr, "ftcf_batcher_fork_stats") == ["ftcf_batcher_t b", "long* requests", "long* siblings", "long* shared_pages",
                                                            "long* prompt_tokens_computed"]
    for name in ("ftcf_batcher_submit_n", "ftcf_batcher_fork_stats"):
        assert name in capi.EXPORTED and hasattr(capi.lib(), name), name
    assert capi.lib().ftcf_version() == 100


def test_the_python_batcher_has_submit_n_and_fork_stats():
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    sub = list(inspect.signature(ContinuousBatcher.submit).parameters)
    assert sub == ["self", "prompt_ids", "max_new_tokens", "top_k", "top_p", "temperature", "seed", "repetition_penalty", "stop_words",
                   "logit_bias", "bad_words", "presence_penalty", "frequency_penalty", "min_new_tokens"]
    sub_n = inspect.signature(ContinuousBatcher.submit_n).parameters
    assert list(sub_n) == sub[:3] + ["n"] + sub[3:]
    for name in sub[3:]:  # the same defaults, the logit processors keyword-only
        assert sub_n[name].default == inspect.signature(ContinuousBatcher.submit).parameters[name].default, name
        assert sub_n[name].kind == inspect.signature(ContinuousBatcher.submit).parameters[name].kind, name
    assert sub_n["n"].default is inspect.Parameter.empty
    assert callable(ContinuousBatcher.fork_stats)


def test_null_arguments_are_refused():
    L = capi.lib()
    assert L.ftcf_batcher_fork_stats(None, None, None, None, None) == -1 and b"NULL" in L.ftcf_last_error()
    assert L.ftcf_batcher_submit_n(None, None, 0, 1, 0, 0, 0, 0, 0, None, 0, None, 2, None) == -1 and b"NULL" in L.ftcf_last_error()
