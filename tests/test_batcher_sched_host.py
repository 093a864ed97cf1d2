"""The continuous batcher's host state (fastertransformer4codefuse_amd/csrc/batcher_sched.h, DESIGN.md §4f: queue, slots, page
accounting, admission policy, rollback) is plain C++: tools/check_batcher_sched.cc drives it with a fake prompt phase that takes
pages as the real admissions do and throws at seeded points, and checks after every operation that page references equal their
holders, that promises never exceed the pool, that a failed admission of any kind leaves the queue in order and nothing behind,
and that take_page never finds the pool empty.  The same program under the sanitizers:
g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all -Ifastertransformer4codefuse_amd/csrc
tools/check_batcher_sched.cc -o check_batcher_sched_san && ./check_batcher_sched_san"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastertransformer4codefuse_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
KINDS = ("beam", "hit", "chunked_one", "ragged")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_scheduler_invariants_under_random_operations_and_failed_admissions(tmp_path):
    exe = str(tmp_path / "check_batcher_sched")
    out = subprocess.run([CXX, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tools", "check_batcher_sched.cc"),
                          "-o", exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:]
    lines = [l for l in run.stdout.splitlines() if ": ok," in l]
    assert len(lines) == 8, run.stdout
    for l in lines:  # every geometry really admitted, and failed to admit, every kind it can produce (a hit needs the cache)
        m = re.search(r"admitted (.*), failed (.*?), (\d+) decode steps inside admissions", l)
        assert m, l
        for part in m.group(1, 2):
            counts = dict(re.findall(r"(\w+) (\d+)", part))
            for kind in KINDS:
                assert (int(counts[kind]) > 0) == (kind != "hit" or "cache" in l), l
        assert int(m.group(3)) > 0, l
