"""The continuous batcher's prefix index (fastertransformer4codefuse_amd/csrc/prefix_index.h) is plain C++:
tools/check_prefix_index.cc replays random admit / finish / evict / clear sequences against it on the host and checks that
references equal their holders, that only unreferenced leaves are evicted (least recently used first), that no chain exists
twice and that a lookup never serves K/V computed for other tokens."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastertransformer4codefuse_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_prefix_index_invariants_under_random_operations(tmp_path):
    exe = str(tmp_path / "check_prefix_index")
    out = subprocess.run([CXX, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tools", "check_prefix_index.cc"),
                          "-o", exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:]
    lines = [l for l in run.stdout.splitlines() if ": ok," in l]
    assert len(lines) == 8, run.stdout
    for l in lines:  # every configuration really exercised hits and evictions
        assert " 0 evictions" not in l and "(0 with a hit)" not in l, l
