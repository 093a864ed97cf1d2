"""The continuous batcher's overcommit policy (fastertransformer4codefuse_amd/csrc/batcher_sched.h, DESIGN.md §4e: pages on
demand, preemption of the latest arrival by swap, resume before admission) is plain C++: tools/check_batcher_preempt.cc drives it
with fake prompt phases, decode steps and swap copies and checks the page and host-page accounting, the request ids, the
victim rule and the drain bound after every operation.  It runs twice, once plain and once as a stand-alone program under the
address and undefined-behaviour sanitizers.  The rest is the CPU-only surface of the feature: the new entry points are declared,
exported and fail loudly without a device."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

from fastertransformer4codefuse_amd import capi
from tests.test_capi_abi import header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastertransformer4codefuse_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
NEW = ("ftcf_batcher_create_opts", "ftcf_batcher_preempt_stats", "ftcf_pages_pack", "ftcf_pages_unpack")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    out = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", *flags, "-I" + CSRC, os.path.join(ROOT, "tools", "check_batcher_preempt.cc"),
                          "-o", exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    return run.stdout


def _check_lines(stdout):
    lines = [l for l in stdout.splitlines() if ": ok," in l]
    assert len(lines) == 8, stdout
    exhausted = 0
    for l in lines:
        m = re.search(r"preemptions (\d+), resumes (\d+), resumes into another slot (\d+), (\d+) decode steps inside admissions, "
                      r"(\d+) evictions, (\d+) times without swap space", l)
        assert m, l
        pre, res, other, hooks, evictions, full = map(int, m.groups())
        assert pre > 0 and res > 0 and other > 0 and hooks > 0, l
        assert (evictions > 0) == ("cache" in l), l
        assert full == 0 or "swap" in l, l  # (only the geometries with a small swap space may run out of it)
        exhausted += full
    assert exhausted > 0, stdout


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_overcommit_invariants_under_random_operations(tmp_path):
    _check_lines(_build_and_run(tmp_path, "check_batcher_preempt", ["-O1"]))


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_overcommit_invariants_under_the_sanitizers(tmp_path):
    """the same host program (its own main, nothing preloaded) with -fsanitize=address,undefined"""
    _check_lines(_build_and_run(tmp_path, "check_batcher_preempt_san",
                                ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def test_the_new_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ftcf.h")).read()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in capi.EXPORTED and hasattr(capi.lib(), name), name
    assert "} ftcf_batcher_options;" in hdr
    fields = [n for n, _ in capi.BatcherOptions._fields_]
    assert fields == ["struct_size", "max_batch", "page_tokens", "num_pages", "max_seq_len", "prefix_cache", "overcommit", "swap_pages",
                      "swap_stage_bytes"]
    assert fields == header_fields("ftcf_batcher_options")
    assert capi.lib().ftcf_version() == 100


def test_the_python_batcher_takes_the_new_arguments():
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    params = inspect.signature(ContinuousBatcher.__init__).parameters
    assert params["overcommit"].default is False and params["swap_pages"].default == 0
    assert params["prefix_cache"].default is False
    assert callable(ContinuousBatcher.preempt_stats)


def test_a_wrong_struct_size_is_refused():
    L = capi.lib()
    engine = (C.c_char * 8)()  # (never dereferenced: the size is checked first)
    o = capi.BatcherOptions()
    o.max_batch, o.page_tokens, o.num_pages, o.max_seq_len, o.overcommit = 2, 8, 8, 32, 1
    out = C.c_void_p()
    for size in (0, C.sizeof(capi.BatcherOptions) - 4, C.sizeof(capi.BatcherOptions) + 8):
        o.struct_size = size
        rc = L.ftcf_batcher_create_opts(C.cast(engine, C.c_void_p), C.byref(o), C.byref(out))
        assert rc == -1 and b"struct_size" in L.ftcf_last_error() and not out.value, size
    assert L.ftcf_batcher_create_opts(C.cast(engine, C.c_void_p), None, C.byref(out)) == -1


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_the_new_entry_points_fail_loudly_without_a_gpu():
    L = capi.lib()
    engine, buf = (C.c_char * 8)(), (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    o = capi.BatcherOptions()
    o.struct_size = C.sizeof(capi.BatcherOptions)
    o.max_batch, o.page_tokens, o.num_pages, o.max_seq_len, o.overcommit = 2, 8, 8, 32, 1
    out = C.c_void_p()
    calls = [
        lambda: L.ftcf_batcher_create_opts(C.cast(engine, C.c_void_p), C.byref(o), C.byref(out)),
        lambda: L.ftcf_batcher_preempt_stats(None, None, None, None, None, None, None, None, None),
        lambda: L.ftcf_pages_pack(p, p, p, p, 1, 2, 2, 64, 8, C.c_size_t(8 * 2 * 8 * 64), None),
        lambda: L.ftcf_pages_unpack(p, p, p, p, 1, 2, 2, 64, 8, C.c_size_t(8 * 2 * 8 * 64), None),
    ]
    for call in calls:
        assert call() == -5 and b"no HIP device" in L.ftcf_last_error()
    assert not out.value
