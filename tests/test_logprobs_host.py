"""Host checks of the per-token log-probability feature: the new fused LM-head kernel, the sampling translation unit that
stores output_log_probs and the beam-search translation unit split off from it cross-compile for gfx950 without spills or
scratch (the method of tests/test_kernel_resources.py), the fused greedy LM head keeps its register budget, and the ctypes
ForwardArgs lays the two new fields out as the C header does."""
import os
import shutil
import subprocess

import pytest

from tests.test_kernel_resources import HIPCC, ROOT, _resource_usage


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_log_prob_kernel_compiles_without_spills(tmp_path):
    kernels = _resource_usage("kernels_logprob.hip", [], tmp_path)
    names = [k for k in kernels if "k_lm_head_logprob" in k]
    assert any("tiles" in k for k in names) and any("merge" in k for k in names), sorted(kernels)
    for name in names:
        r = kernels[name]
        assert r.get("VGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_sampling_kernels_compile_without_new_spills_and_lm_head_greedy_keeps_its_budget(tmp_path):
    kernels = _resource_usage("kernels_sampling.hip", [], tmp_path)
    # (beam search and the gather tree were part of that translation unit and are held to the same: no spill, no scratch)
    kernels.update(_resource_usage("kernels_beam.hip", [], tmp_path))
    for name in ("k_sample", "k_greedy_decode", "k_topk_decode", "k_lm_head_greedy", "k_decode_prep", "k_topk_stage1", "k_beam_rows",
                 "k_beam_batch", "k_tile_inputs", "k_gather_tree_beam"):
        assert any(name in k for k in kernels), name
    for k, r in kernels.items():
        if "k_lm_head_greedy" in k:
            continue
        assert r.get("VGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
    # k_lm_head_greedy: __launch_bounds__(256, 8) -- eight waves per SIMD leave 512 / 8 = 64 VGPRs a lane.  It spilled a few
    # VGPRs before the log-probability store was added (5 at one row, 11 at two): that must not grow
    before = {"ILi1E": 5, "ILi2E": 11}
    for k, r in kernels.items():
        if "k_lm_head_greedy" in k:
            assert r["VGPRs"] <= 64, (k, r)
            rows = next(t for t in before if t in k)
            assert r.get("VGPRs Spill", 0) <= before[rows], (k, r)


CC = shutil.which("gcc") or shutil.which("cc")


@pytest.mark.skipif(CC is None, reason="no C compiler")
def test_forward_args_offsets_match_the_header(tmp_path):
    from fastertransformer4codefuse_amd import capi
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftcf.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", offsetof(ftcf_forward_args, debug_logits), '
                   'offsetof(ftcf_forward_args, output_log_probs), offsetof(ftcf_forward_args, context_log_probs), '
                   'sizeof(ftcf_forward_args));\n  return 0;\n}\n')
    exe = str(tmp_path / "off")
    out = subprocess.run([CC, "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    dbg, olp, clp, size = (int(v) for v in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split())
    F = capi.ForwardArgs
    assert (F.debug_logits.offset, F.output_log_probs.offset, F.context_log_probs.offset) == (dbg, olp, clp)
    assert capi.C.sizeof(F) == size
    assert olp > dbg and clp > olp  # appended after the last existing field
