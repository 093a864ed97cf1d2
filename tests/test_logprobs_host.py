"""Host checks of the per-token log-probability feature: the new fused LM-head kernel, the sampling translation unit that
stores output_log_probs and the beam-search translation unit split off from it cross-compile for gfx950 without spills or
scratch (the method of tests/test_kernel_resources.py), the fused greedy LM head keeps its register budget, and the ctypes
ForwardArgs lays the two new fields out as the C header does."""
import pytest

from tests.test_capi_abi import CC, check_mirror
from tests.test_kernel_resources import HIPCC, _resource_usage


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


@pytest.mark.skipif(CC is None, reason="no C compiler")
def test_forward_args_offsets_match_the_header():
    from fastertransformer4codefuse_amd import capi
    check_mirror("ftcf_forward_args")  # (every field's offset and size and the struct's size: tests/test_capi_abi.py)
    F = capi.ForwardArgs
    dbg, olp, clp = F.debug_logits.offset, F.output_log_probs.offset, F.context_log_probs.offset
    assert olp > dbg and clp > olp  # appended after the last existing field
