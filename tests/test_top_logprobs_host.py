"""CPU (-m "not gpu"): the top_logprobs surface of the C ABI -- the fields added to ftcf_forward_args (with the log-probability
outputs, behind output_log_probs: the speculative fields stay the struct's last ones) and appended to
ftcf_dynamic_decode_args sit in the ctypes structs where the C header puts them, ftcf_batcher_step_top is declared, exported
and bound, the Python entry points take the argument, and the two new kernels are in the sampling translation unit without scratch."""
import inspect
import os

import pytest

from fastertransformer4codefuse_amd import capi
from tests.test_capi_abi import CC, check_mirror
from tests.test_kernel_resources import HIPCC, ROOT, _resource_usage

FIELDS = {
    "ftcf_forward_args": (capi.ForwardArgs, ("output_log_probs", "top_logprobs", "top_logprob_ids", "top_logprob_values",
                                             "context_log_probs", "speculative_tokens", "speculative_ngram", "draft_ids")),
    "ftcf_dynamic_decode_args": (capi.DynamicDecodeArgs, ("finish", "top_logprobs", "top_ids", "top_log_probs")),
}


@pytest.mark.skipif(CC is None, reason="no C compiler")
def test_struct_offsets_match_the_header():
    for struct, (cls, names) in FIELDS.items():
        check_mirror(struct)  # (every field's offset and size and the struct's size: tests/test_capi_abi.py)
        offs = [getattr(cls, n).offset for n in names]
        assert offs == sorted(offs) and len(set(offs)) == len(offs), "in the header's order"
        fields = [f[0] for f in cls._fields_]
        assert fields[-(len(names) - 1):] == list(names[1:]) and fields[-len(names)] == names[0], "the struct's tail, in order"


def test_step_top_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ftcf.h")).read()
    assert "int ftcf_batcher_step_top(ftcf_batcher_t b, long* request_ids, int* tokens, int* finished, float* log_probs, int top_n" in hdr
    assert "ftcf_batcher_step_top" in capi.EXPORTED and hasattr(capi.lib(), "ftcf_batcher_step_top")
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    from fastertransformer4codefuse_amd.gptneox_op import GptNeoXOp
    assert "top_logprobs" in inspect.signature(ContinuousBatcher.step).parameters
    assert "top_logprobs" in inspect.signature(GptNeoXOp.forward).parameters
    # zero-initialised arguments ask for nothing
    assert capi.ForwardArgs().top_logprobs == 0 and not capi.ForwardArgs().top_logprob_ids
    assert capi.DynamicDecodeArgs().top_logprobs == 0 and not capi.DynamicDecodeArgs().top_ids


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_top_logprobs_kernels_compile_without_scratch(tmp_path):
    kernels = _resource_usage("kernels_sampling.hip", [], tmp_path)
    for name in ("k_top_logprobs_slices", "k_top_logprobs_merge"):
        found = [k for k in kernels if name in k]
        assert found, (name, sorted(kernels))
        for k in found:
            r = kernels[k]
            assert r.get("VGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
    kernels = _resource_usage("kernels_logprob.hip", [], tmp_path)
    for name in ("k_fill_top_logprobs", "k_transpose_top_logprobs"):
        assert any(name in k for k in kernels), name
