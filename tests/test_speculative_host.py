"""-m "not gpu": the host side of speculative decoding -- the ctypes mirror of the fields appended to ftcf_forward_args /
ftcf_forward_stats against a struct compiled from include/ftcf.h, the new entry points on a box without a GPU, and the
Python-side argument validation."""
import ctypes as C

import pytest
import torch

from tests.test_capi_abi import CC, check_mirror

ARGS = ("context_log_probs", "speculative_tokens", "speculative_ngram", "draft_ids")
STATS = ("persist_layout", "spec_active", "spec_steps", "spec_drafted", "spec_accepted")


@pytest.mark.skipif(CC is None, reason="no C compiler")
def test_ctypes_mirror_matches_the_header():
    from fastertransformer4codefuse_amd import capi
    check_mirror("ftcf_forward_args")  # (every field's offset and size and the struct's size: tests/test_capi_abi.py)
    check_mirror("ftcf_forward_stats")
    # appended in the header's order, behind everything that was there
    names = [f for f, _ in capi.ForwardArgs._fields_]
    assert names[-4:] == list(ARGS)
    assert [f for f, _ in capi.ForwardStats._fields_][-5:] == list(STATS)


def test_new_entry_points_are_exported_and_need_a_device():
    from fastertransformer4codefuse_amd import capi
    for name in ("ftcf_verify_attention", "ftcf_verify_attention_workspace", "ftcf_ngram_draft"):
        assert name in capi.EXPORTED and hasattr(capi.lib(), name)
    assert capi.lib().ftcf_version() == 100
    assert capi.lib().ftcf_verify_attention_workspace(16, 40, 128, 1536) > 0  # (pure host arithmetic)
    if capi.device_count() > 0:
        return  # a GPU is visible: the kernel tests cover the calls
    buf = (C.c_int * 64)()
    assert capi.lib().ftcf_ngram_draft(buf, 4, 2, 3, buf, buf, None) == -5  # FTCF_ERR_NO_DEVICE
    assert capi.lib().ftcf_verify_attention(buf, None, buf, buf, 0, 0, 1, 1, 64, 0, 8, buf, buf, C.c_size_t(256), None) == -5


def test_python_argument_validation_needs_no_gpu():
    from fastertransformer4codefuse_amd.gptneox_op import check_speculative_args
    assert check_speculative_args(None, None, None, 8) == (0, 0)
    assert check_speculative_args(4, None, None, 8) == (4, 0)
    assert check_speculative_args(15, 8, None, 8) == (15, 8)
    for k, n in ((16, 0), (-1, 0), (4, 9), (4, -1)):
        with pytest.raises(RuntimeError):
            check_speculative_args(k, n, None, 8)
    good = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        check_speculative_args(0, 0, good, 8)  # drafts without speculation
    with pytest.raises(RuntimeError):
        check_speculative_args(4, 0, good.to(torch.int64), 8)
    with pytest.raises(RuntimeError):
        check_speculative_args(4, 0, torch.zeros(7, dtype=torch.int32), 8)
    with pytest.raises(RuntimeError):
        check_speculative_args(4, 0, good, 8)  # a host tensor
