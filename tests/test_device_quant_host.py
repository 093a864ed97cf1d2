"""The device quantiser's surfaces on a host without a GPU (include/ftcf.h ftcf_symmetric_quantize_int8_device): the entry point
fails loudly, the workspace query is host arithmetic and still answers, and every layer exposes the new name."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from fastertransformer4codefuse_amd import capi, gptneox_op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "symmetric_quantize_last_axis_of_batched_matrix_int8_device"


def test_workspace_query_is_host_arithmetic():
    L = capi.lib()
    for E, N in [(1, 16), (3, 32), (1, 20480), (7, 5120)]:
        assert L.ftcf_symmetric_quantize_int8_device_workspace(C.c_size_t(E), C.c_size_t(N)) == E * N * 4
    hdr = open(os.path.join(ROOT, "include", "ftcf.h")).read()
    assert re.search(r"ftcf_symmetric_quantize_int8_device_workspace\(E, N\) = E \* N \* 4 bytes", hdr)


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_entry_point_fails_loudly_without_a_gpu():
    L = capi.lib()
    w = torch.zeros(64, 16, dtype=torch.float16)
    q = torch.zeros(64, 16, dtype=torch.int8)
    s = torch.zeros(16, dtype=torch.float16)
    ws = torch.zeros(64, dtype=torch.uint8)
    rc = L.ftcf_symmetric_quantize_int8_device(C.c_void_p(w.data_ptr()), capi.FP16, C.c_size_t(1), C.c_size_t(64), C.c_size_t(16),
                                               C.c_void_p(q.data_ptr()), C.c_void_p(s.data_ptr()), C.c_void_p(ws.data_ptr()),
                                               C.c_size_t(64), None)
    assert rc == -5 and b"no HIP device" in L.ftcf_last_error()
    with pytest.raises(capi.FtcfError) as e:
        gptneox_op.symmetric_quantize_last_axis_of_batched_matrix_int8_device(w)
    assert e.value.code == -5
    assert int(q.abs().sum()) == 0  # never a silent CPU fallback


def test_every_layer_exposes_the_new_name():
    assert callable(getattr(gptneox_op, NAME))
    assert "ftcf_symmetric_quantize_int8_device" in capi.EXPORTED
    assert "ftcf_symmetric_quantize_int8_device_workspace" in capi.EXPORTED
    libdir = os.path.dirname(capi.LIB_PATH)
    if libdir not in sys.path:
        sys.path.append(libdir)
    import libth_common
    assert callable(getattr(libth_common, NAME))
    assert hasattr(torch.ops.fastertransformer, NAME)
    # the shape and dtype checks come before anything touches a device
    with pytest.raises(RuntimeError):
        getattr(libth_common, NAME)(torch.zeros(4, dtype=torch.float16))
    with pytest.raises(RuntimeError):
        getattr(gptneox_op, NAME)(torch.zeros((64, 16), dtype=torch.int32))


def test_harness_and_converter_flags_default_off():
    import inspect
    from fastertransformer4codefuse_amd import convert, harness
    assert inspect.signature(harness.GptNeoXWeights.__init__).parameters["quantize_on_device"].default is False
    assert inspect.signature(harness.GptNeoX.__init__).parameters["quantize_on_device"].default is False
    assert inspect.signature(convert.quant_and_save).parameters["on_device"].default is False
    w = harness.GptNeoXWeights(4, 16, 1, 64, 128, 1, 1, True, int8_mode=1, inference_data_type="fp16")
    assert w.weight_transpose_calibrate_quantize is gptneox_op.symmetric_quantize_last_axis_of_batched_matrix_int8
    w = harness.GptNeoXWeights(4, 16, 1, 64, 128, 1, 1, True, int8_mode=1, inference_data_type="fp16", quantize_on_device=True)
    assert w.weight_transpose_calibrate_quantize is getattr(gptneox_op, NAME)
