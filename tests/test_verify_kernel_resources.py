"""Speculative decoding's verify attention holds R x 8 fp32 accumulators and a round of K / V rows per lane in registers (DESIGN.md
section 4g): a spilled register would put scratch traffic into the loop that streams the cached keys.  Both head sizes must compile
without spilling vector registers and without scratch (hipcc cross-compiles for gfx950 without a GPU), as the persistent kernels
must in tests/test_kernel_resources.py."""
import pytest

from tests.test_kernel_resources import HIPCC, _resource_usage


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_verify_kernels_compile_without_spills(tmp_path):
    kernels = _resource_usage("kernels_verify.hip", [], tmp_path)
    attn = {k: v for k, v in kernels.items() if "k_verify_attention" in k}
    assert len(attn) == 2, sorted(kernels)  # dh 64 and 128
    for name, r in kernels.items():
        assert r.get("VGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
