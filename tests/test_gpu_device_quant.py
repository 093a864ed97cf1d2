"""-m gpu: the device form of the weight-only int8 quantiser (include/ftcf.h ftcf_symmetric_quantize_int8_device,
csrc/kernels_quant.hip) against the host quantiser ftcf_symmetric_quantize_int8 on the same values: the tiled q bytes and the
scale bits must be identical -- no mismatch is allowed anywhere.  Every kernel-level call here runs with its outputs and its
workspace inside buffers that carry 256 poisoned bytes on either side, which must stay untouched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from fastertransformer4codefuse_amd import capi, convert, harness
from fastertransformer4codefuse_amd.gptneox_op import (symmetric_quantize_last_axis_of_batched_matrix_int8 as host_quant,
                                                       symmetric_quantize_last_axis_of_batched_matrix_int8_device as dev_quant)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
CODE = {torch.float32: capi.FP32, torch.float16: capi.FP16, torch.bfloat16: capi.BF16}
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
GUARD, POISON = 256, 0xA5


def _guarded(nbytes):
    buf = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + GUARD


def _guards_intact(buf, nbytes):
    b = buf.cpu()
    return bool((b[:GUARD] == POISON).all()) and bool((b[GUARD + nbytes:] == POISON).all())


def ekn(w):
    return (1 if w.dim() == 2 else int(w.size(0))), int(w.size(-2)), int(w.size(-1))


def device_call(w_dev, stream=None):
    """ftcf_symmetric_quantize_int8_device on a device tensor, outputs and workspace between poisoned guards.
    Returns (q bytes [E*K*N] uint8, scale bits [E*N] int16/int32) on the CPU."""
    E, K, N = ekn(w_dev)
    L = capi.lib()
    es = w_dev.element_size()
    ws_bytes = int(L.ftcf_symmetric_quantize_int8_device_workspace(C.c_size_t(E), C.c_size_t(N)))
    assert ws_bytes == E * N * 4
    qb, qp = _guarded(E * K * N)
    sb, sp = _guarded(E * N * es)
    wb, wp = _guarded(ws_bytes)
    rc = L.ftcf_symmetric_quantize_int8_device(C.c_void_p(w_dev.data_ptr()), CODE[w_dev.dtype], C.c_size_t(E), C.c_size_t(K),
                                               C.c_size_t(N), C.c_void_p(qp), C.c_void_p(sp), C.c_void_p(wp),
                                               C.c_size_t(ws_bytes), C.c_void_p(stream))
    assert rc == 0, L.ftcf_last_error()
    torch.cuda.synchronize()
    assert _guards_intact(qb, E * K * N), "q guard bytes overwritten"
    assert _guards_intact(sb, E * N * es), "scale guard bytes overwritten"
    assert _guards_intact(wb, ws_bytes), "workspace guard bytes overwritten"
    q = qb[GUARD:GUARD + E * K * N].cpu()
    s = sb[GUARD:GUARD + E * N * es].cpu().view(BITS[w_dev.dtype])
    return q, s


def host_call(w):
    q, s = host_quant(w)
    return q.reshape(-1).view(torch.uint8), s.reshape(-1).view(BITS[w.dtype])


def check_exact(w):
    """device == host, bit for bit; returns the device result"""
    w = w.contiguous()
    hq, hs = host_call(w)
    dq, ds = device_call(w.cuda())
    bad_s = int((hs != ds).sum())
    bad_q = int((hq != dq).sum())
    print(f"shape {tuple(w.shape)} {w.dtype}: {bad_q} differing q bytes of {hq.numel()}, {bad_s} differing scales of {hs.numel()}")
    assert bad_s == 0, (bad_s, hs[hs != ds][:8], ds[hs != ds][:8])
    assert bad_q == 0, bad_q
    return dq, ds


def untile(q_bytes, K, N):
    """tiled u8 (q + 128) bytes of ONE matrix -> row-major int values [K, N]"""
    t = q_bytes.numpy().view(np.int8).copy()
    rm = np.empty(K * N, np.int8)
    i8p = C.POINTER(C.c_int8)
    capi.check(capi.lib().ftcf_int8_tiled_to_rowmajor(t.ctypes.data_as(i8p), C.c_size_t(K), C.c_size_t(N), rm.ctypes.data_as(i8p)))
    return rm.reshape(K, N).astype(np.int32)


def randn(shape, std, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_tile(dtype):
    check_exact(randn((64, 16), 0.05, 1, dtype))


def crafted(dtype):
    K, N = 320, 16
    w = torch.empty(K, N, dtype=torch.float32).uniform_(-0.5, 0.5, generator=torch.Generator().manual_seed(2))
    # 0: exact ties -- fp32 scale exactly 2^-10, rows 1..256 = (m + 0.5) * 2^-10
    w[:, 0] = 0.
    w[0, 0] = 0.125
    w[1:257, 0] = (torch.arange(-128, 128, dtype=torch.float32) + 0.5) * 2.0 ** -10
    w[:, 1] = 0.                                  # 1: all zero
    w[5, 2] = float("nan")                        # 2: one NaN among finite values
    w[3, 3], w[100, 3] = float("inf"), float("-inf")  # 3: one +Inf and one -Inf
    w[:, 4] *= 5.0e-5                             # 4: fp16 subnormals, max |w| = 3e-5 (fp16 scale bits 0x0004)
    w[17, 4] = 3.0e-5
    w[:, 5] = w[:, 5].clamp(-0.7, 0.7)            # 5: the maximum is negative and in the last row
    w[K - 1, 5] = -0.75
    return w.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_crafted_columns(dtype):
    w = crafted(dtype)
    K, N = w.shape
    dq, ds = check_exact(w)
    q = untile(dq, K, N)
    s = ds.view(dtype).float().numpy()
    wf = w.float().numpy()
    # exact ties: half away from zero, clamped
    m = np.arange(-128, 128)
    expect = np.where(m >= 0, np.minimum(m + 1, 127), m)
    assert q[0, 0] == 127 and s[0] == 2.0 ** -10
    assert q[1:257, 0].tolist() == expect.tolist()
    assert (q[257:, 0] == 0).all()
    # all-zero column: 0 / 0 -> 127 everywhere, scale 0
    assert (q[:, 1] == 127).all() and int(ds[1]) == 0
    # one NaN: not the maximum; its q is 127 and the rest quantise normally
    finite = np.delete(wf[:, 2], 5)
    cm = np.float32(np.abs(finite).max()) * np.float32(1 / 128)
    assert np.isfinite(s[2]) and s[2] == torch.tensor(cm).to(dtype).float().item()
    assert q[5, 2] == 127
    t = (finite.astype(np.float32) / cm).astype(np.float64)  # (the fp32 quotient; + 0.5 is exact in float64)
    ref = np.clip(np.sign(t) * np.floor(np.abs(t) + 0.5), -128, 127)
    assert np.delete(q[:, 2], 5).tolist() == ref.astype(np.int32).tolist()
    # +Inf and -Inf: scale Inf, Inf / Inf -> 127, finite / Inf -> 0
    assert np.isposinf(s[3]) and q[3, 3] == 127 and q[100, 3] == 127
    assert (np.delete(q[:, 3], [3, 100]) == 0).all()
    # fp16 subnormal column
    if dtype == torch.float16:
        assert int(ds[4]) == 0x0004
    assert q[17, 4] == 127
    # maximum negative and in the last row
    assert q[K - 1, 5] == -128 and s[5] == torch.tensor(0.75 / 128).to(dtype).float().item()


@pytest.mark.parametrize("shape", [(128, 48), (192, 80)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_n_not_a_multiple_of_64(shape, dtype):
    check_exact(randn(shape, 0.05, 3, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched(dtype):
    w = randn((3, 128, 32), 1.0, 4, torch.float32)
    w[0] *= 1e-3
    w[2] *= 40.
    check_exact(w.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_k_split(dtype):
    """every column's maximum sits at a different row, the first and the last row of the matrix among them"""
    K, N = 8192, 32
    w = randn((K, N), 0.25, 5, torch.float32).clamp(-1., 1.)
    rows = [0, K - 1, 63, 64, 127, 128, K // 2 - 1, K // 2] + [int(r) for r in np.linspace(200, K - 200, N - 8)]
    assert len(set(rows)) == N
    for j, r in enumerate(rows):
        w[r, j] = (2.0 + j / 16.) * (-1 if j % 2 else 1)
    w = w.to(dtype)
    dq, ds = check_exact(w)
    assert ds.view(dtype).float().tolist() == [torch.tensor((2.0 + j / 16.) / 128).to(dtype).float().item() for j in range(N)]


def test_one_real_k():
    check_exact(randn((5120, 2064), 0.02, 6, torch.float16))


def test_purity_and_repeatability():
    w = randn((2, 128, 48), 0.05, 7, torch.float16)
    wd = w.cuda()
    q1, s1 = device_call(wd)
    assert torch.equal(wd.cpu(), w), "the weight tensor was modified"
    q2, s2 = device_call(wd)
    assert torch.equal(q1, q2) and torch.equal(s1, s2)
    side = torch.cuda.Stream()  # and on a stream that is not the null stream
    side.wait_stream(torch.cuda.current_stream())
    q3, s3 = device_call(wd, stream=side.cuda_stream)
    assert torch.equal(q1, q3) and torch.equal(s1, s3)
    hq, hs = host_call(w)
    assert torch.equal(q1, hq) and torch.equal(s1, hs)


def test_argument_checks():
    L = capi.lib()
    w = torch.zeros(64 * 16, dtype=torch.float16, device="cuda")
    q = torch.zeros(64 * 16, dtype=torch.int8, device="cuda")
    s = torch.zeros(16, dtype=torch.float16, device="cuda")
    ws = torch.zeros(64, dtype=torch.uint8, device="cuda")

    def call(K=64, N=16, wp=w.data_ptr(), qp=q.data_ptr(), sp=s.data_ptr(), wsp=ws.data_ptr(), wsb=64, dt=capi.FP16, E=1):
        return L.ftcf_symmetric_quantize_int8_device(C.c_void_p(wp), dt, C.c_size_t(E), C.c_size_t(K), C.c_size_t(N), C.c_void_p(qp),
                                                     C.c_void_p(sp), C.c_void_p(wsp), C.c_size_t(wsb), None)

    assert call() == 0
    assert call(K=60) == -1 and b"K % 64" in L.ftcf_last_error()
    assert call(N=8) == -1
    assert call(wp=None) == -1 and call(qp=None) == -1 and call(sp=None) == -1 and call(wsp=None) == -1
    assert call(wsb=63) == -1 and b"workspace" in L.ftcf_last_error()
    assert call(dt=3) == -1
    assert call(E=0) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
def test_python_surfaces(dtype):
    import sys
    libdir = os.path.join(os.path.dirname(capi.LIB_PATH))
    if libdir not in sys.path:
        sys.path.append(libdir)
    import libth_common
    for shape in [(128, 48), (2, 64, 32)]:
        w = randn(shape, 0.05, 8, dtype)
        hq, hs = host_quant(w)
        forms = {"gptneox_op, device tensor": dev_quant(w.cuda()), "gptneox_op, CPU tensor": dev_quant(w),
                 "libth_common, device tensor": libth_common.symmetric_quantize_last_axis_of_batched_matrix_int8_device(w.cuda()),
                 "libth_common, CPU tensor": libth_common.symmetric_quantize_last_axis_of_batched_matrix_int8_device(w),
                 "torch.ops": torch.ops.fastertransformer.symmetric_quantize_last_axis_of_batched_matrix_int8_device(w.cuda())}
        for name, (q, s) in forms.items():
            assert q.is_cuda and s.is_cuda, name
            assert q.dtype == torch.int8 and s.dtype == dtype and q.shape == hq.shape and s.shape == hs.shape, name
            assert torch.equal(q.cpu(), hq), name
            assert torch.equal(s.cpu().view(BITS[dtype]), hs.view(BITS[dtype])), name
    with pytest.raises(RuntimeError):
        host_quant(w.cuda())  # the reference's surface keeps its CHECK_CPU
    with pytest.raises(RuntimeError):
        dev_quant(torch.zeros(4, device="cuda"))
    with pytest.raises(RuntimeError):
        dev_quant(torch.zeros((60, 16), dtype=torch.float16, device="cuda"))  # K % 64 != 0


@pytest.fixture(scope="module")
def tiny_checkpoint(tmp_path_factory):
    from tests.helpers import load_tiny
    from tests.test_gpu_cli import write_checkpoint
    cfg, w, z = load_tiny()
    d = tmp_path_factory.mktemp("ckpt") / "1-gpu"
    d.mkdir()
    write_checkpoint(str(d), cfg, w, 0)  # fp kernels on disk: the load quantises them
    return cfg, z, str(d)


def test_harness_load_on_device_equals_host_load(tiny_checkpoint):
    cfg, z, d = tiny_checkpoint
    models = []
    for on_device in (False, True):
        m = harness.GptNeoX(cfg["head_num"], cfg["size_per_head"], cfg["vocab_size"], cfg["rotary_dim"], cfg["start_id"],
                            cfg["end_id"], cfg["num_layer"], 1024, 1, 1, True, int8_mode=1, inference_data_type="fp16",
                            weights_data_type=np.float32, inter_size=cfg["inter_size"], quantize_on_device=on_device)
        assert m.load(d)
        models.append(m)
    a, b = models
    assert b.weights.quantize_on_device and not a.weights.quantize_on_device
    assert len(a.weights.int8_w) == len(b.weights.int8_w) == 4 * cfg["num_layer"]
    for x, y in zip(a.weights.int8_w, b.weights.int8_w):
        assert x.is_cuda and y.is_cuda and x.shape == y.shape and torch.equal(x, y)
    for x, y in zip(a.weights.scale, b.weights.scale):
        assert x.is_cuda and y.is_cuda and x.dtype == y.dtype == torch.float16 and torch.equal(x.view(torch.int16), y.view(torch.int16))
    for x, y in zip(a.weights.w, b.weights.w):
        assert x.shape == y.shape and torch.equal(x, y)
    ids = torch.from_numpy(np.asarray(z["prompt"], dtype=np.int32))[None, :]
    lens = torch.IntTensor([ids.size(1)])
    outs = [m(ids, lens, 8, top_k=torch.IntTensor([1])).cpu() for m in models]
    assert outs[0].shape[-1] == ids.size(1) + 8
    assert outs[0].tolist() == outs[1].tolist()


def test_quant_and_save_on_device_writes_the_same_files(tiny_checkpoint, tmp_path):
    cfg, z, d = tiny_checkpoint
    host_dir, dev_dir = str(tmp_path / "host"), str(tmp_path / "dev")
    convert.quant_and_save(d, host_dir, 1)
    convert.quant_and_save(d, dev_dir, 1, on_device=True)
    names = sorted(os.listdir(host_dir))
    assert names == sorted(os.listdir(dev_dir))
    assert sum(n.endswith(".q.bin") for n in names) == 4 * cfg["num_layer"] == sum(n.endswith(".s.bin") for n in names)
    for n in names:
        assert open(os.path.join(host_dir, n), "rb").read() == open(os.path.join(dev_dir, n), "rb").read(), n
