"""-m "not gpu": the host side of the speculative scope switch -- ftcf_gptneox_set_speculative_scope and
ftcf_verify_accept are declared, exported and bound, ftcf_verify_accept_args is laid out as the compiled header lays it out, the
entry points on a box without a GPU, the harness passes the arguments through, and the two kernels of the pass's tail compile
for gfx950 without scratch."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from tests.test_capi_abi import CC, ROOT, check_mirror, declarations, header
from tests.test_kernel_resources import HIPCC, _resource_usage

INVALID_ARG, NO_DEVICE = -1, -5


def test_the_entry_points_are_declared_exported_and_bound():
    from fastertransformer4codefuse_amd import capi
    decl = declarations()
    L = capi.lib()
    for name, argtypes in (("ftcf_gptneox_set_speculative_scope", [C.c_void_p, C.c_int]), ("ftcf_verify_accept", [C.c_void_p, C.c_void_p])):
        assert name in decl and name in capi.EXPORTED and hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
    assert decl["ftcf_verify_accept"][1][0].startswith("const ftcf_verify_accept_args*")
    assert L.ftcf_version() == 100  # (a switch of the engine and a new entry point: no struct of a request changed)


def _tagged_fields(struct):
    body = re.search(r"typedef struct " + struct + r" \{([^}]*)\} " + struct + ";", header()).group(1)
    return [re.findall(r"\w+", piece)[-1] for decl in body.split(";") if decl.strip() for piece in decl.split(",")]


@pytest.mark.skipif(CC is None, reason="no C compiler")
def test_verify_accept_args_mirror_the_compiled_header(tmp_path):
    """The check of tests/test_capi_abi.py check_mirror -- the header's field names in its order, every offset, every size and the
    struct's size as the host C compiler lays them out -- for the struct the header declares with a tag (capi.TAGGED_STRUCTS)."""
    from fastertransformer4codefuse_amd import capi
    struct, cls = "ftcf_verify_accept_args", capi.TAGGED_STRUCTS["ftcf_verify_accept_args"]
    names = [n for n, _ in cls._fields_]
    assert names == _tagged_fields(struct) and names[0] == "struct_size"
    body = f'  printf("%zu", sizeof({struct}));\n'
    for n in names:
        body += f'  printf(" %zu %zu", offsetof({struct}, {n}), sizeof((({struct}*)0)->{n}));\n'
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftcf.h"\nint main(void) {\n' + body + '  printf(" %d\\n", FTCF_VERIFY_ACCEPT_WORKSPACE_BYTES);\n  return 0;\n}\n')
    out = subprocess.run([CC, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()]
    want = [C.sizeof(cls)]
    for n in names:
        want += [getattr(cls, n).offset, getattr(cls, n).size]
    assert got == want + [capi.VERIFY_ACCEPT_WORKSPACE_BYTES]
    # the structs of a request keep their layout: the switch is not a request field
    check_mirror("ftcf_forward_args")
    check_mirror("ftcf_forward_stats")
    assert [f for f, _ in capi.ForwardArgs._fields_][-3:] == ["speculative_tokens", "speculative_ngram", "draft_ids"]


def _accept_args(capi, buf, **kw):
    a = capi.VerifyAcceptArgs()
    a.struct_size = C.sizeof(capi.VerifyAcceptArgs)
    a.R, a.V, a.step, a.end_id, a.max_input_len, a.total_len = 2, 8, 3, 1, 2, 8
    p = C.addressof(buf)
    for name in ("logits", "draft", "output_ids", "finished", "seq_len", "workspace", "emitted", "accepted", "tokens"):
        setattr(a, name, p)
    a.workspace_bytes = capi.VERIFY_ACCEPT_WORKSPACE_BYTES
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_a_bad_scope_is_refused_and_the_kernel_entry_needs_a_device():
    from fastertransformer4codefuse_amd import capi
    L = capi.lib()
    # (no engine exists without a GPU: the handle is NULL here; tests/test_gpu_speculative_scope.py repeats this on an engine)
    for scope in (2, -1, 0, 1):
        assert L.ftcf_gptneox_set_speculative_scope(None, scope) == INVALID_ARG
    if capi.device_count() > 0:
        return  # a GPU is visible: tests/test_gpu_verify_accept.py covers the call
    buf = (C.c_int * 4096)()
    assert L.ftcf_verify_accept(C.byref(_accept_args(capi, buf)), None) == NO_DEVICE
    assert L.ftcf_verify_accept(None, None) == NO_DEVICE


class _Tensor:
    """what GptNeoX.forward needs of a tensor, without a device"""

    def __init__(self, t):
        self.t = t

    def size(self, i):
        return self.t.size(i)

    def cuda(self, device):
        return self


class _StubOp:
    def __init__(self):
        self.calls, self.scopes = [], []

    def set_speculative_scope(self, scope):
        self.scopes.append(scope)

    def forward(self, *args, **kw):
        self.calls.append((args, kw))
        return [torch.zeros((1, 1, 6), dtype=torch.int32), torch.zeros((1, 1), dtype=torch.int32), torch.zeros((1, 1))]


def _harness_model(op):
    from fastertransformer4codefuse_amd import harness
    g = harness.GptNeoX.__new__(harness.GptNeoX)
    torch.nn.Module.__init__(g)
    g.build_model, g.device, g.model, g.end_id = True, 0, op, 2
    return g


def test_the_harness_passes_the_arguments_through_a_stub_op():
    from fastertransformer4codefuse_amd import harness
    ids, lens = _Tensor(torch.zeros((1, 4), dtype=torch.int32)), _Tensor(torch.tensor([4], dtype=torch.int32))
    # defaults: the reference's positional call, no keyword, the scope untouched
    op = _StubOp()
    g = _harness_model(op)
    g.forward(ids, lens, 2, return_output_length=True, return_cum_log_probs=1)
    (args, kw), = op.calls
    assert kw == {} and len(args) == 15 and op.scopes == []
    # given: scope 1, then the arguments by name behind the same positional call
    g.forward(ids, lens, 2, return_cum_log_probs=1, callback=print, speculative_tokens=4, speculative_ngram=2)
    args2, kw2 = op.calls[1]
    assert kw2 == {"speculative_tokens": 4, "speculative_ngram": 2} and op.scopes == [1]
    assert len(args2) == 15 and args2[13] == 1 and args2[14] is print
    g.forward(ids, lens, 2, speculative_tokens=8)
    assert op.calls[2][1] == {"speculative_tokens": 8, "speculative_ngram": None} and op.scopes == [1, 1]
    # an op without the switch gets the reference's call
    old = _StubOp()
    g = _harness_model(old)
    g.model = type("Old", (), {"forward": old.forward})()
    g.forward(ids, lens, 2, speculative_tokens=4)
    assert old.calls[0][1] == {}

    # generate() and the batched-request path
    class Tok:
        def encode(self, text):
            return [5, 6, 7]

        def decode(self, ids):
            return "x" * len(ids)

    seen = []

    def gpt(**kw):
        seen.append(kw)
        return (torch.full((1, 1, 6), 9, dtype=torch.int32), torch.tensor([[6]]), torch.zeros((1, 1)))

    gpt.end_id = 2
    harness.generate(gpt, Tok(), ["a"], 3, 1)
    assert "speculative_tokens" not in seen[0] and "speculative_ngram" not in seen[0]
    harness.generate(gpt, Tok(), ["a"], 3, 1, top_k=1, speculative_tokens=4)
    assert seen[1]["speculative_tokens"] == 4 and seen[1]["speculative_ngram"] is None and seen[1]["return_cum_log_probs"] == 1
    request = {"prompts": [{"prompt": "a"}], "out_seq_length": 3}
    assert "speculative_tokens" not in harness.get_data_package(request, 7)
    pkg = harness.get_data_package(dict(request, speculative_tokens=4, speculative_ngram=2), 7)
    assert pkg["speculative_tokens"] == 4 and pkg["speculative_ngram"] == 2
    harness.generate(gpt, Tok(), **pkg)
    assert seen[2]["speculative_tokens"] == 4 and seen[2]["speculative_ngram"] == 2


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_the_tail_kernels_compile_without_scratch(tmp_path):
    kernels = {k: v for k, v in _resource_usage("kernels_verify.hip", [], tmp_path).items() if "k_verify_slices" in k or "k_verify_close" in k}
    assert len(kernels) == 2, sorted(kernels)
    for name, r in kernels.items():
        assert r.get("VGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
