"""-m "not gpu": the host side of speculative decoding for top-k sampled requests --
ftcf_gptneox_set_speculative_sampling and ftcf_verify_sample are declared, exported and bound, ftcf_verify_sample_args is laid out
as the compiled header lays it out, the entry points on a box without a GPU, the harness switches both engine switches on, the
three kernels of the sampled tail compile for gfx950 without spill or scratch, and every request of
tests/speculative_sampled_cases.py is stable on the CPU oracle (the rule is stated there)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from tests import speculative_sampled_cases as sc
from tests.test_capi_abi import CC, ROOT, check_mirror, declarations
from tests.test_kernel_resources import HIPCC, _resource_usage
from tests.test_speculative_scope_host import _StubOp, _Tensor, _harness_model, _tagged_fields

INVALID_ARG, NO_DEVICE = -1, -5


def test_the_entry_points_are_declared_exported_and_bound():
    from fastertransformer4codefuse_amd import capi
    decl = declarations()
    L = capi.lib()
    for name, argtypes in (("ftcf_gptneox_set_speculative_sampling", [C.c_void_p, C.c_int]), ("ftcf_verify_sample", [C.c_void_p, C.c_void_p])):
        assert name in decl and name in capi.EXPORTED and hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
    assert decl["ftcf_verify_sample"][1][0].startswith("const ftcf_verify_sample_args*")
    assert L.ftcf_version() == 100  # (a switch of the engine and a new entry point: no struct of a request changed)


@pytest.mark.skipif(CC is None, reason="no C compiler")
def test_verify_sample_args_mirror_the_compiled_header(tmp_path):
    """check_mirror's check (tests/test_capi_abi.py) for the struct the header declares with a tag (capi.TAGGED_STRUCTS): the
    header's field names in its order, every offset, every size, the struct's size and the workspace macro; its head is
    ftcf_verify_accept_args field for field."""
    from fastertransformer4codefuse_amd import capi
    struct, cls = "ftcf_verify_sample_args", capi.TAGGED_STRUCTS["ftcf_verify_sample_args"]
    names = [n for n, _ in cls._fields_]
    assert names == _tagged_fields(struct) and names[0] == "struct_size"
    head = [n for n, _ in capi.VerifyAcceptArgs._fields_]
    assert names[:len(head)] == head and names[len(head):] == ["top_k", "top_p_topk", "temperature", "random_seed", "draw_counter"]
    assert all(getattr(cls, n).offset == getattr(capi.VerifyAcceptArgs, n).offset for n in head)
    body = f'  printf("%zu", sizeof({struct}));\n'
    for n in names:
        body += f'  printf(" %zu %zu", offsetof({struct}, {n}), sizeof((({struct}*)0)->{n}));\n'
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ftcf.h"\nint main(void) {\n' + body
                   + '  printf(" %d\\n", FTCF_VERIFY_SAMPLE_WORKSPACE_BYTES);\n  return 0;\n}\n')
    out = subprocess.run([CC, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()]
    want = [C.sizeof(cls)]
    for n in names:
        want += [getattr(cls, n).offset, getattr(cls, n).size]
    assert got == want + [capi.VERIFY_SAMPLE_WORKSPACE_BYTES]
    # candidates {value, id} of 16 rows x 32 slices x 64, {max, sum} per slice, {token, log-probability} per row
    assert capi.VERIFY_SAMPLE_WORKSPACE_BYTES == 4 * (2 * 16 * 32 * 64 + 16 * 32 * 2 + 16 * 2)
    # the structs of a request keep their layout: the switch is not a request field
    check_mirror("ftcf_forward_args")
    check_mirror("ftcf_forward_stats")


def test_a_bad_switch_is_refused_and_the_kernel_entry_needs_a_device():
    from fastertransformer4codefuse_amd import capi
    L = capi.lib()
    # (no engine exists without a GPU: the handle is NULL here; tests/test_gpu_speculative_sampled.py repeats this on an engine)
    for v in (2, -1, 0, 1):
        assert L.ftcf_gptneox_set_speculative_sampling(None, v) == INVALID_ARG
    if capi.device_count() > 0:
        return  # a GPU is visible: tests/test_gpu_verify_sample.py covers the call
    buf = (C.c_int * 4096)()
    a = capi.VerifySampleArgs()
    a.struct_size = C.sizeof(capi.VerifySampleArgs)
    a.R, a.V, a.step, a.end_id, a.max_input_len, a.total_len = 2, 8, 3, 1, 2, 8
    for name in ("logits", "draft", "output_ids", "finished", "seq_len", "workspace", "emitted", "accepted", "tokens", "draw_counter"):
        setattr(a, name, C.addressof(buf))
    a.workspace_bytes, a.top_k, a.top_p_topk, a.temperature = capi.VERIFY_SAMPLE_WORKSPACE_BYTES, 4, 1.0, 1.0
    assert L.ftcf_verify_sample(C.byref(a), None) == NO_DEVICE
    assert L.ftcf_verify_sample(None, None) == NO_DEVICE


class _BothSwitches(_StubOp):
    def __init__(self):
        super().__init__()
        self.sampling = []

    def set_speculative_sampling(self, enabled=1):
        self.sampling.append(enabled)


def test_the_harness_switches_both_switches_on_for_speculative_arguments():
    ids, lens = _Tensor(torch.zeros((1, 4), dtype=torch.int32)), _Tensor(torch.tensor([4], dtype=torch.int32))
    op = _BothSwitches()
    g = _harness_model(op)
    g.forward(ids, lens, 2, return_output_length=True, return_cum_log_probs=1)
    assert op.scopes == [] and op.sampling == [] and op.calls[0][1] == {}
    g.forward(ids, lens, 2, top_k=torch.tensor([50], dtype=torch.int32), speculative_tokens=4)
    assert op.scopes == [1] and op.sampling == [1]
    assert op.calls[1][1] == {"speculative_tokens": 4, "speculative_ngram": None} and len(op.calls[1][0]) == 15
    g.forward(ids, lens, 2, speculative_ngram=2)
    assert op.scopes == [1, 1] and op.sampling == [1, 1]
    # an op with the scope alone (an older library) keeps working
    old = _StubOp()
    g = _harness_model(old)
    g.forward(ids, lens, 2, speculative_tokens=4)
    assert old.scopes == [1] and old.calls[0][1] == {"speculative_tokens": 4, "speculative_ngram": None}


def test_the_op_has_the_switch():
    from fastertransformer4codefuse_amd.gptneox_op import GptNeoXOp
    assert callable(GptNeoXOp.set_speculative_sampling) and callable(GptNeoXOp.set_speculative_scope)


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_the_sampled_tail_kernels_compile_without_spill_or_scratch(tmp_path):
    usage = _resource_usage("kernels_verify.hip", [], tmp_path)
    new = {k: v for k, v in usage.items() if any(n in k for n in ("k_verify_topk_slices", "k_verify_pick", "k_verify_sample_close"))}
    assert len(new) == 3, sorted(new)
    for name, r in new.items():
        assert r.get("VGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
    # the greedy tail's two kernels gained no instantiation and their names are in none of the new ones
    assert len([k for k in usage if "k_verify_slices" in k or "k_verify_close" in k]) == 2


_MODELS = {}


def _model(int8_mode):
    if int8_mode not in _MODELS:
        from oracle import oracle as orc
        from tests.helpers import load_tiny, quantize_layers, weight_list_to_layers
        cfg, w, z = load_tiny()
        layers, glob = weight_list_to_layers(cfg, w)
        lay = quantize_layers(layers) if int8_mode else layers
        _MODELS[int8_mode] = (cfg, z, orc.Model(dict(cfg, fp16=1, int8_mode=int8_mode), lay, glob))
    return _MODELS[int8_mode]


def test_the_table_covers_every_configuration_in_both_modes_on_both_prompts():
    configs = {(2, 1.0, 0.0), (4, 1.0, 0.0), (50, 1.0, 0.0), (50, 0.3, 0.0), (50, 1.0, 0.7), (64, 0.5, 0.0)}
    for mode in (0, 1):
        for prompt in ("golden", "repeating"):
            assert {c[2:5] for c in sc.CASES if c[:2] == (prompt, mode)} == configs, (prompt, mode)
    assert ("golden", 0, 2, 1.0, 0.0, 2) in sc.CASES and ("golden", 0, 4, 1.0, 0.0, 2) in sc.CASES
    assert ("golden", 0, 50, 1.0, 0.0, 2) in sc.CASES and ("repeating", 0, 50, 1.0, 0.0, 12) in sc.CASES


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_every_step_of_every_listed_request_is_stable_on_the_oracle(case):
    """... and the request departs from greedy (a pick that is not the arg max) and, on the repeating prompt, the n-gram lookup's
    drafts are accepted: what the engine test then checks is speculation under real sampling."""
    from tests.test_gpu_speculative import simulate
    pname, mode = case[:2]
    cfg, z, model = _model(mode)
    prompt = sc.prompt_of(pname, cfg, z)
    gen, stable, places = sc.replay(model, prompt, case)
    assert len(gen) == sc.OUT_LEN and all(stable), (case, stable)
    assert sum(1 for p in places if p > 0) >= 1, (case, places)
    if pname == "repeating":
        assert simulate(prompt, gen, 4, 3, sc.OUT_LEN)[2] >= 1, case
