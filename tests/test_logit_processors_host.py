"""CPU (-m "not gpu"): the logit-processor surface -- ftcf_logit_options / ftcf_logit_process_args in ctypes as the header
compiles them, the three new entry points declared, exported and bound, ftcf_logit_process without a device, the new
translation unit without scratch or spills, the numpy reference of the stage on hand-computed cases (one per operation and the
guard), and what ContinuousBatcher.submit can refuse before it reaches the library."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

from fastertransformer4codefuse_amd import capi
from tests import logit_processors_reference as lref
from tests.test_capi_abi import CC, check_mirror
from tests.test_kernel_resources import HIPCC, ROOT, _resource_usage

INF = float("inf")


@pytest.mark.skipif(CC is None, reason="no C compiler")
def test_struct_layouts_match_the_header():
    structs = {"ftcf_logit_options": capi.LogitOptions, "ftcf_logit_process_args": capi.LogitProcessArgs}
    for struct, cls in structs.items():
        check_mirror(struct)  # (every field's offset and size and the struct's size: tests/test_capi_abi.py)
        offs = [getattr(cls, n).offset for n, _ in cls._fields_]
        assert offs == sorted(offs) and len(set(offs)) == len(offs), "every field of the header, in its order"
    assert capi.LogitOptions._fields_[0][0] == "struct_size" and capi.LogitProcessArgs._fields_[0][0] == "struct_size"
    assert [n for n, _ in capi.LogitOptions._fields_] == ["struct_size", "presence_penalty", "frequency_penalty", "min_new_tokens",
                                                          "bias_ids", "bias_values", "n_bias", "bad_words", "bad_words_len"]


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ftcf.h")).read()
    assert "int ftcf_logit_process(const ftcf_logit_process_args* args, void* stream);" in hdr
    assert "const ftcf_logit_options* opts, long* request_id);" in hdr
    assert "int ftcf_batcher_set_token_mask(ftcf_batcher_t b, long request_id, const unsigned* allowed_bits, int n_words);" in hdr
    for name in ("ftcf_logit_process", "ftcf_batcher_submit_opts", "ftcf_batcher_set_token_mask"):
        assert name in capi.EXPORTED and hasattr(capi.lib(), name), name
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher
    params = inspect.signature(ContinuousBatcher.submit).parameters
    for name, default in (("logit_bias", None), ("bad_words", None), ("presence_penalty", 0.0), ("frequency_penalty", 0.0),
                          ("min_new_tokens", 0)):
        assert params[name].default == default and params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert list(params)[:9] == ["self", "prompt_ids", "max_new_tokens", "top_k", "top_p", "temperature", "seed", "repetition_penalty",
                                "stop_words"], "positional use is unchanged"
    assert list(inspect.signature(ContinuousBatcher.set_token_mask).parameters) == ["self", "request_id", "allowed"]
    assert capi.lib().ftcf_version() == 100


@pytest.mark.skipif(capi.device_count() > 0, reason="a GPU is visible")
def test_logit_process_needs_a_device():
    a = capi.LogitProcessArgs()
    a.struct_size = C.sizeof(a)
    assert capi.lib().ftcf_logit_process(C.byref(a), None) == -5


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_logit_kernels_compile_without_scratch_or_spills(tmp_path):
    kernels = _resource_usage("kernels_logits.hip", [], tmp_path)
    for name in ("k_logit_process", "k_logit_guard"):
        found = [k for k in kernels if name in k]
        assert found, (name, sorted(kernels))
        for k in found:
            r = kernels[k]
            assert r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (k, r)
    mk = open(os.path.join(ROOT, "fastertransformer4codefuse_amd", "csrc", "Makefile")).read()
    assert "kernels_logits.hip" in mk.split("SRCS")[1].splitlines()[0]


# ---- the numpy reference, by hand ------------------------------------------------------------------------------------------------
LOGITS = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0], dtype=np.float32)
END = 2


def test_reference_penalties_count_generated_tokens_only():
    # history: prompt [5, 5, 1], generated [1, 3, 3, 3]: c[1] = 1, c[3] = 3; token 5 is prompt only
    out, touched = lref.process_row(LOGITS, [5, 5, 1, 1, 3, 3, 3], 3, END, presence=0.5, frequency=0.25)
    want = LOGITS.astype(np.float64)
    want[1] -= 0.5 + 0.25 * 1
    want[3] -= 0.5 + 0.25 * 3
    assert out.tolist() == want.tolist() and touched.tolist() == [False, True, False, True, False, False, False, False]
    out, touched = lref.process_row(LOGITS, [5, 5, 1], 3, END, presence=0.5, frequency=0.25)  # gen_start == hist_len
    assert out.tolist() == LOGITS.tolist() and not touched.any()


def test_reference_bias_and_minus_infinity():
    out, touched = lref.process_row(LOGITS, [], 0, END, bias=[(0, 1.5), (7, -INF), (4, -2.0)])
    assert out.tolist() == [2.5, 2.0, 3.0, 4.0, 3.0, 6.0, 7.0, -INF]
    assert touched.tolist() == [True, False, False, False, True, False, False, False], "a banned logit is exact, not rounded"


def test_reference_min_new_tokens_holds_the_end_token_back():
    assert lref.process_row(LOGITS, [4, 4], 1, END, min_new=2)[0][END] == -INF  # one generated token < 2
    out, _ = lref.process_row(LOGITS, [4, 4, 4], 1, END, min_new=2)  # two: a row with the option set and nothing to do
    assert out.tolist() == LOGITS.tolist()


def test_reference_bad_words():
    hist = [6, 1, 4]
    words = [[0], [1, 4, 7], [9, 4, 5], [6, 1, 4, 3], [5, 6, 1, 4, 1]]  # single (id 0), a match, no match, the whole history, too long
    out, touched = lref.process_row(LOGITS, hist, 2, END, bad_words=words)
    assert out.tolist() == [-INF, 2.0, 3.0, -INF, 5.0, 6.0, 7.0, -INF] and not touched.any()
    assert lref.words_of(lref.word_list(words, 32)) == words
    wl = lref.word_list([[1, 2], [3]], 8)
    assert wl.tolist() == [[1, 2, 3, 0, 0, 0, 0, 0], [2, 3, -1, -1, -1, -1, -1, -1]]


def test_reference_mask_and_order_of_operations():
    mask = np.zeros(8, dtype=bool)
    mask[[1, 3, 6]] = True
    # bias on a masked token stays masked; penalty then bias on an allowed one add up; min_new bans end_id before the mask does
    out, touched = lref.process_row(LOGITS, [3, 3], 0, END, presence=1.0, frequency=0.5, bias=[(3, 10.0), (0, 100.0)], min_new=5, mask=mask)
    assert out.tolist() == [-INF, 2.0, -INF, 4.0 - (1.0 + 0.5 * 2) + 10.0, -INF, -INF, 7.0, -INF]
    assert touched.tolist() == [False, False, False, True, False, False, False, False]
    assert lref.pack_mask(mask).tolist() == [0b01001010]
    assert lref.pack_mask(np.ones(33, dtype=bool)).tolist() == [0xFFFFFFFF, 1]


def test_reference_guard_and_untouched_rows():
    mask = np.zeros(8, dtype=bool)
    mask[5] = True
    out, touched = lref.process_row(LOGITS, [], 0, END, bad_words=[[5]], mask=mask)
    assert out.tolist() == [-INF, -INF, 0.0, -INF, -INF, -INF, -INF, -INF] and not touched.any()
    # a finished row and a row without options keep their values, an all -inf one included
    dead = np.full(8, -INF, dtype=np.float32)
    assert lref.process_row(dead, [1], 0, END)[0].tolist() == dead.tolist()
    assert lref.process_row(LOGITS, [1], 0, END, bias=[(1, 1.0)], finished=True)[0].tolist() == LOGITS.tolist()
    assert lref.tolerance(8.0, presence=1.0, frequency_times_count=2.0, bias=16.0) == 4 * 2.0 ** -24 * 16.0


# ---- what submit() refuses before the library sees it ------------------------------------------------------------------------------
def test_submit_validates_the_new_keywords_without_a_gpu():
    from fastertransformer4codefuse_amd.batcher import ContinuousBatcher, pack_logit_options
    assert pack_logit_options() == (None, ())
    assert pack_logit_options(logit_bias={}, bad_words=[], presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0) == (None, ())
    o, keep = pack_logit_options(logit_bias={7: -INF, 3: 1.5}, bad_words=[[4], [5, 6]], presence_penalty=0.5, frequency_penalty=0.25,
                                 min_new_tokens=3)
    assert o.struct_size == C.sizeof(capi.LogitOptions) and (o.presence_penalty, o.frequency_penalty, o.min_new_tokens) == (0.5, 0.25, 3)
    assert o.n_bias == 2 and [o.bias_ids[i] for i in range(2)] == [7, 3] and o.bias_values[0] == -INF and o.bias_values[1] == 1.5
    assert o.bad_words_len == 3 and [o.bad_words[i] for i in range(6)] == [4, 5, 6, 1, 3, -1] and len(keep) == 3
    assert pack_logit_options(logit_bias=[(1, 2.0)])[0].n_bias == 1, "pairs as well as a dict"
    cb = ContinuousBatcher.__new__(ContinuousBatcher)  # (no engine: every case below is refused before the library is called)
    cb._h = None
    bad = [dict(logit_bias=[(1, 1.0), (1, 2.0)]), dict(logit_bias={-1: 1.0}), dict(logit_bias={1: math.nan}), dict(logit_bias={1: INF}),
           dict(logit_bias={i: 1.0 for i in range(1025)}), dict(min_new_tokens=-1), dict(bad_words=[list(range(257))]),
           dict(bad_words=[[]]), dict(bad_words=[[-3]]), dict(presence_penalty=math.nan), dict(frequency_penalty=INF)]
    for kw in bad:
        with pytest.raises(ValueError):
            cb.submit([1, 2, 3], 4, **kw)
