"""-m gpu: top_logprobs of ONE dynamic-decode step (include/ftcf.h ftcf_dynamic_decode_step: top_logprobs / top_ids /
top_log_probs; kernels_sampling.hip k_top_logprobs_slices + k_top_logprobs_merge) on the crafted logits of
tests/decode_cases.py, against the float64 statement tests/top_logprobs_reference.py.

Every sampling case at N = 5; the V = 5 / 7 cases (N > V) and one case per V in {1000, 2051, 4099, 100864} (two at 100864)
at N = 1 and N = 20.  Ids are exact but for the excused swaps of top-p rows (test_top_logprobs_reference.py), values compare by
rank within LP_TOL, -inf and the (-1, ...) patterns are exact.  The step takes the general form; tokens, cum_log_probs,
output_log_probs, draw counters, lengths and flags are byte for byte those of the same call without the fields; only row
step - max_input_len of the time-major buffers is written (row 0 with row_len), rows that were finished keep what the buffers
held; the guard bands of the buffers and of the logits are untouched; two runs are bit-identical.

The two length_criterion cases run at step == total_len, where the time-major buffers have no row: the call is refused, as
it is with output_log_probs.  ONE_HOT's top-p rows are left out (test_top_logprobs_reference.py, (c))."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import decode_cases as dc
from tests import decode_reference as ref
from tests import top_logprobs_reference as tlp
from tests.decode_cases import LP_TOL
from tests.test_gpu_decode_step import GUARD_F, GUARD_I, Guarded, dev, host_arg, stream

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

capi = None
CASES = {c.name: c for c in dc.sampling_cases()}
FILL_I, FILL_F = -5, 77.0  # what the buffers hold before the step


@pytest.fixture(scope="module", autouse=True)
def _lib():
    global capi
    from fastertransformer4codefuse_amd import capi as _c
    capi = _c
    capi.require_gpu()
    yield


def _runs():
    runs = [(n, 5) for n in CASES]
    small = [n for n, c in CASES.items() if c.V in (5, 7)]
    sized = ["qgauss_V1000_k50", "qgauss_V2051_p0.9", "batch_16_mixed", "flat_V100864_p1.0", "all_equal_V100864_k50"]
    assert [CASES[n].V for n in sized] == [1000, 2051, 4099, 100864, 100864]
    return runs + [(n, N) for N in (1, 20) for n in small + sized]


RUNS = _runs()


def gpu_step(case, seed, monkeypatch, N, fused="1", null_buffer=False):
    """ftcf_dynamic_decode_step with return_cum_log_probs and output_log_probs on; N > 0 adds the top_logprobs fields.  The
    fused forms are enabled for the run with the fields (they must not be taken) and disabled for the one without."""
    monkeypatch.setenv("FTCF_TOPK_FUSED", fused)
    monkeypatch.setenv("FTCF_GREEDY_FUSED", fused)
    B = case.B
    rows = max(1, case.total_len - case.max_input_len)
    has_row = case.row_len is not None or case.step < case.total_len
    logits, ids = Guarded(case.logits, np.float32(GUARD_F)), Guarded(case.output_ids, np.int32(GUARD_I))
    fin, slen = dev(case.finished, np.uint8), dev(case.seq_len, np.int32)
    cum, draws = dev(case.cum_log_probs, np.float32), dev(case.draw_counter, np.uint64)
    pads, in_len = dev(np.full(B, 100, np.int32), np.int32), dev(case.input_lengths, np.int32)
    olp = Guarded(np.full((rows, B), FILL_F, np.float32), np.float32(GUARD_F)) if has_row else None
    t_ids = Guarded(np.full((rows, B, max(N, 1)), FILL_I, np.int32), np.int32(GUARD_I))
    t_lps = Guarded(np.full((rows, B, max(N, 1)), FILL_F, np.float32), np.float32(GUARD_F))
    sw, opt, row_len = dev(case.stop_words, np.int32), dev(case.optional_last_tokens, np.int32), dev(case.row_len, np.int32)
    keep = [host_arg(case.top_k, np.int32), host_arg(case.top_p, np.float32), host_arg(case.temperature, np.float32),
            host_arg(case.repetition_penalty, np.float32), host_arg(case.min_length, np.int32), host_arg(case.seeds(seed), np.uint64)]
    all_finished, next_step, ran = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    a = capi.DynamicDecodeArgs()
    a.logits, a.output_ids = logits.ptr, ids.ptr
    a.finished, a.seq_len, a.cum_log_probs = fin.data_ptr(), slen.data_ptr(), cum.data_ptr()
    a.output_log_probs = olp.ptr if olp else None
    a.draw_counter, a.pad_count, a.input_lengths = draws.data_ptr(), pads.data_ptr(), in_len.data_ptr()
    a.stop_words = sw.data_ptr() if sw is not None else None
    a.optional_last_tokens = opt.data_ptr() if opt is not None else None
    a.row_len = row_len.data_ptr() if row_len is not None else None
    for name, (_, ptr, n) in zip(("top_k", "top_p", "temperature", "repetition_penalty", "min_length", "random_seed"), keep):
        setattr(a, name, ptr)
        setattr(a, "n_" + name, n)
    a.all_finished, a.next_step, a.form = C.pointer(all_finished), C.pointer(next_step), C.pointer(ran)
    a.stop_len = 0 if case.stop_words is None else case.stop_words.shape[2]
    a.optional_count = 0 if case.optional_last_tokens is None else case.optional_last_tokens.shape[1]
    a.B, a.V, a.step, a.max_input_len = B, case.V, case.step, case.max_input_len
    a.total_len, a.end_id = case.total_len, case.end_id
    a.return_cum_log_probs, a.finish = 1, int(case.finish)
    if N > 0:
        a.top_logprobs, a.top_ids, a.top_log_probs = N, t_ids.ptr, None if null_buffer else t_lps.ptr
    rc = capi.lib().ftcf_dynamic_decode_step(C.byref(a), stream())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None
    logits.read()
    return rc, dict(output_ids=ids.read(), finished=fin.cpu().numpy(), seq_len=slen.cpu().numpy(), cum_log_probs=cum.cpu().numpy(),
                    draw_counter=draws.cpu().numpy(), pad_count=pads.cpu().numpy(), output_log_probs=olp.read() if olp else None,
                    top_ids=t_ids.read(), top_log_probs=t_lps.read(), all_finished=all_finished.value, next_step=next_step.value,
                    form=ran.value)


_BASE, _REF = {}, {}


def baseline(case, monkeypatch):
    """the same call without the fields in the general form, once per case"""
    if case.name not in _BASE:
        rc, got = gpu_step(case, dc.SEEDS[case.name], monkeypatch, 0, fused="0")
        assert rc == 0 and got["form"] == dc.GENERAL
        _BASE[case.name] = got
    return _BASE[case.name]


def reference(case, N):
    if (case.name, N) not in _REF:
        _REF[case.name, N] = tlp.case_top_n(case, N, atol=LP_TOL["atol"])
    return _REF[case.name, N]


@pytest.mark.parametrize("name,N", RUNS, ids=[f"{n}-N{N}" for n, N in RUNS])
def test_top_logprobs_step(name, N, monkeypatch):
    case = CASES[name]
    seed = dc.SEEDS[name]
    rc, got = gpu_step(case, seed, monkeypatch, N)
    if case.row_len is None and case.step >= case.total_len:
        assert rc == -1 and b"top_logprobs has no row" in capi.lib().ftcf_last_error()
        return
    assert rc == 0, capi.lib().ftcf_last_error()
    assert got["form"] == dc.GENERAL, "a step with top_logprobs must take the general form"
    base = baseline(case, monkeypatch)
    for key in ("output_ids", "finished", "seq_len", "cum_log_probs", "output_log_probs", "draw_counter", "pad_count"):
        assert got[key].tobytes() == base[key].tobytes(), f"{key} differs from the call without top_logprobs"
    assert (got["all_finished"], got["next_step"]) == (base["all_finished"], base["next_step"])
    rc2, again = gpu_step(case, seed, monkeypatch, N)
    assert rc2 == 0 and again["top_ids"].tobytes() == got["top_ids"].tobytes()
    assert again["top_log_probs"].tobytes() == got["top_log_probs"].tobytes(), "two runs differ"

    t = 0 if case.row_len is not None else case.step - case.max_input_len
    ids, lps = got["top_ids"], got["top_log_probs"]
    assert (np.delete(ids, t, axis=0) == FILL_I).all() and (np.delete(lps, t, axis=0) == FILL_F).all(), "another row was written"
    want = reference(case, N)
    k_eff, _, _ = ref.route(case.top_k, case.top_p, case.B)
    steps = [int(r) + 1 for r in case.row_len] if case.row_len is not None else [case.step] * case.B
    for b in range(case.B):
        gi, gl = ids[t, b], lps[t, b]
        w = want[b]
        if w is None:  # finished before the step: not written
            assert (gi == FILL_I).all() and (gl == FILL_F).all(), f"row {b} was finished and was written"
            continue
        if w["topp"] and not w["well_posed"]:
            assert name in ("one_hot_p0.9",)
            continue
        print(name, N, "row", b, "ids", gi.tolist(), "expected", w["ids"].tolist(), "lp", gl.tolist())
        for j in range(N):
            if gi[j] != w["ids"][j]:
                assert w["excused"][j] and int(gi[j]) in w["clusters"][j], (b, j, int(gi[j]), int(w["ids"][j]))
        live = gi[gi >= 0]
        assert len(set(live.tolist())) == live.size
        inf = np.isneginf(w["log_probs"])
        assert (np.isneginf(gl) == inf).all(), (b, gl, w["log_probs"])
        np.testing.assert_allclose(gl[~inf], w["log_probs"][~inf], err_msg=f"row {b}", **LP_TOL)
        # the emitted token
        tok = int(got["output_ids"][steps[b], b])
        if k_eff[b] == 1:
            assert gi[0] == tok, (b, "a greedy row's first pair is its token")
        if 1 <= k_eff[b] <= N:
            assert tok in gi.tolist(), (b, "the token of a top_k <= N row is among the pairs")
        if tok in gi.tolist():
            j = gi.tolist().index(tok)
            np.testing.assert_allclose(gl[j], got["output_log_probs"][t, b], **LP_TOL)


def test_refusals(monkeypatch):
    case = CASES["qgauss_V100_k2"]
    rc, _ = gpu_step(case, dc.SEEDS[case.name], monkeypatch, 21)
    assert rc == -1 and b"top_logprobs" in capi.lib().ftcf_last_error()
    rc, _ = gpu_step(case, dc.SEEDS[case.name], monkeypatch, 5, null_buffer=True)
    assert rc == -1 and b"top_logprobs needs" in capi.lib().ftcf_last_error()
