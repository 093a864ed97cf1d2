"""-m gpu: ONE dynamic-decode step of kernels_sampling.hip and ONE beam-search step of kernels_beam.hip on crafted logits (include/ftcf.h
ftcf_dynamic_decode_step, ftcf_beam_search_step), against the CPU oracle and the float64 statement of the layer
(tests/decode_reference.py), through every form a case is eligible for: the general four launches, k_topk_decode,
k_greedy_decode.  The cases (tests/decode_cases.py) are the tie, mask and size edges a random model's logits never reach;
test_decode_step_reference.py shows on the CPU that each of them is well-posed.

Tokens, finished, sequence lengths, draw counters, all_finished and the next step are exact; log-probabilities use the
tolerance of test_gpu_sampling_vocab.py.  Every cell of output_ids but the written ones keeps its sentinel, and a guard band
on both sides of the logits and of the id buffer is unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import decode_cases as dc
from tests.decode_cases import LP_TOL, SCORE_TOL, oracle_beam_step, oracle_step

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

capi = None
CASES, BEAM_CASES = dc.sampling_cases(), dc.beam_cases()
GUARD = 256            # elements on both sides of a guarded buffer
GUARD_F, GUARD_I = 12345.5, -99
ENV = {dc.GENERAL: ("0", "0"), dc.TOPK_FUSED: ("1", "0"), dc.GREEDY_FUSED: ("0", "1")}  # FTCF_TOPK_FUSED, FTCF_GREEDY_FUSED


@pytest.fixture(scope="module", autouse=True)
def _lib():
    global capi
    from fastertransformer4codefuse_amd import capi as _c
    capi = _c
    capi.require_gpu()
    yield


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """a device copy of `a` with GUARD elements of a fill value on both sides"""

    def __init__(self, a, fill):
        a = np.ascontiguousarray(a)
        self.shape, self.fill = a.shape, fill
        host = np.full(a.size + 2 * GUARD, fill, a.dtype)
        host[GUARD:GUARD + a.size] = a.reshape(-1)
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + GUARD * a.dtype.itemsize

    def read(self):
        """the payload; the guard bands must be as they were"""
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == self.fill).all() and (host[-GUARD:] == self.fill).all(), "a guard band was written"
        return host[GUARD:-GUARD].reshape(self.shape)


def dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def host_arg(v, dtype):
    """a runtime argument as (pointer, count): 1 entry broadcasts, None is "not given" """
    if v is None:
        return None, C.c_void_p(None), 0
    a = np.ascontiguousarray(np.asarray(v, dtype=dtype).reshape(-1))
    return a, C.c_void_p(a.ctypes.data), a.size


def gpu_step(case, seed, monkeypatch, form=dc.GENERAL, total_len=None):
    """ftcf_dynamic_decode_step on device copies of the case's state -> (status, dict)"""
    monkeypatch.setenv("FTCF_TOPK_FUSED", ENV[form][0])
    monkeypatch.setenv("FTCF_GREEDY_FUSED", ENV[form][1])
    B = case.B
    want_lp = case.return_cum_log_probs or case.output_log_probs
    logits, ids = Guarded(case.logits, np.float32(GUARD_F)), Guarded(case.output_ids, np.int32(GUARD_I))
    fin, slen = dev(case.finished, np.uint8), dev(case.seq_len, np.int32)
    cum, draws = dev(case.cum_log_probs, np.float32), dev(case.draw_counter, np.uint64)
    pads, in_len = dev(np.full(B, 100, np.int32), np.int32), dev(case.input_lengths, np.int32)
    olp_rows = max(1, case.total_len - case.max_input_len)
    olp = Guarded(np.full((olp_rows, B), 77.0, np.float32), np.float32(GUARD_F)) if case.output_log_probs else None
    sw, opt, row_len = dev(case.stop_words, np.int32), dev(case.optional_last_tokens, np.int32), dev(case.row_len, np.int32)
    keep = [host_arg(case.top_k, np.int32), host_arg(case.top_p, np.float32), host_arg(case.temperature, np.float32),
            host_arg(case.repetition_penalty, np.float32), host_arg(case.min_length, np.int32), host_arg(case.seeds(seed), np.uint64)]
    all_finished, next_step, ran = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    a = capi.DynamicDecodeArgs()
    a.logits, a.output_ids = logits.ptr, ids.ptr
    a.finished, a.seq_len, a.cum_log_probs = fin.data_ptr(), slen.data_ptr(), cum.data_ptr() if want_lp else None
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
    a.total_len, a.end_id = case.total_len if total_len is None else total_len, case.end_id
    a.return_cum_log_probs, a.finish = int(case.return_cum_log_probs), int(case.finish)
    rc = capi.lib().ftcf_dynamic_decode_step(C.byref(a), stream())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None
    logits.read()  # (the row is modified in place, differently by every form: only the guard bands are held)
    return rc, dict(output_ids=ids.read(), finished=fin.cpu().numpy(), seq_len=slen.cpu().numpy(), cum_log_probs=cum.cpu().numpy(),
                    draw_counter=draws.cpu().numpy(), pad_count=pads.cpu().numpy(), output_log_probs=olp.read() if olp else None,
                    all_finished=all_finished.value, next_step=next_step.value, form=ran.value)


_ORACLE = {}


def expected(case):
    """the float64 statement and the oracle's step of a case, computed once and shared by the forms"""
    if case.name not in _ORACLE:
        seed = dc.SEEDS[case.name]
        _ORACLE[case.name] = (case.reference(seed), oracle_step(case, seed))
    return _ORACLE[case.name]


RUNS = [(c, f) for c in CASES for f in c.forms()]


def test_every_form_meets_a_tie_case_and_a_minus_inf_case():
    for form in ENV:
        names = [c.name for c, f in RUNS if f == form]
        assert any(n.startswith(("all_equal", "plateau", "signed_zero")) for n in names), dc.FORM_NAMES[form]
        assert any(n.startswith("minus_inf") for n in names), dc.FORM_NAMES[form]


@pytest.mark.parametrize("case,form", RUNS, ids=[f"{c.name}-{dc.FORM_NAMES[f]}" for c, f in RUNS])
def test_decode_step(case, form, monkeypatch):
    want, orc_out = expected(case)
    rc, got = gpu_step(case, dc.SEEDS[case.name], monkeypatch, form)
    assert rc == 0, capi.lib().ftcf_last_error()
    assert got["form"] == form, "the launcher took another form than the eligibility rule says"
    rows = [int(r) + 1 for r in case.row_len] if case.row_len is not None else [case.step] * case.B
    print(case.name, dc.FORM_NAMES[form], "tokens", [int(got["output_ids"][rows[b], b]) for b in range(case.B)], "expected",
          want["tokens"].tolist())
    for name, exp in (("float64", want), ("oracle", orc_out)):
        np.testing.assert_array_equal(got["output_ids"], exp["output_ids"], err_msg=f"output_ids vs {name}")
        np.testing.assert_array_equal(got["finished"], exp["finished"], err_msg=f"finished vs {name}")
        np.testing.assert_array_equal(got["seq_len"], exp["seq_len"], err_msg=f"seq_len vs {name}")
        np.testing.assert_array_equal(got["draw_counter"], exp["draw_counter"], err_msg=f"draw_counter vs {name}")
        if case.return_cum_log_probs or case.output_log_probs:
            np.testing.assert_allclose(got["cum_log_probs"], exp["cum_log_probs"], err_msg=f"cum_log_probs vs {name}", **LP_TOL)
        else:
            np.testing.assert_array_equal(got["cum_log_probs"], case.cum_log_probs)
    # (output_ids above is the whole buffer: every cell but the written ones still holds its sentinel or its history token)
    if case.output_log_probs:
        olp = got["output_log_probs"]
        row = 0 if case.row_len is not None else case.step - case.max_input_len
        live = case.finished == 0
        np.testing.assert_allclose(olp[row][live], want["step_log_probs"][live], **LP_TOL)
        assert (olp[row][~live] == 77.0).all() and (np.delete(olp, row, axis=0) == 77.0).all(), "output_log_probs written elsewhere"
    if case.finish:
        assert got["all_finished"] == want["all_finished"] and got["next_step"] == want["next_step"]
        np.testing.assert_array_equal(got["pad_count"], 100 + want["pad_count"])
    else:  # the batcher's step leaves the state alone
        assert got["all_finished"] == 0 and got["next_step"] == case.step
        np.testing.assert_array_equal(got["pad_count"], 100)


def _one_row(V, **kw):
    l = dc.smooth("refusal", 1, 1000)[0]
    return dc.Case("refusal", np.resize(l, (1, V)), end_id=1, **kw)


def test_vocabulary_limit_of_the_general_path(monkeypatch):
    """a stage-1 slice holds 256 x 60 logits in registers: V = 8 * 15360 is taken, one more is refused"""
    ok = _one_row(122880, top_k=1)
    rc, got = gpu_step(ok, 5, monkeypatch, dc.GENERAL)
    assert rc == 0 and got["form"] == dc.GENERAL
    want = ok.reference(5)
    np.testing.assert_array_equal(got["output_ids"], want["output_ids"])
    rc, _ = gpu_step(_one_row(122881, top_k=1), 5, monkeypatch, dc.GENERAL)
    assert rc == -1 and b"vocabulary too large" in capi.lib().ftcf_last_error()


def test_history_limit_of_the_repetition_penalty(monkeypatch):
    """the penalty stages total_len {value, id} pairs in 60 KiB of LDS: 7680 is taken (a case of the table), 7681 is refused"""
    case = next(c for c in CASES if c.name == "repetition_total_len_7680")
    rc, _ = gpu_step(case, dc.SEEDS[case.name], monkeypatch, dc.GENERAL, total_len=7681)
    assert rc == -1 and b"sequence too long" in capi.lib().ftcf_last_error()


def test_top_k_must_not_be_negative(monkeypatch):
    case = dc.Case("negative_k", dc.smooth("refusal", 1, 100), top_k=-1, top_p=0.5)
    rc, _ = gpu_step(case, 5, monkeypatch, dc.GENERAL)
    assert rc == -1 and b"top_k" in capi.lib().ftcf_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# beam search
# ---------------------------------------------------------------------------------------------------------------------
def gpu_beam_step(case):
    BK = case.B * case.K
    logits = Guarded(case.logits, np.float32(GUARD_F))
    ids, par = Guarded(case.output_ids, np.int32(GUARD_I)), Guarded(case.parent_ids, np.int32(GUARD_I))
    indir = Guarded(case.cache_indir, np.int32(GUARD_I))
    fin, slen, cum = dev(case.finished, np.uint8), dev(case.seq_len, np.int32), dev(case.cum_log_probs, np.float32)
    in_len, sw, opt = dev(case.input_lengths, np.int32), dev(case.stop_words, np.int32), dev(case.optional_last_tokens, np.int32)
    keep = [host_arg(case.temperature, np.float32), host_arg(case.repetition_penalty, np.float32), host_arg(case.diversity_rate, np.float32),
            host_arg(case.len_penalty, np.float32), host_arg(case.min_length, np.int32)]
    a = capi.BeamSearchArgs()
    a.logits, a.output_ids, a.parent_ids, a.cache_indir = logits.ptr, ids.ptr, par.ptr, indir.ptr
    a.finished, a.seq_len, a.cum_log_probs, a.input_lengths = fin.data_ptr(), slen.data_ptr(), cum.data_ptr(), in_len.data_ptr()
    a.stop_words = sw.data_ptr() if sw is not None else None
    a.optional_last_tokens = opt.data_ptr() if opt is not None else None
    for name, (_, ptr, n) in zip(("temperature", "repetition_penalty", "beam_search_diversity_rate", "len_penalty", "min_length"), keep):
        setattr(a, name, ptr)
        setattr(a, "n_" + name, n)
    a.stop_len = 0 if case.stop_words is None else case.stop_words.shape[2]
    a.optional_count = 0 if case.optional_last_tokens is None else case.optional_last_tokens.shape[1]
    a.B, a.K, a.V, a.step, a.max_input_len = case.B, case.K, case.V, case.step, case.max_input_len
    a.total_len, a.s_max, a.end_id = case.total_len, case.s_max, case.end_id
    capi.check(capi.lib().ftcf_beam_search_step(C.byref(a), stream()))
    torch.cuda.synchronize()
    logits.read()
    planes = indir.read()
    np.testing.assert_array_equal(planes[case.src_plane], case.cache_indir[case.src_plane], err_msg="the plane the step reads was written")
    return dict(output_ids=ids.read(), parent_ids=par.read(), finished=fin.cpu().numpy(), seq_len=slen.cpu().numpy(),
                cum_log_probs=cum.cpu().numpy(), tgt_indir=planes[1 - case.src_plane].reshape(case.B, case.K, -1))


@pytest.mark.parametrize("case", BEAM_CASES, ids=lambda c: c.name)
def test_beam_search_step(case):
    want, orc_out = case.reference(), oracle_beam_step(case)
    got = gpu_beam_step(case)
    print(case.name, "tokens", got["output_ids"][case.step].tolist()[:8], "parents", got["parent_ids"][case.step].tolist()[:8])
    for name, exp in (("float64", want), ("oracle", orc_out)):
        for key in ("output_ids", "parent_ids", "finished", "seq_len", "tgt_indir"):
            np.testing.assert_array_equal(got[key], exp[key], err_msg=f"{key} vs {name}")
        np.testing.assert_allclose(got["cum_log_probs"], exp["cum_log_probs"], err_msg=f"cum_log_probs vs {name}", **SCORE_TOL)
