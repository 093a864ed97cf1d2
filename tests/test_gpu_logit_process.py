"""-m gpu: ftcf_logit_process against the float64 reference of tests/logit_processors_reference.py.

Shapes V in {97, 4129, 100864} (no multiple of 32 nor of a slice) x B in {1, 3, 16}, the history time-major and row-major.  The
rows of a case come from one catalogue (ROW_KINDS): a 2000-token history with heavy repetition under every option at once,
histories of length 0 and 1, gen_start == hist_len, ids on the edges (0, V - 1, the first and last id of a slice, end_id), bad
words longer than the history / equal to it / across the prompt-generated boundary in a -1 padded list, a bias of -inf and one on a
masked token, rows whose options leave nothing (the guard), finished, disabled and option-free rows.  B = 16 runs all of them, B =
3 and B = 1 the first ones (the first row carries every option).

Tolerance: masked, banned, held-back and guarded logits and every logit no arithmetic reached are exact (-inf, 0 at end_id, or
the input BITS); a penalised or biased logit is within 4 * 2^-24 * max(|logit|, |penalty|, |bias|) of the float64 value.  Runs
over three slice sizes are bit-identical."""
import ctypes as C

import numpy as np
import pytest

from tests import logit_processors_reference as lref

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
INF = float("inf")
SLICE = 2048  # the default slice: its edges are the ids the catalogue puts options on
END_ID = {97: 2, 4129: 2048, 100864: 4095}
BAD_LEN = 64


def edges(V):
    e = {0, V - 1, END_ID[V], (V - 1) // SLICE * SLICE}
    if V > SLICE:
        e |= {SLICE - 1, SLICE}
    return sorted(e)


def row_kinds(V, rng):
    """the catalogue: dicts of process_row's keyword arguments (+ row_on)"""
    end, E = END_ID[V], edges(V)
    pool = np.array(E + rng.randint(0, V, size=12).tolist())
    long_hist = pool[rng.randint(0, len(pool), size=2000)].tolist()  # heavy repetition, the edge ids among the tokens
    others = [t for t in rng.permutation(V).tolist() if t not in E]
    allowed = rng.rand(V) < 0.5
    allowed[E] = True
    allowed[others[0]] = False  # ... and a bias on a masked token
    n_rand = min(300, len(others) - 1)
    bias_all = [(t, float(v)) for t, v in zip(E, rng.randn(len(E)) * 3)] + [(others[0], 50.0), (others[1], -INF)] + [
        (t, float(v)) for t, v in zip(others[2:n_rand], rng.randn(n_rand) * 3)]
    h = long_hist
    words_all = [[0], [h[-1], V - 1], [h[-2], h[-1], others[3]], [h[-1], h[-1], others[4]], [others[5], others[6]], [end, end, end]]
    short = [7 % V, 9 % V, 11 % V, 5 % V]  # prompt [7, 9], generated [11, 5]
    only = np.zeros(V, dtype=bool)
    only[others[7]] = True
    kinds = [
        dict(history=long_hist, gen_start=700, presence=0.7, frequency=0.3, bias=bias_all, min_new=0, bad_words=words_all, mask=allowed),
        dict(history=short, gen_start=2),  # no option: untouched
        dict(history=short, gen_start=2, presence=1.0, frequency=1.0, bias=[(0, 1.0)], mask=allowed, finished=True),
        dict(history=[], gen_start=0, presence=1.5, frequency=0.5, bias=[(V - 1, -2.0), (0, -INF)]),
        dict(history=[V - 1], gen_start=0, presence=1.5, frequency=-0.5),
        dict(history=short, gen_start=4, presence=2.0, frequency=2.0, min_new=1),  # nothing generated: end_id held back
        dict(history=short, gen_start=2, bad_words=[[1, 2, 3, 7 % V, 9 % V, 11 % V, 5 % V, E[1]],  # longer than the history
                                                    short + [V - 1],                                  # the whole history
                                                    [9 % V, 11 % V, 5 % V, 0],                        # across the boundary
                                                    [9 % V, 11 % V, 6 % V, E[-1]]]),                  # no match
        dict(history=short, gen_start=2, bad_words=[[others[7]]], mask=only),  # nothing left: the guard
        dict(history=short, gen_start=2, bias=[(others[7], -INF)], mask=only),  # the same through the bias
        dict(history=short, gen_start=2, mask=rng.rand(V) < 0.9),
        dict(history=long_hist, gen_start=0, min_new=100),  # satisfied: an option that has nothing to do
        dict(history=long_hist, gen_start=1999, presence=3.0),
        dict(history=long_hist, gen_start=3, frequency=-0.125),
        dict(history=short, gen_start=2, bias=[(t, 2.5) for t in E]),
        dict(history=long_hist, gen_start=0, presence=1.0, bias=[(end, 4.0)], bad_words=[[3 % V]], row_on=False),
        dict(history=short, gen_start=2, bad_words=[[0], [V - 1], [end]], min_new=3),
    ]
    return kinds


_CASES = {}


def case(V, B):
    """rows, logits fp32 [B, V], reference float64 [B, V], touched, tolerance -- built once per shape, shared by both layouts"""
    if (V, B) not in _CASES:
        rng = np.random.RandomState(V + B)
        rows = row_kinds(V, rng)[:B]
        logits = (rng.randn(B, V) * 5).astype(np.float32)
        logits[:, 5 % V] = -INF
        logits[:, 6 % V] = -0.0
        ref, touched, tol = np.zeros((B, V)), np.zeros((B, V), dtype=bool), np.zeros((B, V))
        for b, r in enumerate(rows):
            kw = {k: v for k, v in r.items() if k != "row_on"}
            if r.get("row_on", True):
                ref[b], touched[b] = lref.process_row(logits[b], end_id=END_ID[V], **kw)
            else:
                ref[b] = logits[b]
            tol[b] = lref.tolerance_row(logits[b], r["history"], r["gen_start"], r.get("presence", 0.0), r.get("frequency", 0.0),
                                        r.get("bias", ()))
        _CASES[(V, B)] = rows, logits, ref, touched, tol
    return _CASES[(V, B)]


def launch(rows, logits, V, layout, slice_=0, hist_len_add=0):
    import torch
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    B = len(rows)
    T = max(1, max(len(r["history"]) for r in rows))
    hist = np.full((B, T), -7, dtype=np.int32)
    for b, r in enumerate(rows):
        hist[b, :len(r["history"])] = r["history"]
    nb = max(1, max(len(r.get("bias", ())) for r in rows))
    bias_ids, bias_vals = np.zeros((B, nb), dtype=np.int32), np.zeros((B, nb), dtype=np.float32)
    bad = np.zeros((B, 2, BAD_LEN), dtype=np.int32)
    mask = np.zeros((B, (V + 31) // 32), dtype=np.uint32)
    for b, r in enumerate(rows):
        for i, (t, v) in enumerate(r.get("bias", ())):
            bias_ids[b, i], bias_vals[b, i] = t, v
        bad[b] = lref.word_list(r.get("bad_words", []), BAD_LEN)
        if r.get("mask") is not None:
            mask[b] = lref.pack_mask(r["mask"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    col = lambda key, dt, default=0: dev(np.array([r.get(key, default) for r in rows], dtype=dt))
    t = dict(logits=dev(logits.copy()), finished=col("finished", np.uint8), row_on=col("row_on", np.uint8, True),
             hist=dev(hist.T if layout == "time_major" else hist),
             hist_len=dev(np.array([len(r["history"]) - hist_len_add for r in rows], dtype=np.int32)), gen_start=col("gen_start", np.int32),
             presence=col("presence", np.float32), frequency=col("frequency", np.float32), min_new=col("min_new", np.int32),
             bias_ids=dev(bias_ids), bias_vals=dev(bias_vals), n_bias=dev(np.array([len(r.get("bias", ())) for r in rows], dtype=np.int32)),
             bad=dev(bad), mask=dev(mask.view(np.int32)), mask_on=dev(np.array([r.get("mask") is not None for r in rows], dtype=np.uint8)))
    a = capi.LogitProcessArgs()
    a.struct_size, a.batch_size, a.vocab_size, a.end_id = C.sizeof(a), B, V, END_ID[V]
    a.logits, a.finished, a.row_on, a.hist = t["logits"].data_ptr(), t["finished"].data_ptr(), t["row_on"].data_ptr(), t["hist"].data_ptr()
    a.stride_t, a.stride_b = (B, 1) if layout == "time_major" else (1, T)
    a.hist_len, a.gen_start, a.hist_len_add = t["hist_len"].data_ptr(), t["gen_start"].data_ptr(), hist_len_add
    a.presence_penalty, a.frequency_penalty, a.min_new_tokens = t["presence"].data_ptr(), t["frequency"].data_ptr(), t["min_new"].data_ptr()
    a.bias_ids, a.bias_values, a.n_bias, a.bias_stride = t["bias_ids"].data_ptr(), t["bias_vals"].data_ptr(), t["n_bias"].data_ptr(), nb
    a.bad_words, a.bad_words_len, a.mask, a.mask_on, a.slice = t["bad"].data_ptr(), BAD_LEN, t["mask"].data_ptr(), t["mask_on"].data_ptr(), slice_
    capi.check(capi.lib().ftcf_logit_process(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return t["logits"].cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("layout", ["time_major", "row_major"])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("V", [97, 4129, 100864])
def test_stage_matches_the_float64_reference(V, B, layout):
    rows, logits, ref, touched, tol = case(V, B)
    got = launch(rows, logits, V, layout, hist_len_add=1 if layout == "time_major" else 0)
    exact = ~touched
    wrong = exact & (bits(got) != bits(ref))
    assert not wrong.any(), ("exact entries", np.argwhere(wrong)[:8].tolist(), got[wrong][:8], ref[wrong][:8])
    err = np.abs(got[touched].astype(np.float64) - ref[touched])
    print(f"V={V} B={B} {layout}: {int(touched.sum())} rounded logits, max err / tol = {float((err / tol[touched]).max()) if err.size else 0.0:.3f}")
    assert (err <= tol[touched]).all(), (float(err.max()), np.argwhere(touched)[np.argmax(err / tol[touched])].tolist())
    for b, r in enumerate(rows):
        if r.get("finished") or not r.get("row_on", True) or not lref.has_options(**{k: v for k, v in r.items() if k in (
                "presence", "frequency", "bias", "min_new", "bad_words", "mask")}):
            assert (bits(got[b]) == bits(logits[b])).all(), ("an unprocessed row keeps its bits", b)
    if B >= 9:  # the guard rows: exactly end_id finite, at 0
        for b in (7, 8):
            fin = np.isfinite(got[b])
            assert fin.sum() == 1 and fin[END_ID[V]] and got[b, END_ID[V]] == 0.0, b


@pytest.mark.parametrize("V", [97, 4129, 100864])
def test_result_does_not_depend_on_the_launch_shape(V):
    rows, logits, ref, touched, tol = case(V, 16)
    base = launch(rows, logits, V, "row_major")
    for slice_ in (32, 96, 4096):
        assert (bits(launch(rows, logits, V, "row_major", slice_=slice_)) == bits(base)).all(), slice_
    assert (bits(launch(rows, logits, V, "time_major")) == bits(base)).all(), "both layouts, the same bits"


def test_bad_arguments_are_refused():
    import torch
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    lg = torch.zeros(97, device="cuda")
    a = capi.LogitProcessArgs()
    a.struct_size, a.batch_size, a.vocab_size, a.end_id, a.logits = C.sizeof(a), 1, 97, 2, lg.data_ptr()
    assert capi.lib().ftcf_logit_process(C.byref(a), None) == 0  # no option at all: nothing to do
    for field, value in (("struct_size", 8), ("end_id", 97), ("slice", 48), ("slice", 8192), ("batch_size", 0)):
        b = capi.LogitProcessArgs.from_buffer_copy(a)
        setattr(b, field, value)
        assert capi.lib().ftcf_logit_process(C.byref(b), None) == -1, field
    torch.cuda.synchronize()
    assert float(lg.abs().sum()) == 0.0
