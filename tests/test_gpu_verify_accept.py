"""-m gpu: the decode tail of a verify pass (include/ftcf.h ftcf_verify_accept: k_verify_slices + k_verify_close of
kernels_verify.hip) on crafted logits.  The reference is the plain step itself: row i's logits go through
ftcf_dynamic_decode_step (B = 1, top_k 1, finish 1) at step st + i on buffers that start in the same state, until a row finishes
or the model disagrees with a draft.  Tokens, the written cells of output_ids, finished, seq_len and the emitted / accepted counts
are exact; log-probabilities use LP_TOL of tests/decode_cases.py, against that reference and against a float64 restatement;
every cell nothing may write keeps its sentinel, every buffer has a guard band on both sides, and two launches give the same
bits."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests.decode_cases import LP_TOL

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

capi = None
GUARD = 256
GUARD_F, GUARD_I, SENTINEL, LP_SENTINEL = 12345.5, -99, -7, 77.0
END_ID, S0, ST = 1, 5, 9   # the end token, max_input_len, the step of the pass's first row (four generated tokens of history)
SLICES = 32                # vocabulary slices of a row (kernels.h VERIFY_ACCEPT_SLICES): where the tie cases put their maxima
INVALID_ARG = -1
SHAPES = [(R, V) for R in (1, 2, 5, 16) for V in (50, 257, 4099)] + [(5, 100864)]


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
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == self.fill).all() and (host[-GUARD:] == self.fill).all(), "a guard band was written"
        return host[GUARD:-GUARD].reshape(self.shape)


class Scenario:
    """logits [R, V], draft [R - 1], the history output_ids[0, ST), stop words [2, stop_len] or None, total_len, log-probs on"""

    def __init__(self, name, R, V):
        rng = np.random.RandomState(zlib.crc32(repr((name, R, V)).encode()))
        self.name, self.R, self.V = name, R, V
        self.total_len = ST + R + 3
        self.lp = True
        # quantised values (exact in fp32, many equal ones below the maximum), the model's token two above everything else
        self.logits = (rng.randint(-16, 17, size=(R, V)) * 0.25).astype(np.float32)
        self.a = rng.permutation(np.arange(3, V))[:R].astype(np.int32) if V - 3 >= R else rng.randint(3, V, size=R).astype(np.int32)
        self.hist = rng.randint(3, V, size=ST).astype(np.int32)
        self.set_tokens(self.a)
        self.draft = self.a[:R - 1].copy()
        self.words = [[2, 2, 2], [int(self.a[0]), 2]]  # decoys: never complete (token 2 is never generated)

    def set_tokens(self, a):
        self.a = np.asarray(a, np.int32).copy()
        for i, t in enumerate(self.a):
            self.logits[i] = np.minimum(self.logits[i], 4.0)
            self.logits[i, t] = 6.0

    def wrong(self, t):
        """another token: never the end token, never one the model emits in this pass"""
        w = 3 + (int(t) - 3 + 1) % (self.V - 3)
        while w in self.a:
            w = 3 + (w - 3 + 1) % (self.V - 3)
        return w

    def token_before(self, i):
        """the token of position ST + i - 1 (history or the pass's)"""
        return int(self.a[i - 1]) if i >= 1 else int(self.hist[ST - 1])

    def stop_words(self):
        if self.words is None:
            return None
        ids = [t for w in self.words for t in w]
        ends = np.cumsum([len(w) for w in self.words]).tolist()
        n = len(ids) + 2  # (padded: the -1 offsets are skipped)
        out = np.zeros((2, n), np.int32)
        out[0, :len(ids)] = ids
        out[1, :] = -1
        out[1, :len(ends)] = ends
        return out


def build(name, R, V):
    s = Scenario(name, R, V)
    mid = (R - 1) // 2
    sl = (V + SLICES - 1) // SLICES
    if name == "all drafts right":
        pass
    elif name == "draft 0 wrong":
        if R > 1:
            s.draft[0] = s.wrong(s.a[0])
    elif name == "a wrong draft in the middle":
        if R > 1:
            s.draft[mid] = s.wrong(s.a[mid])
    elif name == "two equal maxima in one slice":
        # rows 0 and R - 1: the maximum at two indices of ONE slice (and a third copy in a later slice); the lower index wins
        a = s.a.copy()
        for i in {0, R - 1}:
            lo = 3 * sl if sl >= 2 and 3 * sl + 1 < V else V - 2
            s.logits[i] = np.minimum(s.logits[i], 4.0)
            s.logits[i, [lo, lo + 1, V - 1]] = 6.0
            a[i] = lo
        s.a = a
        s.draft = s.a[:R - 1].copy()
        s.words = None
    elif name == "two equal maxima across a slice boundary":
        a = s.a.copy()
        for i in {0, R - 1}:
            hi = 5 * sl if 5 * sl < V else sl  # the first index of a slice: its twin is the last index of the slice below
            s.logits[i] = np.minimum(s.logits[i], 4.0)
            s.logits[i, [hi - 1, hi]] = 6.0
            a[i] = hi - 1
        s.a = a
        s.draft = s.a[:R - 1].copy()
        s.words = None
    elif name == "end_id at an accepted position":
        a = s.a.copy()
        a[min(1, R - 1)] = END_ID
        s.set_tokens(a)
        s.draft = s.a[:R - 1].copy()  # (the drafts behind it agree with the model too: they are not emitted)
    elif name == "a one-token stop word inside the accepted run":
        s.words.append([int(s.a[mid])])
    elif name == "a three-token stop word ending at accepted token 0":
        s.words.append([int(s.hist[ST - 2]), int(s.hist[ST - 1]), int(s.a[0])])
    elif name == "a three-token stop word ending at accepted token m":
        seq = s.hist.tolist() + s.a.tolist()
        s.words.append(seq[ST + R - 3:ST + R])
    elif name == "a stop word only a rejected draft would complete":
        if R > 1:
            s.draft[mid] = s.wrong(s.a[mid])
            s.words.append([s.token_before(mid), int(s.draft[mid])])
            s.words.append([int(s.draft[mid])])
    elif name == "a stop word and end_id at the same position":
        a = s.a.copy()
        a[mid] = END_ID
        s.set_tokens(a)
        s.draft = s.a[:R - 1].copy()
        s.words.append([END_ID])
    elif name == "the pass ends exactly at total_len":
        s.total_len = ST + R
    elif name == "no log-prob buffer and no stop words":
        s.lp, s.words = False, None
    else:
        raise KeyError(name)
    return s


NAMES = ["all drafts right", "draft 0 wrong", "a wrong draft in the middle", "two equal maxima in one slice",
         "two equal maxima across a slice boundary", "end_id at an accepted position", "a one-token stop word inside the accepted run",
         "a three-token stop word ending at accepted token 0", "a three-token stop word ending at accepted token m",
         "a stop word only a rejected draft would complete", "a stop word and end_id at the same position",
         "the pass ends exactly at total_len", "no log-prob buffer and no stop words"]


class State:
    """device buffers of one sequence in the state a pass (or the plain steps) starts from"""

    def __init__(self, s):
        T = s.total_len
        ids = np.full(T, SENTINEL, np.int32)
        ids[:ST] = s.hist
        self.ids = Guarded(ids, np.int32(GUARD_I))
        self.fin = Guarded(np.zeros(1, np.uint8), np.uint8(9))
        self.slen = Guarded(np.array([ST - 1], np.int32), np.int32(GUARD_I))
        self.cum = Guarded(np.array([-1.25], np.float32), np.float32(GUARD_F))
        self.olp = Guarded(np.full(T - S0, LP_SENTINEL, np.float32), np.float32(GUARD_F))
        sw = s.stop_words()
        self.sw = None if sw is None else torch.from_numpy(sw).cuda()
        self.stop_len = 0 if sw is None else sw.shape[1]

    def read(self):
        return dict(output_ids=self.ids.read().copy(), finished=self.fin.read().copy(), seq_len=self.slen.read().copy(),
                    cum=self.cum.read().copy(), olp=self.olp.read().copy())


def plain_steps(s):
    """the reference: one ftcf_dynamic_decode_step per row until a row finishes or the model disagrees with a draft"""
    st = State(s)
    draws = torch.zeros(1, dtype=torch.int64, device="cuda")
    pads = torch.zeros(1, dtype=torch.int32, device="cuda")
    in_len = torch.tensor([S0], dtype=torch.int32, device="cuda")
    top_k = np.array([1], np.int32)
    emitted = accepted = 0
    for i in range(s.R):
        row = Guarded(s.logits[i:i + 1], np.float32(GUARD_F))
        all_finished, next_step = C.c_int(-1), C.c_int(-1)
        a = capi.DynamicDecodeArgs()
        a.logits, a.output_ids, a.finished, a.seq_len = row.ptr, st.ids.ptr, st.fin.ptr, st.slen.ptr
        a.cum_log_probs = st.cum.ptr if s.lp else None
        a.output_log_probs = st.olp.ptr if s.lp else None
        a.draw_counter, a.pad_count, a.input_lengths = draws.data_ptr(), pads.data_ptr(), in_len.data_ptr()
        a.stop_words, a.stop_len = (st.sw.data_ptr() if st.sw is not None else None), st.stop_len
        a.top_k, a.n_top_k = top_k.ctypes.data, 1
        a.all_finished, a.next_step = C.pointer(all_finished), C.pointer(next_step)
        a.B, a.V, a.step, a.max_input_len, a.total_len, a.end_id = 1, s.V, ST + i, S0, s.total_len, END_ID
        a.return_cum_log_probs, a.finish = int(s.lp), 1
        capi.check(capi.lib().ftcf_dynamic_decode_step(C.byref(a), stream()))
        torch.cuda.synchronize()
        emitted += 1
        tok = int(st.ids.read()[ST + i])
        hit = i < s.R - 1 and tok == int(s.draft[i])  # (a draft that became an output token counts, also when it ends the row)
        accepted += 1 if hit else 0
        if all_finished.value or not hit:
            break
    out = st.read()
    out.update(emitted=emitted, accepted=accepted)
    return out


def accept_args(s, st, logits, draft, ws, emitted, accepted, tokens):
    a = capi.VerifyAcceptArgs()
    a.struct_size = C.sizeof(capi.VerifyAcceptArgs)
    a.R, a.V, a.step, a.end_id, a.max_input_len, a.total_len = s.R, s.V, ST, END_ID, S0, s.total_len
    a.logits, a.draft, a.output_ids = logits.ptr, (draft.ptr if s.R > 1 else None), st.ids.ptr
    a.stop_words, a.stop_len = (st.sw.data_ptr() if st.sw is not None else None), st.stop_len
    a.finished, a.seq_len = st.fin.ptr, st.slen.ptr
    a.cum_log_probs = st.cum.ptr if s.lp else None
    a.output_log_probs = st.olp.ptr if s.lp else None
    a.workspace, a.workspace_bytes = ws.ptr, capi.VERIFY_ACCEPT_WORKSPACE_BYTES
    a.emitted, a.accepted, a.tokens = emitted.ptr, accepted.ptr, tokens.ptr
    return a


def verify_accept(s):
    st = State(s)
    logits = Guarded(s.logits, np.float32(GUARD_F))
    draft = Guarded(s.draft if s.R > 1 else np.zeros(1, np.int32), np.int32(GUARD_I))
    ws = Guarded(np.zeros(capi.VERIFY_ACCEPT_WORKSPACE_BYTES // 4, np.float32), np.float32(GUARD_F))
    emitted, accepted = Guarded(np.array([SENTINEL], np.int32), np.int32(GUARD_I)), Guarded(np.array([SENTINEL], np.int32), np.int32(GUARD_I))
    tokens = Guarded(np.full(16, SENTINEL, np.int32), np.int32(GUARD_I))
    a = accept_args(s, st, logits, draft, ws, emitted, accepted, tokens)
    capi.check(capi.lib().ftcf_verify_accept(C.byref(a), stream()))
    torch.cuda.synchronize()
    assert np.array_equal(logits.read().view(np.uint32), s.logits.view(np.uint32)), "the logits are read only"
    draft.read()
    ws.read()
    out = st.read()
    out.update(emitted=int(emitted.read()[0]), accepted=int(accepted.read()[0]), tokens=tokens.read().copy())
    return out


def float64_log_probs(s, e):
    x = s.logits[:e].astype(np.float64)
    mx = x.max(axis=1, keepdims=True)
    v = x[np.arange(e), [int(np.argmax(r)) for r in x]][:, None]
    return np.log(np.exp(v - mx) / (np.exp(x - mx).sum(axis=1, keepdims=True) + 1e-6))[:, 0]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("R,V", SHAPES)
def test_a_pass_closes_as_the_plain_steps_do(R, V, name):
    s = build(name, R, V)
    ref = plain_steps(s)
    got = verify_accept(s)
    again = verify_accept(s)
    e = ref["emitted"]
    print(f"[{name} R {R} V {V}: emitted {got['emitted']} (plain {e}) accepted {got['accepted']} (plain {ref['accepted']}) "
          f"cum {got['cum'][0]!r} (plain {ref['cum'][0]!r})] ", end="")
    # what the scenario is about
    m = 0
    while m < R - 1 and s.draft[m] == s.a[m]:
        m += 1
    if name in ("all drafts right", "the pass ends exactly at total_len", "no log-prob buffer and no stop words",
                "two equal maxima in one slice", "two equal maxima across a slice boundary", "a three-token stop word ending at accepted token m"):
        assert e == R
    if name == "a stop word only a rejected draft would complete" and R > 1:
        assert e == m + 1 and ref["finished"][0] == 0
    if name == "a three-token stop word ending at accepted token 0":
        assert e == 1 and ref["finished"][0] == 1
    if name in ("a one-token stop word inside the accepted run", "a stop word and end_id at the same position"):
        assert e == (R - 1) // 2 + 1 and ref["finished"][0] == 1
    if name == "end_id at an accepted position":
        assert e == min(1, R - 1) + 1 and ref["finished"][0] == 1
    if name == "a three-token stop word ending at accepted token m":
        assert ref["finished"][0] == 1
    # exact: counts, tokens, every cell of output_ids (the unwritten ones hold the sentinel in both), finished, seq_len
    assert (got["emitted"], got["accepted"]) == (e, ref["accepted"])
    assert np.array_equal(got["output_ids"], ref["output_ids"])
    assert got["output_ids"][ST:ST + e].tolist() == s.a[:e].tolist() and (got["output_ids"][ST + e:] == SENTINEL).all()
    assert got["tokens"][:e].tolist() == s.a[:e].tolist() and (got["tokens"][e:] == SENTINEL).all()
    assert got["finished"][0] == ref["finished"][0] and got["seq_len"][0] == ref["seq_len"][0] == ST - 1 + e
    # log-probabilities
    if s.lp:
        lp64 = float64_log_probs(s, e)
        rows = slice(ST - S0, ST - S0 + e)
        np.testing.assert_allclose(got["olp"][rows], ref["olp"][rows], **LP_TOL)
        np.testing.assert_allclose(got["olp"][rows], lp64, **LP_TOL)
        np.testing.assert_allclose(got["cum"], ref["cum"], **LP_TOL)
        np.testing.assert_allclose(got["cum"][0], -1.25 + lp64.sum(), **LP_TOL)
        keep = np.ones(len(got["olp"]), bool)
        keep[rows] = False
        assert (got["olp"][keep] == LP_SENTINEL).all() and (ref["olp"][keep] == LP_SENTINEL).all()
        # cum_log_probs is the sequential fp32 sum of the stored values
        acc = np.float32(-1.25)
        for v in got["olp"][rows]:
            acc = np.float32(acc + v)
        assert acc.view(np.uint32) == got["cum"].view(np.uint32)[0]
    else:
        assert got["cum"][0] == np.float32(-1.25) and (got["olp"] == LP_SENTINEL).all()
    # two launches: identical bits
    for k in ("output_ids", "finished", "seq_len", "cum", "olp", "tokens"):
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k
    assert (got["emitted"], got["accepted"]) == (again["emitted"], again["accepted"])


def test_bad_arguments_are_refused():
    s = build("all drafts right", 5, 257)
    st = State(s)
    logits = Guarded(s.logits, np.float32(GUARD_F))
    draft = Guarded(s.draft, np.int32(GUARD_I))
    ws = Guarded(np.zeros(capi.VERIFY_ACCEPT_WORKSPACE_BYTES // 4, np.float32), np.float32(GUARD_F))
    one = [Guarded(np.array([SENTINEL], np.int32), np.int32(GUARD_I)) for _ in range(2)]
    tokens = Guarded(np.full(16, SENTINEL, np.int32), np.int32(GUARD_I))
    bad = [dict(struct_size=0), dict(struct_size=C.sizeof(capi.VerifyAcceptArgs) + 8), dict(R=0), dict(R=17), dict(logits=None),
           dict(output_ids=None), dict(workspace_bytes=16), dict(step=0), dict(total_len=ST + 4), dict(end_id=257)]
    for kw in bad:
        a = accept_args(s, st, logits, draft, ws, one[0], one[1], tokens)
        for k, v in kw.items():
            setattr(a, k, v)
        assert capi.lib().ftcf_verify_accept(C.byref(a), stream()) == INVALID_ARG, kw
    assert capi.lib().ftcf_verify_accept(None, stream()) == INVALID_ARG
    torch.cuda.synchronize()
    # nothing was launched: every buffer is as it was
    out = st.read()
    assert (out["output_ids"][ST:] == SENTINEL).all() and out["seq_len"][0] == ST - 1 and (tokens.read() == SENTINEL).all()
