"""-m gpu: the sampled tail of a verify pass (include/ftcf.h ftcf_verify_sample: k_verify_topk_slices + k_verify_pick +
k_verify_sample_close of kernels_verify.hip) on crafted logits.  The reference is the plain sampled step itself: row i's logits go
through ftcf_dynamic_decode_step (B = 1, top_k = k, finish 1) at step st + i with the same seed on buffers that start in the same
state, the draw counter carrying on from row to row, until a row finishes or the sampled token differs from the draft; the
drafts are built from that reference's tokens.  Tokens, the written cells of output_ids, finished, seq_len, the emitted / accepted
counts and the draw counter (before + emitted) are exact; log-probabilities use LP_TOL of tests/decode_cases.py, against that
reference and against float64; every cell nothing may write keeps its sentinel, every buffer has a guard band on both sides, and
two launches give the same bits."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests.decode_cases import LP_TOL
from tests.speculative_sampled_cases import uniform
from tests.test_gpu_verify_accept import END_ID, GUARD_F, GUARD_I, INVALID_ARG, LP_SENTINEL, S0, SENTINEL, SLICES, ST, Guarded, State, stream

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

capi = None
SHAPES = [(R, V) for R in (1, 2, 5, 16) for V in (50, 257, 4099)] + [(5, 100864), (2, 131072)]
KS = (2, 5, 50, 64)
STAGE1_MAX_V = 122880  # the four-launch form of the plain step (the one a temperature takes) holds a row of at most this
TOPK_FUSED = 1         # ftcf_dynamic_decode_args.form: k_topk_decode


@pytest.fixture(scope="module", autouse=True)
def _lib():
    global capi
    from fastertransformer4codefuse_amd import capi as _c
    capi = _c
    capi.require_gpu()
    yield


def scaled(logits, T):
    """the logits as the kernels read them under a temperature (k_decode_prep's expression, fp32)"""
    l = np.asarray(logits, np.float32)
    return l if T == 1.0 else l * (np.float32(1.0) / (np.float32(T) + np.float32(1e-6)))


def sorted_top(row, k, T):
    """the k best of a row as the kernels order them (value descending, index ascending) -> (ids, cumulative exp(v - best), float64)"""
    l = scaled(row, T).astype(np.float64)
    order = np.lexsort((np.arange(l.size), -l))[:k]
    return order, np.cumsum(np.exp(l[order] - l[order[0]]))


def bucket(c, p, seed, draw):
    """the top-k walk restated: the bucket draw `draw` of `seed` lands in, and its distance from the nearest boundary as a fraction
    of the total"""
    x = float(uniform(seed, 0, draw)) * p * c[-1]
    b = next((j for j in range(len(c)) if x <= c[j]), len(c) - 1)
    return b, (np.abs(x - c[:-1]).min() / c[-1] if len(c) > 1 else 1.0)


class Case:
    """logits [R, V], the history output_ids[0, ST), what the top-k layer draws with, stop words or None, total_len, log-probs on;
    `drafts(tokens)` turns the reference's tokens into the pass's drafts"""

    def __init__(self, name, R, V, k):
        rng = np.random.RandomState(zlib.crc32(repr((name, R, V, k)).encode()))
        self.name, self.R, self.V, self.k = name, R, V, k
        self.total_len = ST + R + 3
        self.lp, self.T, self.p, self.base = True, 1.0, 1.0, 3
        self.seed = int(rng.randint(1, 2 ** 31 - 1))
        # quantised values (exact in fp32 and under a temperature's rounding alike on both sides; many equal ones)
        self.logits = (rng.randint(-16, 17, size=(R, V)) * 0.25).astype(np.float32)
        self.logits[:, :3] = -30.0  # tokens 0, the end token and 2 are not sampled unless a scenario makes them
        self.hist = rng.randint(3, V, size=ST).astype(np.int32)
        self.words = [[2, 2, 2]]  # a decoy: never completes
        self.wrong_at = None
        self.stop_from_tokens = None

    def peak(self, i, token):
        """row i samples `token` whatever the draw: every other candidate has probability e**-26"""
        self.logits[i] = np.minimum(self.logits[i], 4.0)
        self.logits[i, token] = 30.0

    def wrong(self, t, avoid):
        w = 3 + (int(t) - 3 + 1) % (self.V - 3)
        while w in avoid:
            w = 3 + (w - 3 + 1) % (self.V - 3)
        return w

    def drafts(self, tokens):
        d = np.zeros(max(self.R - 1, 1), np.int32)
        n = min(len(tokens), self.R - 1)
        d[:n] = tokens[:n]
        for i in range(n, self.R - 1):  # (behind a row that finished the reference: never looked at)
            d[i] = 3
        if self.wrong_at is not None and self.wrong_at < self.R - 1:
            d[self.wrong_at] = self.wrong(d[self.wrong_at], set(int(t) for t in tokens))
        return d[:self.R - 1] if self.R > 1 else d[:0]

    def stop_words(self):
        if self.words is None:
            return None
        ids = [t for w in self.words for t in w]
        ends = np.cumsum([len(w) for w in self.words]).tolist()
        out = np.zeros((2, len(ids) + 2), np.int32)
        out[0, :len(ids)] = ids
        out[1, :] = -1
        out[1, :len(ends)] = ends
        return out


def tie_block(c, i, lo, m):
    """row i: m equal values at lo .. lo + m - 1 above everything else"""
    c.logits[i] = np.minimum(c.logits[i], 3.0)
    c.logits[i, lo:lo + m] = 5.0


def find_seed(c, want):
    """the first seed from the case's own at which row 0's draw lands in a bucket `want` accepts, well inside it -> that token"""
    order, cum = sorted_top(c.logits[0], c.k, c.T)
    for seed in range(c.seed, c.seed + 20000):
        b, margin = bucket(cum, c.p, seed, c.base)
        if want(b, cum) and margin >= 1e-3:
            c.seed = seed
            return int(order[b])
    raise AssertionError("no seed lands where the scenario wants it")


def build(name, R, V, k):
    c = Case(name, R, V, k)
    mid = (R - 1) // 2
    sl = (V + SLICES - 1) // SLICES
    m = k + 2
    c.row0_token = None
    if name == "all drafts right":
        pass
    elif name == "draft 0 wrong":
        c.wrong_at = 0
    elif name == "a wrong draft in the middle":
        c.wrong_at = mid
    elif name == "equal values straddling the k-th place in one slice":
        # rows 0 and R - 1: k + 2 equal values (one slice where a slice is that long); the k with the lowest indices are the candidates
        for i in {0, R - 1}:
            tie_block(c, i, 3 * sl if sl >= m and 3 * sl + m <= V else 3, m)
    elif name == "equal values straddling the k-th place across a slice boundary":
        for i in {0, R - 1}:
            lo = 5 * sl - m // 2 if 5 * sl + m <= V and 5 * sl - m // 2 >= 3 else max(3, min(sl - 1, V - m))
            tie_block(c, i, lo, m)
    elif name == "equal values next to the pick":
        # three candidates in front, three equal ones behind them, everything else below: whatever is picked has an equal neighbour
        for i in range(R):
            c.logits[i] = np.minimum(c.logits[i], 3.0)
            spread = np.linspace(3, V - 1, 6).astype(int)
            c.logits[i, spread[::2]] = 5.0
            c.logits[i, spread[1::2]] = 4.75
    elif name == "a draw in the last bucket, counter above 2**32":
        c.base = 2 ** 32 + 5
        if k > V - 3:
            c.logits[0, :3] = (np.arange(3) - 16) * 0.25  # (every token is a candidate: the last one must be reachable)
        c.row0_token = find_seed(c, lambda b, cum: b == k - 1)
    elif name == "top_p_topk 0.5":
        c.p = 0.5
        # behind the best candidate, unless that one alone holds the half of the mass the walk is confined to (always so with k = 2)
        c.row0_token = find_seed(c, lambda b, cum: b >= 1 or cum[0] >= 0.499 * cum[-1])
    elif name == "temperature 0.7":
        c.T = 0.7
    elif name == "no log-prob buffer and no stop words":
        c.lp, c.words = False, None
    elif name == "end_id sampled inside the accepted run":
        c.peak(min(1, R - 1), END_ID)
    elif name == "end_id sampled at the end of the accepted run":
        c.wrong_at = mid
        c.peak(mid, END_ID)
    elif name == "end_id sampled beyond the accepted run":
        c.wrong_at = mid if R > 1 else None
        if R > 1:
            c.peak(R - 1, END_ID)
    elif name == "a stop word straddling history and pass":
        c.stop_from_tokens = lambda tokens: [int(c.hist[ST - 2]), int(c.hist[ST - 1]), int(tokens[0])]
    elif name == "the pass ends exactly at total_len":
        c.total_len = ST + R
    else:
        raise KeyError(name)
    return c


NAMES = ["all drafts right", "draft 0 wrong", "a wrong draft in the middle", "equal values straddling the k-th place in one slice",
         "equal values straddling the k-th place across a slice boundary", "equal values next to the pick",
         "a draw in the last bucket, counter above 2**32", "top_p_topk 0.5", "temperature 0.7", "no log-prob buffer and no stop words",
         "end_id sampled inside the accepted run", "end_id sampled at the end of the accepted run",
         "end_id sampled beyond the accepted run", "a stop word straddling history and pass", "the pass ends exactly at total_len"]


def counter(base):
    return Guarded(np.array([base], np.int64), np.int64(GUARD_I))


def plain_steps(c, st, draws, logits, step0, draft):
    """the reference: one ftcf_dynamic_decode_step per row from the state `st`, until a row finishes or the sampled token is not
    the draft (draft None: every row) -> (emitted, accepted, tokens)"""
    pads = torch.zeros(1, dtype=torch.int32, device="cuda")
    in_len = torch.tensor([S0], dtype=torch.int32, device="cuda")
    top_k, top_p = np.array([c.k], np.int32), np.array([0.0 if c.p == 1.0 else c.p], np.float32)
    seed, temp = np.array([c.seed], np.uint64), np.array([c.T], np.float32)
    host_scale = c.T != 1.0 and c.V > STAGE1_MAX_V  # (no plain step takes such a row under a temperature: scaled here, the same product)
    emitted = accepted = 0
    tokens = []
    for i in range(len(logits)):
        row = Guarded(scaled(logits[i:i + 1], c.T) if host_scale else logits[i:i + 1], np.float32(GUARD_F))
        all_finished, next_step, form = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        a = capi.DynamicDecodeArgs()
        a.logits, a.output_ids, a.finished, a.seq_len = row.ptr, st.ids.ptr, st.fin.ptr, st.slen.ptr
        a.cum_log_probs = st.cum.ptr if c.lp else None
        a.output_log_probs = st.olp.ptr if c.lp else None
        a.draw_counter, a.pad_count, a.input_lengths = draws.ptr, pads.data_ptr(), in_len.data_ptr()
        a.stop_words, a.stop_len = (st.sw.data_ptr() if st.sw is not None else None), st.stop_len
        a.top_k, a.n_top_k, a.top_p, a.n_top_p = top_k.ctypes.data, 1, top_p.ctypes.data, 1
        a.random_seed, a.n_random_seed = seed.ctypes.data, 1
        if c.T != 1.0 and not host_scale:
            a.temperature, a.n_temperature = temp.ctypes.data, 1
        a.all_finished, a.next_step, a.form = C.pointer(all_finished), C.pointer(next_step), C.pointer(form)
        a.B, a.V, a.step, a.max_input_len, a.total_len, a.end_id = 1, c.V, step0 + i, S0, c.total_len, END_ID
        a.return_cum_log_probs, a.finish = int(c.lp), 1
        capi.check(capi.lib().ftcf_dynamic_decode_step(C.byref(a), stream()))
        torch.cuda.synchronize()
        if c.T == 1.0 or host_scale:
            assert form.value == TOPK_FUSED  # the plain step of such a request: k_topk_decode
        emitted += 1
        tok = int(st.ids.read()[step0 + i])
        tokens.append(tok)
        hit = draft is None or (i < len(logits) - 1 and tok == int(draft[i]))
        accepted += 1 if (hit and draft is not None) else 0
        if all_finished.value or not hit:
            break
    return emitted, accepted, tokens


def sample_args(c, st, draws, logits, draft, ws, emitted, accepted, tokens, step, R):
    a = capi.VerifySampleArgs()
    a.struct_size = C.sizeof(capi.VerifySampleArgs)
    a.R, a.V, a.step, a.end_id, a.max_input_len, a.total_len = R, c.V, step, END_ID, S0, c.total_len
    a.logits, a.draft, a.output_ids = logits.ptr, (draft.ptr if R > 1 else None), st.ids.ptr
    a.stop_words, a.stop_len = (st.sw.data_ptr() if st.sw is not None else None), st.stop_len
    a.finished, a.seq_len = st.fin.ptr, st.slen.ptr
    a.cum_log_probs = st.cum.ptr if c.lp else None
    a.output_log_probs = st.olp.ptr if c.lp else None
    a.workspace, a.workspace_bytes = ws.ptr, capi.VERIFY_SAMPLE_WORKSPACE_BYTES
    a.emitted, a.accepted, a.tokens = emitted.ptr, accepted.ptr, tokens.ptr
    a.top_k, a.top_p_topk, a.temperature, a.random_seed, a.draw_counter = c.k, c.p, c.T, c.seed, draws.ptr
    return a


def verify_sample(c, st, draws, logits_np, step, draft_np):
    R = len(logits_np)
    logits = Guarded(logits_np, np.float32(GUARD_F))
    draft = Guarded(draft_np if R > 1 else np.zeros(1, np.int32), np.int32(GUARD_I))
    ws = Guarded(np.zeros(capi.VERIFY_SAMPLE_WORKSPACE_BYTES // 4, np.float32), np.float32(GUARD_F))
    emitted, accepted = Guarded(np.array([SENTINEL], np.int32), np.int32(GUARD_I)), Guarded(np.array([SENTINEL], np.int32), np.int32(GUARD_I))
    tokens = Guarded(np.full(16, SENTINEL, np.int32), np.int32(GUARD_I))
    a = sample_args(c, st, draws, logits, draft, ws, emitted, accepted, tokens, step, R)
    capi.check(capi.lib().ftcf_verify_sample(C.byref(a), stream()))
    torch.cuda.synchronize()
    assert np.array_equal(logits.read().view(np.uint32), logits_np.view(np.uint32)), "the logits are read only"
    draft.read()
    ws.read()
    return int(emitted.read()[0]), int(accepted.read()[0]), tokens.read().copy()


def float64_log_probs(c, logits, tokens):
    x = scaled(logits[:len(tokens)], c.T).astype(np.float64)
    mx = x.max(axis=1, keepdims=True)
    v = x[np.arange(len(tokens)), tokens][:, None]
    return np.log(np.exp(v - mx) / (np.exp(x - mx).sum(axis=1, keepdims=True) + 1e-6))[:, 0]


def one_pass(c):
    """-> (the reference's result, the tail's, the tail's again, the pass's drafts)"""
    # the tokens the reference samples when every draft is right (no stop word but the decoy yet): the drafts come from them
    _, _, free = plain_steps(c, State(c), counter(c.base), c.logits, ST, None)
    if c.stop_from_tokens is not None:
        c.words.append(c.stop_from_tokens(free))
    draft = c.drafts(free)
    st, draws = State(c), counter(c.base)
    e, acc, toks = plain_steps(c, st, draws, c.logits, ST, draft if c.R > 1 else np.zeros(0, np.int32))
    ref = st.read()
    ref.update(emitted=e, accepted=acc, tokens=toks, draws=int(draws.read()[0]))
    out = []
    for _ in range(2):
        st, draws = State(c), counter(c.base)
        ge, ga, gt = verify_sample(c, st, draws, c.logits, ST, draft)
        got = st.read()
        got.update(emitted=ge, accepted=ga, tokens=gt, draws=int(draws.read()[0]))
        out.append(got)
    return ref, out[0], out[1], draft


def check_pass(c, ref, got, again, step0=ST):
    logits = c.logits
    e = ref["emitted"]
    # exact: counts, the draw counter, tokens, every cell of output_ids (the unwritten ones hold the sentinel in both), finished, seq_len
    assert (got["emitted"], got["accepted"]) == (e, ref["accepted"])
    assert got["draws"] == ref["draws"]
    assert np.array_equal(got["output_ids"], ref["output_ids"])
    assert got["output_ids"][step0:step0 + e].tolist() == ref["tokens"] and (got["output_ids"][step0 + e:] == SENTINEL).all()
    assert got["tokens"][:e].tolist() == ref["tokens"] and (got["tokens"][e:] == SENTINEL).all()
    assert got["finished"][0] == ref["finished"][0] and got["seq_len"][0] == ref["seq_len"][0] == step0 - 1 + e
    if c.lp:
        lp64 = float64_log_probs(c, logits, ref["tokens"])
        rows = slice(step0 - S0, step0 - S0 + e)
        np.testing.assert_allclose(got["olp"][rows], ref["olp"][rows], **LP_TOL)
        np.testing.assert_allclose(got["olp"][rows], lp64, **LP_TOL)
        np.testing.assert_allclose(got["cum"], ref["cum"], **LP_TOL)
        assert (got["olp"][step0 - S0 + e:] == LP_SENTINEL).all() and (ref["olp"][step0 - S0 + e:] == LP_SENTINEL).all()
        assert (got["olp"][:ST - S0] == LP_SENTINEL).all()
        # cum_log_probs is the sequential fp32 sum of the stored values
        acc = np.float32(-1.25)
        for v in got["olp"][ST - S0:step0 - S0 + e]:
            acc = np.float32(acc + v)
        assert acc.view(np.uint32) == got["cum"].view(np.uint32)[0]
    else:
        assert got["cum"][0] == np.float32(-1.25) and (got["olp"] == LP_SENTINEL).all()
    # two launches: identical bits
    for key in ("output_ids", "finished", "seq_len", "cum", "olp", "tokens"):
        assert np.array_equal(got[key].view(np.uint8), again[key].view(np.uint8)), key
    assert (got["emitted"], got["accepted"], got["draws"]) == (again["emitted"], again["accepted"], again["draws"])


def scenario_cases():
    out = []
    for si, (R, V) in enumerate(SHAPES):
        ks = [k for k in KS if k <= V]
        for ni, name in enumerate(NAMES):
            out.append(pytest.param(R, V, ks[(si + ni) % len(ks)], name, id=f"{name}-R{R}-V{V}"))
    # every k at every shape once more, where slices are shorter than k (V = 50, k = 50) and where they are not
    for R, V in SHAPES:
        for k in KS:
            if k <= V:
                out.append(pytest.param(R, V, k, "all drafts right", id=f"every k-R{R}-V{V}-k{k}"))
    return out


@pytest.mark.parametrize("R,V,k,name", scenario_cases())
def test_a_sampled_pass_closes_as_the_plain_sampled_steps_do(R, V, k, name):
    c = build(name, R, V, k)
    ref, got, again, draft = one_pass(c)
    e, toks = ref["emitted"], ref["tokens"]
    print(f"[{name} R {R} V {V} k {k}: emitted {got['emitted']} (plain {e}) accepted {got['accepted']} (plain {ref['accepted']}) "
          f"draws {got['draws'] - c.base} cum {got['cum'][0]!r} (plain {ref['cum'][0]!r})] ", end="")
    assert ref["draws"] == c.base + e, "one draw per emitted token"
    mid = (R - 1) // 2
    # what the scenario is about
    if name in ("all drafts right", "the pass ends exactly at total_len", "no log-prob buffer and no stop words", "temperature 0.7",
                "equal values next to the pick") or name.startswith("equal values straddling"):
        assert e == R and ref["accepted"] == R - 1
    if name in ("draft 0 wrong", "a wrong draft in the middle") and R > 1:
        assert e == c.wrong_at + 1 and ref["accepted"] == c.wrong_at and ref["finished"][0] == 0
    if name.startswith("equal values straddling"):
        for i in {0, R - 1}:  # the k lowest indices of the k + 2 equal values
            lo = int(np.argmax(c.logits[i] == 5.0))
            assert lo <= toks[i] < lo + k
    if name == "equal values next to the pick":
        assert all(c.logits[i, t] in (5.0, 4.75) or k > 6 for i, t in enumerate(toks))
    if c.row0_token is not None:
        assert toks[0] == c.row0_token, "row 0's draw lands where the host walk puts it"
    if name == "end_id sampled inside the accepted run":
        assert e == min(1, R - 1) + 1 and toks[-1] == END_ID and ref["finished"][0] == 1
    if name == "end_id sampled at the end of the accepted run":
        assert e == mid + 1 and toks[-1] == END_ID and ref["finished"][0] == 1 and ref["accepted"] == mid
    if name == "end_id sampled beyond the accepted run" and R > 1:
        assert e == mid + 1 and END_ID not in toks and ref["finished"][0] == 0
    if name == "a stop word straddling history and pass":
        assert e == 1 and ref["finished"][0] == 1
    if name == "the pass ends exactly at total_len":
        assert ST + e == c.total_len
    check_pass(c, ref, got, again)


@pytest.mark.parametrize("R,V", SHAPES)
def test_a_rejected_pass_and_the_next_one_are_the_plain_steps(R, V):
    """Two calls, the second from the state the first leaves: the first pass rejects a draft in the middle (the rows behind it
    consumed no draw), the second one's rows are sampled with the draws that follow the emitted tokens."""
    k = [k for k in KS if k <= V][R % 3 if V >= 64 else R % 2]
    c = build("a wrong draft in the middle", R, V, k)
    c.total_len = ST + 2 * R + 3
    second = (np.random.RandomState(R * 131 + V).randint(-16, 17, size=(R, V)) * 0.25).astype(np.float32)
    second[:, :3] = -30.0
    _, _, free = plain_steps(c, State(c), counter(c.base), c.logits, ST, None)
    draft1 = c.drafts(free)
    # the reference: the first pass's rows up to the rejected draft, then every row of the second pass
    st, draws = State(c), counter(c.base)
    e1, a1, t1 = plain_steps(c, st, draws, c.logits, ST, draft1 if R > 1 else np.zeros(0, np.int32))
    e2, _, t2 = plain_steps(c, st, draws, second, ST + e1, None)
    ref = st.read()
    ref.update(draws=int(draws.read()[0]))
    draft2 = np.asarray((t2 + [3] * R)[:R - 1], np.int32)
    results = []
    for _ in range(2):
        st, draws = State(c), counter(c.base)
        g1 = verify_sample(c, st, draws, c.logits, ST, draft1)
        assert int(draws.read()[0]) == c.base + g1[0]
        g2 = verify_sample(c, st, draws, second, ST + g1[0], draft2)
        got = st.read()
        got.update(draws=int(draws.read()[0]), tokens=np.concatenate([g1[2], g2[2]]))
        results.append((g1, g2, got))
    g1, g2, got = results[0]
    print(f"[R {R} V {V} k {k}: first pass emitted {g1[0]} accepted {g1[1]}, second {g2[0]} / {g2[1]}] ", end="")
    assert (g1[0], g1[1], g1[2][:e1].tolist()) == (e1, a1, t1)
    assert (g2[0], g2[2][:e2].tolist()) == (e2, t2) and g2[1] == min(e2, R - 1)  # (every draft of the second pass is right)
    assert got["draws"] == ref["draws"] == c.base + e1 + e2
    e = e1 + e2
    assert np.array_equal(got["output_ids"], ref["output_ids"]) and (got["output_ids"][ST + e:] == SENTINEL).all()
    assert got["finished"][0] == ref["finished"][0] and got["seq_len"][0] == ref["seq_len"][0] == ST - 1 + e
    rows = slice(ST - S0, ST - S0 + e)
    np.testing.assert_allclose(got["olp"][rows], ref["olp"][rows], **LP_TOL)
    np.testing.assert_allclose(got["olp"][rows], np.concatenate([float64_log_probs(c, c.logits, t1), float64_log_probs(c, second, t2)]), **LP_TOL)
    np.testing.assert_allclose(got["cum"], ref["cum"], **LP_TOL)
    again = results[1][2]
    for key in ("output_ids", "finished", "seq_len", "cum", "olp", "tokens"):
        assert np.array_equal(got[key].view(np.uint8), again[key].view(np.uint8)), key


def test_bad_arguments_are_refused():
    c = build("all drafts right", 5, 257, 5)
    st, draws = State(c), counter(c.base)
    logits = Guarded(c.logits, np.float32(GUARD_F))
    draft = Guarded(np.full(4, 3, np.int32), np.int32(GUARD_I))
    ws = Guarded(np.zeros(capi.VERIFY_SAMPLE_WORKSPACE_BYTES // 4, np.float32), np.float32(GUARD_F))
    one = [Guarded(np.array([SENTINEL], np.int32), np.int32(GUARD_I)) for _ in range(2)]
    tokens = Guarded(np.full(16, SENTINEL, np.int32), np.int32(GUARD_I))
    bad = [dict(struct_size=0), dict(struct_size=C.sizeof(capi.VerifyAcceptArgs)), dict(R=0), dict(R=17), dict(logits=None),
           dict(output_ids=None), dict(workspace_bytes=capi.VERIFY_ACCEPT_WORKSPACE_BYTES), dict(step=0), dict(total_len=ST + 4),
           dict(end_id=257), dict(top_k=0), dict(top_k=65), dict(V=131073), dict(draw_counter=None), dict(top_p_topk=0.0)]
    for kw in bad:
        a = sample_args(c, st, draws, logits, draft, ws, one[0], one[1], tokens, ST, 5)
        for key, v in kw.items():
            setattr(a, key, v)
        assert capi.lib().ftcf_verify_sample(C.byref(a), stream()) == INVALID_ARG, kw
    assert capi.lib().ftcf_verify_sample(None, stream()) == INVALID_ARG
    torch.cuda.synchronize()
    # nothing was launched: every buffer is as it was
    out = st.read()
    assert (out["output_ids"][ST:] == SENTINEL).all() and out["seq_len"][0] == ST - 1 and (tokens.read() == SENTINEL).all()
    assert int(draws.read()[0]) == c.base
