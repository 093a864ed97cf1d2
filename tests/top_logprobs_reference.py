"""A float64 statement of top_logprobs (include/ftcf.h): the N best (id, log-probability) pairs of the distribution a
dynamic-decode step samples from -- the row after the optional-token mask, temperature, repetition penalty and min-length
mask, before top-k / top-p truncation.

The processed row is built as tests/decode_reference.py sampling_step builds it (its helpers are imported, its text is not
changed): every penalty stores fp32, so the ORDER of a row is an order of fp32 numbers and ties are exact ties.  Everything
after it is float64: the row's maximum, the denominator with the layer's + 1e-6, the logarithm.

Rules: log-probability descending, equal values by id ascending (-0.0 == +0.0); masked entries (a processed logit of -inf or
<= -FLT_MAX) follow every other entry, by id ascending, with -inf; with V < N the trailing pairs are (-1, -inf).

Rows of the top-p layer.  The kernels find such a row as fp32 PROBABILITIES and order those, so two different logits whose
log-probabilities differ by less than LP_TOL's atol cannot be told apart there (`excused`: the positions may swap), and an
entry below exp(-80) is a probability of 0 there (`well_posed` False: the row is left out).  Both are properties of the
inputs alone and are counted by tests/test_top_logprobs_reference.py.
"""
import numpy as np

from tests import decode_reference as ref

NS = (1, 5, 20)
TOPP_FLOOR = -80.0  # log-probability below which an fp32 probability may be 0 (FLT_MIN is exp(-87.3))


def processed_row(case, b):
    """(row b after step 1 of sampling_step as float64 of the stored fp32 values, is the row the top-p layer's)"""
    B, V = case.B, case.V
    k_eff, _, _ = ref.route(case.top_k, case.top_p, B)
    temp = ref._bc(case.temperature, B, np.float32, 1.0).astype(np.float64)
    rep = ref._bc(case.repetition_penalty, B, np.float32, 1.0).astype(np.float64)
    minl = ref._bc(case.min_length, B, np.int64, 0)
    apply_temperature = bool(np.any(temp != 1.0))
    apply_repetition = case.repetition_penalty is not None and bool(np.any(rep != 1.0))
    st = int(case.row_len[b]) + 1 if case.row_len is not None else int(case.step)
    in_len, mil = case.input_lengths.astype(np.int64), case.max_input_len
    l = case.logits[b].astype(np.float64)
    if case.optional_last_tokens is not None and st == mil:
        allow = np.zeros(V, bool)
        for t in case.optional_last_tokens[b]:
            if 0 <= t < V:
                allow[t] = True
        l[~allow] = -np.inf
    if apply_temperature:
        l = ref.stored(l * ref.stored(1.0 / ref.stored(temp[b] + ref.stored(1e-6))))
    if apply_repetition and st > 1:
        hist = [int(case.output_ids[t, b]) for t in range(st) if not (in_len[b] <= t < mil)]
        before = l.copy()
        for t in set(hist):
            l[t] = ref.stored(before[t] * rep[b]) if before[t] < 0.0 else ref.stored(before[t] / rep[b])
    if case.min_length is not None and int(case.seq_len[b]) + 1 - mil < minl[b]:
        l[case.end_id] = -ref.FLT_MAX
    return l, bool(k_eff[b] == 0)


def top_n(row, N, topp=False, atol=2e-4):
    """row: the processed logits (float64).  Returns a dict: ids [N] int64, log_probs [N] float64, excused [N] bool (top-p rows:
    positions that may swap with a neighbour), clusters (lists of ids an excused position may hold), well_posed."""
    l = np.asarray(row, dtype=np.float64)
    V = l.size
    masked = ~(l > -ref.FLT_MAX)
    with np.errstate(over="ignore", invalid="ignore"):
        mx = l.max()
        e = np.where(masked, 0.0, np.exp(l - mx))
        lse = np.log(e.sum() + 1e-6)
        lp = np.where(masked, -np.inf, (l - mx) - lse)
    live = ref.best_first(np.where(masked, -np.inf, l))[:int((~masked).sum())]
    order = np.concatenate([live, np.nonzero(masked)[0]]).astype(np.int64)
    ids = np.full(N, -1, np.int64)
    vals = np.full(N, -np.inf)
    n = min(N, V)
    ids[:n] = order[:n]
    vals[:n] = lp[order[:n]]
    excused = np.zeros(N, bool)
    clusters = {}
    well_posed = True
    if topp:
        head = live[:N + 1]  # the first N + 1 unmasked entries decide what the first N places hold
        hv = lp[head]
        well_posed = bool(np.all(hv > TOPP_FLOOR))
        dl = np.diff(l[head]) if head.size > 1 else np.zeros(0)
        close = (dl != 0.0) & (np.abs(np.diff(hv)) < atol) if head.size > 1 else np.zeros(0, bool)
        link = close | (dl == 0.0)  # (exact ties next to a close pair move with it)
        i = 0
        while i < link.size:
            if not link[i]:
                i += 1
                continue
            j = i
            while j < link.size and link[j]:
                j += 1
            if close[i:j].any():  # entries i .. j of the head are one run
                members = [int(t) for t in head[i:j + 1]]
                if j == link.size:  # the run reaches the end of the head: the entries that tie with its last one belong to it
                    tail = live[head.size:]
                    members += tail[l[tail] == l[head[-1]]].tolist()
                for pos in range(i, min(j + 1, N)):
                    excused[pos] = True
                    clusters[pos] = members
            i = j
    return dict(ids=ids, log_probs=vals, excused=excused, clusters=clusters, well_posed=well_posed)


def case_top_n(case, N, atol=2e-4):
    """the pairs of every row of a decode_cases.Case (finished rows: None)"""
    out = []
    for b in range(case.B):
        if case.finished[b]:
            out.append(None)
            continue
        l, topp = processed_row(case, b)
        r = top_n(l, N, topp, atol)
        r["topp"], r["row"] = topp, l
        out.append(r)
    return out
