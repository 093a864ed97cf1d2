"""A float64 statement of ONE step of the dynamic-decode layer (beam_width 1) and of ONE beam-search step, in plain numpy.

It shares no code with oracle/ftcf_oracle.c: the CPU test (test_decode_step_reference.py) holds the oracle's fp32 result
against this module, the GPU test (test_gpu_decode_step.py) holds the HIP kernels against both.

What is stated in the layer's own number format and what in float64:

* The logits are an fp32 BUFFER that the penalties modify in place, so every penalty stores fp32: `stored()` rounds the
  float64 result of one multiplication / division of two fp32 numbers to fp32, which is the fp32 operation exactly (the
  product is exact in float64, and float64 carries more than 2 * 24 + 2 bits, so the double rounding of a quotient is
  innocuous).  The ORDER of a row (value descending, index ascending, -0.0 == +0.0) is therefore an order of fp32 numbers and
  has no rounding of its own; ties are exact ties.
* The probabilities a walk runs over are stored fp32 too (the top-p layer writes them over the logits, the top-k layer
  into its candidate array), and the walk's accumulator is an fp32 number: the layer promises the same additions in the same
  order as the reference, and over thousands of nearly equal terms the rounding of that accumulator moves a boundary by
  more than any margin could cover.  So the walks below add / subtract stored masses in an fp32 accumulator, in order.
* Everything else is float64: exponentials, the row's denominator (with the reference's + 1e-6), the quotient before it is
  stored, the logarithm added to cum_log_probs, the beam scores.

Knife edges.  A draw within rounding of a boundary of the walk may legitimately land on either side in an fp32
implementation, so every sampled row reports `margin`: the distance from the scaled draw to the nearest cumulative boundary
(the end of the mass included: beyond it the walk falls back to its last entry) as a share of the mass walked.  The case
tables only use seeds whose margin clears MARGIN = 2**-18 (64 fp32 ulps): the walk's scale cancels (the draw is multiplied
by the sum it is walked against) and the implementations add the same terms in the same order, which leaves a few ulps of
expf per term.  The beam step reports the same for its two selections: the smallest gap between two DIFFERENT adjacent
scores around the places taken, relative to max(1, |score|); equal scores are decided by the index, exactly.
"""
import numpy as np

MARGIN = 2.0 ** -18
FLT_MAX = float(np.finfo(np.float32).max)
_M64 = (1 << 64) - 1


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def uniform(seed, draw):
    """The draw stream of the contract: 24 bits of splitmix64(seed ^ splitmix64(draw)), in (0, 1]."""
    z = _splitmix64((int(seed) ^ _splitmix64(int(draw) & _M64)) & _M64)
    return float((z >> 40) + 1) / 16777216.0


def stored(x):
    """float64 -> the fp32 number the logits buffer holds -> float64"""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _bc(v, B, dtype, default):
    if v is None:
        return np.full(B, default, dtype=dtype)
    a = np.asarray(v, dtype=dtype).reshape(-1)
    return np.ascontiguousarray(np.broadcast_to(a, (B,)) if a.size == 1 else a, dtype=dtype)


def route(top_k, top_p, B):
    """(k, p of the top-k layer, p of the top-p layer) per row; k == 0: the row belongs to the top-p layer."""
    k_in, p_in = _bc(top_k, B, np.int64, 0), _bc(top_p, B, np.float32, 0.0).astype(np.float64)
    k_eff, p_topk, p_topp = np.zeros(B, np.int64), np.zeros(B), np.zeros(B)
    for b in range(B):
        k, p = int(k_in[b]), float(p_in[b])
        if k == 0 and p == 0.0:
            k = 1
        pk = 1.0 if (k > 0 and p == 0.0) else p
        k_eff[b] = min(k, 1024)
        p_topk[b] = min(max(pk, 0.0), 1.0)
        p_topp[b] = min(max(p, 0.0), 1.0)
    return k_eff, p_topk, p_topp


def best_first(values):
    """indices of a row, value descending, index ascending on ties (-0.0 == +0.0 is a tie)"""
    v = np.asarray(values, dtype=np.float64)
    return np.lexsort((np.arange(v.size), -v))


def _stop_word_hit(tokens_at, words_row, stop_len, step):
    """stop-words criterion: words_row [2, stop_len] = {flattened words, exclusive end offsets (-1 padded)}; tokens_at(t) is the
    row's token at time t <= step"""
    words, offs = words_row[0], words_row[1]
    for i in range(stop_len):
        if offs[i] < 0:
            continue
        start = int(offs[i - 1]) if i > 0 else 0
        size = int(offs[i]) - start
        if step + 1 >= size and all(tokens_at(step - (size - 1) + t) == int(words[start + t]) for t in range(size)):
            return True
    return False


def _walk_topk(mass, u, p):
    """The top-k layer's walk: the draw, scaled by p and by the sum of the k masses, loses one mass after the other; the first
    entry at which nothing is left is taken (the last one otherwise).  margin: what is left nearest to zero, as a share of the sum."""
    m = np.asarray(mass, dtype=np.float32)
    total = np.add.accumulate(m, dtype=np.float32)[-1]
    rnd = np.float32(np.float32(u * p) * np.float64(total))
    left = np.subtract.accumulate(np.concatenate(([rnd], m)).astype(np.float32), dtype=np.float32)[1:]
    hit = np.nonzero(left <= 0.0)[0]
    pick = int(hit[0]) if hit.size else len(m) - 1
    margin = float(np.min(np.abs(left.astype(np.float64)))) / float(total) if total > 0 else 0.0
    return pick, margin


def _walk_topp(mass, u, p):
    """The top-p layer's walk over the whole sorted row: the first entry at which the cumulative probability reaches draw * p
    (the last one otherwise).  margin: the distance from draw * p to the nearest cumulative value, as a share of the row's mass."""
    m = np.asarray(mass, dtype=np.float32)
    c = np.add.accumulate(m, dtype=np.float32)
    rnd = np.float32(u * p)
    hit = np.nonzero(rnd <= c)[0]
    pick = int(hit[0]) if hit.size else len(m) - 1
    margin = float(np.min(np.abs(np.float64(rnd) - c.astype(np.float64)))) / float(c[-1]) if c[-1] > 0 else 0.0
    return pick, margin


def sampling_step(logits, step, max_input_len, input_lengths, end_id, output_ids, finished, seq_len, cum_log_probs,
                  draw_counter, *, total_len, top_k=None, top_p=None, temperature=None, repetition_penalty=None,
                  min_length=None, random_seed=None, stop_words=None, optional_last_tokens=None,
                  return_cum_log_probs=True, row_len=None, finish=True, pad_count=None):
    """One step on copies of the state; returns a dict.  logits [B, V] fp32, output_ids time-major [rows, B]."""
    logits = np.asarray(logits)
    assert logits.dtype == np.float32
    B, V = logits.shape
    l_all = logits.astype(np.float64)
    ids = np.array(output_ids, dtype=np.int64, copy=True)
    fin = np.array(finished, dtype=np.uint8, copy=True)
    slen = np.array(seq_len, dtype=np.int64, copy=True)
    cum = np.array(cum_log_probs, dtype=np.float64, copy=True)
    draws = np.array(draw_counter, dtype=np.uint64, copy=True)
    pads = np.zeros(B, np.int64) if pad_count is None else np.array(pad_count, dtype=np.int64, copy=True)
    in_len = np.asarray(input_lengths, dtype=np.int64)
    k_eff, p_topk, p_topp = route(top_k, top_p, B)
    temp = _bc(temperature, B, np.float32, 1.0).astype(np.float64)
    rep = _bc(repetition_penalty, B, np.float32, 1.0).astype(np.float64)
    minl = _bc(min_length, B, np.int64, 0)
    seeds = _bc(random_seed, B, np.uint64, 0)
    # a penalty is on for the whole batch as soon as one row differs from its default
    apply_temperature = bool(np.any(temp != 1.0))
    apply_repetition = repetition_penalty is not None and bool(np.any(rep != 1.0))
    tokens, step_lp, margin = np.zeros(B, np.int64), np.zeros(B), np.full(B, np.inf)
    for b in range(B):
        st = int(row_len[b]) + 1 if row_len is not None else int(step)
        l = l_all[b].copy()
        # 1. masks and penalties
        if optional_last_tokens is not None and st == max_input_len:
            allow = np.zeros(V, bool)
            for t in np.asarray(optional_last_tokens)[b]:
                if 0 <= t < V:
                    allow[t] = True
            l[~allow] = -np.inf
        if apply_temperature:
            inv = stored(1.0 / stored(temp[b] + stored(1e-6)))
            l = stored(l * inv)
        if apply_repetition and st > 1:
            hist = [int(ids[t, b]) for t in range(st) if not (in_len[b] <= t < max_input_len)]
            before = l.copy()  # every history token is penalised once, from the value it had
            for t in set(hist):
                l[t] = stored(before[t] * rep[b]) if before[t] < 0.0 else stored(before[t] / rep[b])
        if min_length is not None and slen[b] + 1 - max_input_len < minl[b]:
            l[end_id] = -FLT_MAX
        was_finished = bool(fin[b])
        if k_eff[b] > 0:
            # 3. the top-k layer
            if was_finished:  # the end mask: the row emits end_id, nothing else moves
                tokens[b] = end_id
                ids[st, b] = end_id
                continue
            order = best_first(l)[:min(int(k_eff[b]), V)]
            if return_cum_log_probs:
                mx = l.max()
                mass = np.exp(l[order] - mx) / (np.exp(l - mx).sum() + 1e-6)
            else:
                mass = np.exp(l[order] - l[order[0]])
            u = uniform(seeds[b], draws[b])
            draws[b] += np.uint64(1)
            pick, margin[b] = _walk_topk(mass, u, p_topk[b])
        else:
            # 4. the top-p layer: the walk runs over the whole sorted row, finished rows included (their row is the end mask)
            if was_finished:
                l = np.where(np.arange(V) == end_id, FLT_MAX, -FLT_MAX)
            mx = l.max()
            e = np.exp(l - mx)
            q = e / (e.sum() + 1e-6)
            order = best_first(q if was_finished else l)
            mass = q[order]
            u = uniform(seeds[b], draws[b])
            draws[b] += np.uint64(1)
            pick, margin[b] = _walk_topp(mass, u, p_topp[b])
        tok = int(order[pick])
        tokens[b] = tok
        ids[st, b] = tok
        # 5. the log-probability added (the + 1e-6 of the denominator included: a one-hot row adds about -1e-6, not 0)
        if return_cum_log_probs:
            step_lp[b] = np.log(mass[pick]) if mass[pick] > 0 else -np.inf
            cum[b] += step_lp[b]
        if not was_finished:
            slen[b] += 1
        fin[b] = 1 if tok == end_id else 0
    out = dict(tokens=tokens, output_ids=ids, finished=fin, seq_len=slen, cum_log_probs=cum, step_log_probs=step_lp,
               draw_counter=draws, margin=margin, pad_count=pads, all_finished=0, next_step=int(step))
    if not finish:
        return out
    # 6. the bookkeeping
    for b in range(B):
        if stop_words is not None:
            sw = np.asarray(stop_words)
            if _stop_word_hit(lambda t: int(ids[t, b]), sw[b], sw.shape[2], int(step)):
                fin[b] = 1
        if step >= total_len:
            fin[b] = 1
        if step == max_input_len:
            pads[b] += max_input_len - in_len[b]
    out["all_finished"] = int(bool(np.all(fin != 0)))
    out["next_step"] = int(step) + 1
    return out


def _min_gap(sorted_scores, places):
    """smallest gap between two different adjacent scores among the first places + 1, relative to max(1, |score|)"""
    s = np.asarray(sorted_scores, dtype=np.float64)[:places + 1]
    s = s[np.isfinite(s)]
    if s.size < 2:
        return np.inf
    d = np.abs(np.diff(s))
    rel = d / np.maximum(1.0, np.abs(s[:-1]))
    rel = rel[d > 0]
    return float(rel.min()) if rel.size else np.inf


def beam_step(logits, K, step, max_input_len, input_lengths, end_id, output_ids, parent_ids, finished, seq_len,
              cum_log_probs, src_indir, tgt_indir, *, temperature=None, repetition_penalty=None, diversity_rate=None,
              len_penalty=None, min_length=None, stop_words=None, optional_last_tokens=None):
    """One beam-search step on copies of the state; rows bb = batch * K + beam.  logits [B * K, V] fp32, output_ids /
    parent_ids time-major [total, B * K], src_indir / tgt_indir [B, K, s_max]."""
    logits = np.asarray(logits)
    assert logits.dtype == np.float32
    BK, V = logits.shape
    B = BK // K
    ids = np.array(output_ids, dtype=np.int64, copy=True)
    par = np.array(parent_ids, dtype=np.int64, copy=True)
    old_fin = np.array(finished, dtype=np.uint8, copy=True)
    old_len = np.array(seq_len, dtype=np.int64, copy=True)
    old_cum = np.asarray(cum_log_probs, dtype=np.float64)
    in_len = np.asarray(input_lengths, dtype=np.int64)
    src = np.asarray(src_indir, dtype=np.int64).reshape(B, K, -1)
    tgt = np.array(tgt_indir, dtype=np.int64, copy=True).reshape(B, K, -1)
    s_max = src.shape[2]
    temp = _bc(temperature, B, np.float32, 1.0).astype(np.float64)
    rep = _bc(repetition_penalty, B, np.float32, 1.0).astype(np.float64)
    div = _bc(diversity_rate, B, np.float32, 0.0).astype(np.float64)
    lenp = _bc(len_penalty, B, np.float32, 0.0).astype(np.float64)
    minl = _bc(min_length, B, np.int64, 0)
    fin, slen, cum = old_fin.copy(), old_len.copy(), old_cum.copy()
    margin = np.inf
    new_parent = np.zeros(BK, np.int64)
    for b in range(B):
        cand_score, cand_tok = np.zeros((K, K)), np.zeros((K, K), np.int64)
        for k in range(K):
            bb = b * K + k
            l = logits[bb].astype(np.float64)
            if optional_last_tokens is not None and step == max_input_len:
                allow = np.zeros(V, bool)
                for t in np.asarray(optional_last_tokens)[b]:
                    if 0 <= t < V:
                        allow[t] = True
                l[~allow] = -np.inf
            if temp[b] != 1.0:
                l = stored(l * stored(1.0 / stored(temp[b] + stored(1e-6))))
            if repetition_penalty is not None and step > 0 and rep[b] != 1.0:
                # the history of THIS beam: its last token, then along the parent chain (padding positions skipped)
                hist, parent = [int(ids[step - 1, bb])], k
                for t in range(step - 2, -1, -1):
                    if in_len[bb] <= t < max_input_len:
                        continue
                    parent = int(par[t, b * K + parent])
                    hist.append(int(ids[t, b * K + parent]))
                before = l.copy()
                for t in set(hist):
                    l[t] = stored(before[t] / rep[b]) if before[t] > 0.0 else stored(before[t] * rep[b])
            if step - max_input_len < minl[b] and old_len[bb] + 1 - max_input_len < minl[b]:
                l[end_id] = -FLT_MAX
            if old_fin[bb]:  # a finished beam offers its end token at its score and nothing else
                ls = np.where(np.arange(V) == end_id, 0.0, -np.inf)
            else:
                mx = l.max()
                ls = (l - mx) - np.log(np.exp(l - mx).sum())
            order = best_first(ls if old_fin[bb] else l)
            margin = min(margin, _min_gap(ls[order], K))
            cand_tok[k] = order[:K]
            cand_score[k] = ls[order[:K]] + old_cum[bb]
        # the K best of the batch entry's K * K candidates.  The length of the penalty is read at the BATCH index, as the
        # reference's kernel does (only matters with len_penalty != 0)
        flat = cand_score.reshape(-1)
        score = flat.copy()
        length = int(old_len[b]) if old_fin[b] else int(old_len[b]) + 1
        if lenp[b] != 0.0 and length != 1:
            score = score / np.power(float(length), lenp[b])
        score = score + div[b] * (np.arange(K * K) % K)
        order = best_first(score)
        margin = min(margin, _min_gap(score[order], K))
        for r in range(K):
            e = int(order[r])
            bb, pk = b * K + r, e // K
            pb = b * K + pk
            new_parent[bb] = pk
            tok = int(cand_tok.reshape(-1)[e])
            ids[step, bb] = tok
            par[step, bb] = pk
            cum[bb] = flat[e]
            slen[bb] = old_len[pb] if old_fin[pb] else old_len[pb] + 1
            fin[bb] = 1 if tok == end_id else 0
    # the cache indirection: rows that just finished keep their stale entries
    for bb in range(BK):
        if fin[bb]:
            continue
        b, k = divmod(bb, K)
        for t in range(min(step + 1, s_max)):
            tgt[b, k, t] = k if t == step else src[b, new_parent[bb], t]
    if stop_words is not None:
        sw = np.asarray(stop_words)
        for bb in range(BK):
            b = bb // K
            chain = {}
            parent = bb % K
            for t in range(step, -1, -1):  # the row's tokens along the parent chain
                chain[t] = int(ids[t, b * K + parent])
                parent = int(par[t, b * K + parent])
            if _stop_word_hit(lambda t: chain[t], sw[b], sw.shape[2], step):
                fin[bb] = 1
    return dict(output_ids=ids, parent_ids=par, finished=fin, seq_len=slen, cum_log_probs=cum, tgt_indir=tgt, margin=margin)
