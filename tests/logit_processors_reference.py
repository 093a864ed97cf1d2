"""numpy reference of the logit-processor stage (include/ftcf.h ftcf_logit_process), in float64 over fp32 inputs.

process_row(logits, ...) returns (out, touched): `out` the processed row as float64, `touched` a bool array that is True where
the arithmetic of a penalty or a bias reached the logit (those carry the fp32 roundings of the kernel; every other entry is
exactly -inf, exactly 0 at end_id from the guard, or the input value).  The order is the contract's: penalties over the generated
tokens, bias, min_new_tokens, bad words, mask, guard."""
import numpy as np


def word_list(words, length):
    """token-id lists -> the reference's [2, length] word list: ids back to back, cumulative end offsets, -1 padded"""
    flat = [t for w in words for t in w]
    assert len(flat) <= length and len(words) <= length
    arr = np.zeros((2, length), dtype=np.int32)
    arr[0, :len(flat)] = flat
    arr[1] = -1
    arr[1, :len(words)] = np.cumsum([len(w) for w in words]) if words else []
    return arr


def words_of(word_list_row):
    """the valid words of a [2, length] list: entry j needs a non-negative offset before it, so they are a prefix"""
    ids, offs = np.asarray(word_list_row[0]), np.asarray(word_list_row[1])
    out, start = [], 0
    for j in range(len(offs)):
        end = int(offs[j])
        if end < 0:
            break
        if end > start and end <= len(ids):
            out.append(ids[start:end].tolist())
        start = end
    return out


def pack_mask(allowed):
    """bool [V] -> ceil(V / 32) uint32 words, bit t of word t // 32"""
    allowed = np.asarray(allowed, dtype=bool)
    return np.packbits(np.pad(allowed, (0, -len(allowed) % 32)), bitorder="little").view(np.uint32).copy()


def has_options(presence=0.0, frequency=0.0, bias=(), min_new=0, bad_words=(), mask=None):
    return bool(presence != 0.0 or frequency != 0.0 or len(bias) > 0 or min_new > 0 or len(bad_words) > 0 or mask is not None)


def process_row(logits, history, gen_start, end_id, presence=0.0, frequency=0.0, bias=(), min_new=0, bad_words=(), mask=None,
                finished=False):
    """logits fp32 [V]; history: the row's tokens (prompt then generated), generated from gen_start on; bias: (id, value) pairs;
    bad_words: token-id lists; mask: bool [V] (True = allowed) or None"""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    V = len(x)
    touched = np.zeros(V, dtype=bool)
    history = [int(t) for t in history]
    if finished or not has_options(presence, frequency, bias, min_new, bad_words, mask):
        return x, touched
    gen_start = min(max(int(gen_start), 0), len(history))
    presence, frequency = float(np.float32(presence)), float(np.float32(frequency))
    if presence != 0.0 or frequency != 0.0:
        counts = np.bincount([t for t in history[gen_start:] if 0 <= t < V], minlength=V)
        seen = counts > 0
        x[seen] -= presence + frequency * counts[seen]
        touched |= seen
    for t, v in bias:
        if 0 <= t < V:
            x[t] += float(np.float32(v))
            touched[t] = True
    if len(history) - gen_start < min_new:
        x[end_id] = -np.inf
    for w in bad_words:
        n = len(w)
        if n == 1 or (n > 1 and len(history) >= n - 1 and history[len(history) - (n - 1):] == [int(t) for t in w[:-1]]):
            if 0 <= w[-1] < V:
                x[w[-1]] = -np.inf
    if mask is not None:
        x[~np.asarray(mask, dtype=bool)] = -np.inf
    if not np.isfinite(x).any():
        x[end_id] = 0.0
        touched[end_id] = False
    touched &= np.isfinite(x)
    return x, touched


def tolerance_row(logits, history, gen_start, presence=0.0, frequency=0.0, bias=()):
    """tolerance() of every logit of a row: the penalty of a token is presence * (c > 0) + frequency * c"""
    x = np.abs(np.asarray(logits, dtype=np.float32).astype(np.float64))
    V = len(x)
    x[~np.isfinite(x)] = 0.0
    gen_start = min(max(int(gen_start), 0), len(history))
    counts = np.bincount([t for t in history[gen_start:] if 0 <= t < V], minlength=V)
    pen = np.abs(float(np.float32(presence)) * (counts > 0) + float(np.float32(frequency)) * counts)
    b = np.zeros(V)
    for t, v in bias:
        if 0 <= t < V and np.isfinite(v):
            b[t] = abs(float(np.float32(v)))
    return 4.0 * 2.0 ** -24 * np.maximum(np.maximum(x, pen), b)


def tolerance(logit, presence=0.0, frequency_times_count=0.0, bias=0.0):
    """|got - ref64| of a penalised or biased logit: at most three fp32 roundings of values no larger than the largest operand"""
    return 4.0 * 2.0 ** -24 * max(abs(float(logit)), abs(float(presence) + float(frequency_times_count)), abs(float(bias)))
