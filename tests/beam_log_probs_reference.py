"""The gather tree of a beam request (k_gather_tree_beam, decoding_kernels.cu:452-583 + the transpose) restated in numpy with a
payload: besides the token of every output position, the value recorded in the cell that token was read from.

    gather_tree_with_payload(ids, parents, payload, seq_len, tiled_lengths, K, max_input_len, end_id)
        ids / parents / payload   time-major [total, B*K]
        -> output_ids [B, K, total] int32, sequence_lengths [B, K] int32,
           values [B, K, total - max_input_len] (payload's dtype), from_cell [B, K, total - max_input_len] bool

values[b, k, i] belongs to the i-th generated token, output_ids[b, k, input_lengths[b] + i].  It is the payload of the cell
the tree read that token from, and 0 (from_cell False) where the tree takes no token from a cell: positions no level maps to,
the end_id fill beyond the longest beam, and the rewrite behind the hypothesis' first end token.  The tree is restated as
written, quirks included: the rewrite scans row indices [max_input_len, msl), not generated positions.

step_differences(cum_before, cum_after, parents, K) forms what a beam step records: fp32 cum_after[bb] - cum_before[parent].
"""
import numpy as np


def gather_tree_with_payload(ids, parents, payload, seq_len, tiled_lengths, K, max_input_len, end_id):
    total, BK = ids.shape
    B = BK // K
    out_len = total - max_input_len
    out = np.zeros((B, K, total), np.int32)
    lens = np.zeros((B, K), np.int32)
    val = np.zeros((B, K, out_len), payload.dtype)
    src = np.zeros((B, K, out_len), bool)
    for b in range(B):
        max_len = max(int(seq_len[b * K + j]) + 1 for j in range(K))
        msl = min(max_len, total)
        for k in range(K):
            bb = b * K + k
            lens[b, k] = int(seq_len[bb]) + 1
            if msl <= 0:
                continue
            in_len = int(tiled_lengths[bb])
            pad_off = max_input_len - in_len
            beams = out[b, k]
            # the payload travels with the row index of `beams` it was written to: generated position i is row in_len + i
            row_val = np.zeros(total, payload.dtype)
            row_src = np.zeros(total, bool)

            def take(row, level, slot):
                beams[row] = ids[level, slot]
                if level >= max_input_len:
                    row_val[row] = payload[level, slot]
                    row_src[row] = True

            take(msl - 1 - pad_off, msl - 1, bb)
            parent = int(parents[msl - 1, bb]) % K
            for level in range(msl - 2, -1, -1):
                if in_len <= level < max_input_len:
                    continue
                take(level - pad_off if level >= max_input_len else level, level, b * K + parent)
                parent = int(parents[level, b * K + parent]) % K
            for index in range(max_len - pad_off, total):
                beams[index] = end_id
                row_val[index] = 0
                row_src[index] = False
            fin = False
            for t in range(max_input_len, msl):
                if fin:
                    beams[t] = end_id
                    row_val[t] = 0
                    row_src[t] = False
                elif beams[t] == end_id:
                    fin = True
            val[b, k] = row_val[in_len:in_len + out_len]
            src[b, k] = row_src[in_len:in_len + out_len]
    return out, lens, val, src


def step_differences(cum_before, cum_after, parents, K):
    """cum_before / cum_after [B*K] fp32 around one beam step, parents [B*K] (beam index within the batch entry) -> the step's
    recorded values [B*K] fp32: one IEEE subtraction each."""
    cum_before = np.asarray(cum_before, np.float32)
    cum_after = np.asarray(cum_after, np.float32)
    bb = np.arange(cum_after.size)
    return (cum_after - cum_before[(bb // K) * K + np.asarray(parents)]).astype(np.float32)
