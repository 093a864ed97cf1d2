"""Crafted inputs of ONE dynamic-decode step / ONE beam-search step: the tie, mask and size edges of kernels_sampling.hip
and kernels_beam.hip.

Shared by test_decode_step_reference.py (CPU: oracle against tests/decode_reference.py) and test_gpu_decode_step.py (GPU: the
kernels against both).  Every logit family keeps different values well apart (a grid of 2**-10 or coarser) or exactly equal,
so that the order of a row does not depend on how an implementation rounds its exponentials.

Seeds: a case's rows draw with random_seed = seed + 7919 * row.  `seed` is pinned in SEEDS: the first one from the case's base
(crc32 of its name) at which every sampling row's margin (decode_reference.MARGIN) clears; `python -m tests.decode_cases`
prints the table.  test_decode_step_reference.py checks that every pinned seed is that seed.
"""
import zlib

import numpy as np

from oracle import oracle as orc
from tests import decode_reference as ref

SENTINEL = -7          # cells of output_ids nothing may touch (and nothing reads)
GENERAL, TOPK_FUSED, GREEDY_FUSED = 0, 1, 2
FORM_NAMES = {GENERAL: "general", TOPK_FUSED: "topk_fused", GREEDY_FUSED: "greedy_fused"}
TKD_MAXK, TKD_MAXB = 64, 4
LP_TOL = dict(rtol=1e-4, atol=2e-4)     # log-probabilities (test_gpu_sampling_vocab.py)
SCORE_TOL = dict(rtol=1e-4, atol=1e-3)  # beam scores (test_gpu_sampling_vocab.py)


class Case:
    """Inputs of one sampling step.  logits [B, V] fp32; history: dict time -> [B] tokens (rows of output_ids below `step`)."""

    def __init__(self, name, logits, *, top_k=None, top_p=None, temperature=None, repetition_penalty=None, min_length=None,
                 step=None, max_input_len=4, total_len=16, input_lengths=None, end_id=0, history=None, finished=None,
                 stop_words=None, optional_last_tokens=None, return_cum_log_probs=True, output_log_probs=False, row_len=None,
                 finish=True, seq_len=None, cum_log_probs=None, draw_counter=None):
        self.name = name
        self.logits = np.ascontiguousarray(logits, dtype=np.float32)
        self.B, self.V = self.logits.shape
        B = self.B
        self.top_k, self.top_p, self.temperature = top_k, top_p, temperature
        self.repetition_penalty, self.min_length = repetition_penalty, min_length
        self.max_input_len, self.total_len, self.end_id = max_input_len, total_len, end_id
        self.step = max_input_len if step is None else step
        self.input_lengths = np.full(B, max_input_len, np.int32) if input_lengths is None else np.asarray(input_lengths, np.int32)
        self.row_len = None if row_len is None else np.asarray(row_len, np.int32)
        self.finish = finish
        rows = max(total_len, self.step + 1)
        self.output_ids = np.full((rows, B), SENTINEL, np.int32)
        rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
        for b in range(B):  # a valid token wherever the layer may read: the row's history without its padding positions
            upto = self.step if self.row_len is None else int(self.row_len[b]) + 1
            for t in range(upto):
                if not (self.input_lengths[b] <= t < max_input_len):
                    self.output_ids[t, b] = rng.integers(0, self.V)
        for t, toks in (history or {}).items():
            for b in range(B):
                upto = self.step if self.row_len is None else int(self.row_len[b]) + 1
                if t < upto and not (self.input_lengths[b] <= t < max_input_len):
                    self.output_ids[t, b] = toks[b]
        self.finished = np.zeros(B, np.uint8) if finished is None else np.asarray(finished, np.uint8)
        # the state a request has at `step`: one token per step so far
        base = self.step - 1 if self.row_len is None else self.row_len
        self.seq_len = (np.zeros(B, np.int32) + base).astype(np.int32) if seq_len is None else np.asarray(seq_len, np.int32)
        self.cum_log_probs = (-0.5 * np.arange(B)).astype(np.float32) if cum_log_probs is None else np.asarray(cum_log_probs, np.float32)
        self.draw_counter = (np.arange(B) % 3).astype(np.uint64) if draw_counter is None else np.asarray(draw_counter, np.uint64)
        self.stop_words = None if stop_words is None else np.ascontiguousarray(stop_words, np.int32)
        self.optional_last_tokens = None if optional_last_tokens is None else np.ascontiguousarray(optional_last_tokens, np.int32)
        self.return_cum_log_probs = return_cum_log_probs
        self.output_log_probs = output_log_probs
        self.seed_base = zlib.crc32(name.encode())

    def seeds(self, seed):
        return (np.uint64(seed) + np.uint64(7919) * np.arange(self.B, dtype=np.uint64)).astype(np.uint64)

    def reference(self, seed):
        return ref.sampling_step(
            self.logits, self.step, self.max_input_len, self.input_lengths, self.end_id, self.output_ids, self.finished,
            self.seq_len, self.cum_log_probs, self.draw_counter, total_len=self.total_len, top_k=self.top_k, top_p=self.top_p,
            temperature=self.temperature, repetition_penalty=self.repetition_penalty, min_length=self.min_length,
            random_seed=self.seeds(seed), stop_words=self.stop_words, optional_last_tokens=self.optional_last_tokens,
            return_cum_log_probs=self.return_cum_log_probs or self.output_log_probs, row_len=self.row_len, finish=self.finish)

    def find_seed(self, limit=4096):
        for seed in range(self.seed_base, self.seed_base + limit):
            if float(np.min(self.reference(seed)["margin"])) > ref.MARGIN:
                return seed
        raise AssertionError(f"{self.name}: no seed clears the margin")

    def forms(self):
        """the forms launch_dynamic_decode may take for this case (kernels_sampling.hip: dynamic_decode_is_*_fused), the general
        one first"""
        k_eff, _, _ = ref.route(self.top_k, self.top_p, self.B)
        temp = np.asarray(1.0 if self.temperature is None else self.temperature, np.float32).reshape(-1)
        rep = np.asarray(1.0 if self.repetition_penalty is None else self.repetition_penalty, np.float32).reshape(-1)
        plain = (self.finish and not np.any(k_eff == 0) and np.all(temp == 1.0) and (self.repetition_penalty is None or np.all(rep == 1.0))
                 and self.optional_last_tokens is None and self.row_len is None and self.V <= 32 * 256 * 16)
        out = [GENERAL]
        kmax = max(1, int(k_eff.max()))
        if plain and 2 <= kmax <= TKD_MAXK and self.B <= TKD_MAXB:
            out.append(TOPK_FUSED)
        if plain and kmax == 1 and self.B <= 1024:
            out.append(GREEDY_FUSED)
        return out


# ---- logit families ----
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def qgauss(name, B, V, q=0.25):
    """randn * 2 rounded to multiples of q: about 30 different values, ties at every rank"""
    return (np.round(_rng(name).standard_normal((B, V)) * 2.0 / q) * q).astype(np.float32)


def smooth(name, B, V):
    """randn * 2 on a grid of 2**-10: (almost) no ties, different values well apart"""
    return (np.round(_rng(name).standard_normal((B, V)) * 2.0 * 1024.0) / 1024.0).astype(np.float32)


def flat(name, B, V, levels=5, span=1e-3):
    """a nearly uniform row: `levels` values within `span` of each other, thousands of ties per value"""
    lv = (np.arange(levels) * (span / (levels - 1))).astype(np.float32)
    return lv[_rng(name).integers(0, levels, (B, V))].astype(np.float32)


def minus_inf_rows(B, V, finite_ids, values):
    l = np.full((B, V), -np.inf, np.float32)
    for i, v in zip(finite_ids, values):
        l[:, i] = v
    return l


def _plateau_row(name, V, ids, value, above=0):
    """a smooth row below `value`, `above` entries over it, and a plateau of equal entries at `ids`"""
    l = np.minimum(smooth(name, 1, V)[0], 4.0) - 6.0
    free = [i for i in range(V) if i not in set(ids)]
    for j, i in enumerate(_rng(name + "a").permutation(free)[:above]):
        l[i] = value + (j + 1) / 64.0  # (little above it: the plateau keeps a good share of the mass)
    l[list(ids)] = value
    return l.astype(np.float32)


def _tile(row, B):
    return np.tile(np.asarray(row, np.float32)[None, :], (B, 1))


def _stop(B, stop_len, rows):
    """stop_words [B, 2, stop_len] from {row: [word, ...]}"""
    sw = np.zeros((B, 2, stop_len), np.int32)
    sw[:, 1, :] = -1
    for b, words in rows.items():
        flat_, offs = [], []
        for w in words:
            flat_ += list(w)
            offs.append(len(flat_))
        sw[b, 0, :len(flat_)] = flat_
        sw[b, 1, :len(offs)] = offs
    return sw


def sampling_cases():
    cases = []
    add = cases.append
    KS, PS = (1, 2, 50, 64, 65, 1024), (0.3, 0.9, 1.0)
    # ---- quantised Gaussians: every k and every p at every slice geometry ----
    for V in (5, 7, 100, 1000, 2051, 4099):
        for k in KS:
            add(Case(f"qgauss_V{V}_k{k}", qgauss(f"qg{V}", 3, V), top_k=k, end_id=1))
        for p in PS:
            add(Case(f"qgauss_V{V}_p{p}", qgauss(f"qg{V}", 3, V), top_k=0, top_p=p, end_id=1))
    for k in (2, 50, 1024):  # without the row's soft-max (the k masses are exp(l - best))
        add(Case(f"qgauss_nocum_V4099_k{k}", qgauss("qg4099", 3, 4099), top_k=k, return_cum_log_probs=False))
    add(Case("qgauss_V4099_k50_p0.7", qgauss("qg4099", 3, 4099), top_k=50, top_p=0.7))  # the top-k layer's own p
    add(Case("smooth_V4099_k50", smooth("sm", 4, 4099), top_k=50))
    add(Case("smooth_V4099_p0.9", smooth("sm", 4, 4099), top_k=0, top_p=0.9))
    # ---- a plateau across the k-th place: inside one slice, across two slices (general slices of 513, fused ones of 129), and
    # at the top of the order, where every pick shows a member of the set ----
    add(Case("plateau_one_slice_k50", _tile(_plateau_row("p1", 4099, range(1100, 1125), 5.0, above=30), 4), top_k=50))
    add(Case("plateau_two_slices_k50", _tile(_plateau_row("p2", 4099, range(500, 540), 5.0, above=30), 4), top_k=50))
    add(Case("plateau_top_two_slices_k50", _tile(_plateau_row("p3", 4099, range(480, 545), 5.0), 4), top_k=50))
    add(Case("plateau_top_spread_k64", _tile(_plateau_row("p4", 4099, range(7, 4099, 41), 5.0), 4), top_k=64))
    add(Case("plateau_top_spread_k65", _tile(_plateau_row("p4", 4099, range(7, 4099, 41), 5.0), 4), top_k=65))
    # ---- all-equal rows: every slice takes the tie branch, the set is the lowest ids ----
    for k in (2, 50, 64, 65, 1024):
        add(Case(f"all_equal_V4099_k{k}", np.full((2, 4099), 1.5, np.float32), top_k=k, end_id=4000))
    add(Case("all_equal_V4099_k1", np.full((2, 4099), 1.5, np.float32), top_k=1, end_id=4000))
    add(Case("all_equal_min_length_k50", np.full((4, 4099), 1.5, np.float32), top_k=50, end_id=3, min_length=8))
    add(Case("all_equal_min_length_k1", np.full((2, 4099), 1.5, np.float32), top_k=1, end_id=0, min_length=8))
    add(Case("all_equal_V100864_k50", np.full((1, 100864), -2.25, np.float32), top_k=50, end_id=2))
    add(Case("all_equal_V1000_p0.9", np.full((2, 1000), 0.5, np.float32), top_k=0, top_p=0.9, end_id=999))
    # ---- signed zeros: -0.0 == +0.0, the index decides ----
    for V, ids in ((100, (40, 45, 50)), (4099, (40, 600, 1200))):
        for tag, zs in (("mm_p", (-0.0, -0.0, 0.0)), ("p_m_p", (0.0, -0.0, 0.0)), ("m_p_m", (-0.0, 0.0, -0.0))):
            row = -1.0 - np.abs(smooth(f"z{V}", 1, V)[0])
            row[list(ids)] = zs
            add(Case(f"signed_zero_{tag}_V{V}_k2", _tile(row, 4), top_k=2, end_id=1))
        row = -1.0 - np.abs(smooth(f"z{V}", 1, V)[0])
        row[list(ids)] = (-0.0, 0.0, 0.0)
        add(Case(f"signed_zero_V{V}_k1", _tile(row, 2), top_k=1, end_id=1))
        add(Case(f"signed_zero_V{V}_p1.0", _tile(row, 4), top_k=0, top_p=1.0, end_id=1))
    # ---- rows with fewer finite logits than k: made directly and by the optional-token list of the first step; ids on both
    # sides of a slice boundary (512 | 513 general, 128 | 129 fused) ----
    for M, ids, vals in ((1, (513,), (0.25,)), (3, (512, 513, 129), (0.25, 0.5, 0.25))):
        for k in (1, 50, 1024):
            add(Case(f"minus_inf_M{M}_k{k}", minus_inf_rows(3, 4099, ids, vals), top_k=k, end_id=7))
        add(Case(f"minus_inf_M{M}_p0.9", minus_inf_rows(3, 4099, ids, vals), top_k=0, top_p=0.9, end_id=7))
        opt = np.full((3, 5), -1, np.int32)
        opt[:, :len(ids)] = ids
        for k in (50, 1024):
            add(Case(f"optional_M{M}_k{k}_first_step", smooth("opt", 3, 4099), top_k=k, end_id=7, optional_last_tokens=opt))
        add(Case(f"optional_M{M}_p1.0_first_step", smooth("opt", 3, 4099), top_k=0, top_p=1.0, end_id=7, optional_last_tokens=opt))
        add(Case(f"optional_M{M}_k50_second_step", smooth("opt", 3, 4099), top_k=50, end_id=7, optional_last_tokens=opt, step=5))
    # ---- one-hot: the row's probability is 1 / (1 + 1e-6) ----
    hot = smooth("hot", 2, 1000)
    hot[:, 700] = hot.max() + 80.0
    add(Case("one_hot_k50", hot, top_k=50, end_id=1))
    add(Case("one_hot_k1", hot, top_k=1, end_id=1))
    add(Case("one_hot_p0.9", hot, top_k=0, top_p=0.9, end_id=1))
    # ---- flat rows for the top-p layer: the walk leaves the candidates (128 per slice) and sorts the whole row ----
    for V in (2051, 4099):
        for p in (0.9, 1.0):
            add(Case(f"flat_V{V}_p{p}", flat(f"fl{V}", 3, V), top_k=0, top_p=p, end_id=1))
    add(Case("flat_V1000_p1.0", flat("fl1000", 3, 1000), top_k=0, top_p=1.0, end_id=1))  # every slice below 128: no cut at all
    add(Case("flat_V100864_p1.0", flat("flbig", 1, 100864), top_k=0, top_p=1.0, end_id=1))
    add(Case("flat_two_levels_V4099_p1.0", flat("fl2", 3, 4099, levels=2), top_k=0, top_p=1.0, end_id=1))
    # ---- penalties ----
    for t in (0.05, 3.0):
        add(Case(f"temperature_{t}_k50", smooth("tmp", 3, 1000), top_k=50, temperature=t, end_id=1))
        add(Case(f"temperature_{t}_p0.9", qgauss("tmpq", 3, 1000), top_k=0, top_p=0.9, temperature=t, end_id=1))
    add(Case("temperature_per_row_k50", smooth("tmp", 3, 1000), top_k=50, temperature=[1.0, 0.7, 1.0], end_id=1))
    rl = smooth("rep", 3, 1000)
    rl[:, 11] = 0.0   # a history token whose logit is exactly 0
    rl[:, 12] = -1.5  # negative ones
    rl[:, 13] = -0.25
    rl[:, 14] = 6.0   # and the best of the row, met three times
    hist = {t: [tok, tok, tok] for t, tok in enumerate((14, 11, 12, 14, 13, 977, 14, 12, 11))}
    for pen in (1.3, 0.8):
        kw = dict(repetition_penalty=pen, max_input_len=6, step=9, input_lengths=[6, 4, 2], history=hist, end_id=1)
        add(Case(f"repetition_{pen}_k50", rl, top_k=50, **kw))
        add(Case(f"repetition_{pen}_p0.9", rl, top_k=0, top_p=0.9, **kw))
    add(Case("repetition_per_row_k50", rl, top_k=50, repetition_penalty=[1.0, 1.3, 0.8], max_input_len=6, step=9,
             input_lengths=[6, 4, 2], history=hist, end_id=1))
    add(Case("repetition_temperature_min_length_k50", rl, top_k=50, repetition_penalty=1.3, temperature=0.7, min_length=9,
             max_input_len=6, step=9, input_lengths=[6, 4, 2], history=hist, end_id=14))
    add(Case("repetition_total_len_7680", smooth("rep2", 2, 1000), top_k=2, repetition_penalty=1.3, max_input_len=6, step=9,
             total_len=7680, end_id=1))
    # ---- batches: 1, 4 | 5 around the fused top-k form's row limit, 16 rows of every kind ----
    for B in (1, 4, 5):
        add(Case(f"batch_{B}_k50", qgauss("bt", B, 4099), top_k=50, end_id=1))
        add(Case(f"batch_{B}_k1", qgauss("bt", B, 4099), top_k=1, end_id=1))
    fin5 = [0, 1, 0, 1, 0]
    add(Case("finished_among_live_k50", qgauss("bt", 5, 4099), top_k=50, end_id=1, finished=fin5, step=6))
    add(Case("finished_among_live_k2_B4", qgauss("bt", 4, 4099), top_k=2, end_id=1, finished=fin5[:4], step=6))
    add(Case("finished_among_live_k1", qgauss("bt", 5, 4099), top_k=1, end_id=1, finished=fin5, step=6))
    add(Case("finished_among_live_p0.9", qgauss("bt", 5, 4099), top_k=0, top_p=0.9, end_id=1, finished=fin5, step=6))
    mixed = qgauss("mix", 16, 4099)
    mixed[2] = 1.5
    mixed[3] = minus_inf_rows(1, 4099, (512, 513, 129), (0.25, 0.5, 0.25))[0]
    mixed[4] = flat("mixf", 1, 4099)[0]
    mixed[5, [40, 600, 1200]] = 9.0
    mixed[6] = -1.0 - np.abs(smooth("mixz", 1, 4099)[0])
    mixed[6, [40, 600, 1200]] = (-0.0, -0.0, 0.0)
    mixed[7, 700] = 90.0
    mixed[12] = flat("mixg", 1, 4099, levels=3)[0]
    add(Case("batch_16_mixed", mixed, end_id=1, step=6,
             top_k=[1, 2, 50, 50, 0, 2, 2, 64, 65, 1024, 0, 0, 0, 50, 0, 1],
             top_p=[0.0, 0.0, 0.0, 0.5, 1.0, 0.0, 0.9, 0.0, 0.0, 0.0, 0.3, 0.9, 1.0, 0.0, 0.9, 0.0],
             finished=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1], min_length=[0] * 8 + [9] * 8))
    # ---- the batcher's step: every row at its own step, no bookkeeping ----
    add(Case("row_len_no_finish", rl, top_k=[50, 0, 1], top_p=[0.0, 0.9, 0.0], repetition_penalty=1.3, max_input_len=2,
             input_lengths=[2, 1, 2], row_len=[8, 5, 3], history={t: [tok, tok, tok] for t, tok in enumerate((14, 11, 12, 14, 13, 977, 14, 12, 11))},
             finish=False, step=0, total_len=16, end_id=1, output_log_probs=True))
    # ---- the finish step ----
    g = smooth("fin", 3, 1000)
    g[0, 17] = g[1, 31] = g[2, 5] = 30.0
    sw = _stop(3, 4, {0: [[17]], 1: [[99, 98], [23, 31]], 2: [[23, 31]]})
    add(Case("stop_words_k1", g, top_k=1, end_id=1, step=6, history={5: [23, 23, 23]}, stop_words=sw))
    add(Case("stop_words_k2", g, top_k=2, top_p=0.5, end_id=1, step=6, history={5: [23, 23, 23]}, stop_words=sw))
    sw_all = _stop(3, 4, {0: [[17]], 1: [[99, 98], [23, 31]], 2: [[5]]})
    add(Case("stop_words_all_finished_k1", g, top_k=1, end_id=1, step=6, history={5: [23, 23, 23]}, stop_words=sw_all))
    add(Case("end_id_all_finished_k1", g, top_k=1, end_id=17, step=6, finished=[0, 1, 1]))
    add(Case("length_criterion_k1", g, top_k=1, end_id=1, step=16, total_len=16))
    add(Case("length_criterion_p0.9", g, top_k=0, top_p=0.9, end_id=1, step=16, total_len=16))
    add(Case("first_step_padding_k50", smooth("fin", 3, 1000), top_k=50, end_id=1, max_input_len=6, input_lengths=[6, 4, 1]))
    add(Case("output_log_probs_k50", smooth("fin", 3, 1000), top_k=50, end_id=1, step=7, output_log_probs=True, return_cum_log_probs=False))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


class BeamCase:
    """Inputs of one beam-search step; rows bb = batch * K + beam.  logits [B * K, V] fp32."""

    def __init__(self, name, logits, K, *, step=None, max_input_len=4, total_len=12, input_lengths=None, end_id=0, cum_log_probs=None,
                 finished=None, history=None, parents=None, temperature=None, repetition_penalty=None, diversity_rate=None,
                 len_penalty=None, min_length=None, stop_words=None, optional_last_tokens=None, seq_len=None):
        self.name, self.K = name, K
        self.logits = np.ascontiguousarray(logits, dtype=np.float32)
        BK, self.V = self.logits.shape
        self.B = BK // K
        self.max_input_len, self.total_len, self.end_id = max_input_len, total_len, end_id
        self.s_max = total_len
        self.step = max_input_len if step is None else step
        self.input_lengths = np.full(BK, max_input_len, np.int32) if input_lengths is None else np.repeat(np.asarray(input_lengths, np.int32), K)
        rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
        self.output_ids = np.full((total_len, BK), SENTINEL, np.int32)
        self.parent_ids = np.full((total_len, BK), SENTINEL, np.int32)
        for bb in range(BK):
            for t in range(self.step):
                pad = self.input_lengths[bb] <= t < max_input_len
                self.output_ids[t, bb] = SENTINEL if pad else rng.integers(0, self.V)
                self.parent_ids[t, bb] = 0 if t < max_input_len else rng.integers(0, K)  # (the prompt's parents are zero)
        for t, toks in (history or {}).items():
            self.output_ids[t] = toks
        for t, par in (parents or {}).items():
            self.parent_ids[t] = par
        if cum_log_probs is None:  # the first step: beams above 0 start behind
            cum_log_probs = np.where(np.arange(BK) % K == 0, 0.0, -1e20)
        self.cum_log_probs = np.asarray(cum_log_probs, np.float32)
        self.finished = np.zeros(BK, np.uint8) if finished is None else np.asarray(finished, np.uint8)
        self.seq_len = np.full(BK, self.step - 1, np.int32) if seq_len is None else np.asarray(seq_len, np.int32)
        # both planes of the cache indirection: the one the step reads holds beams, the other one a sentinel
        self.cache_indir = np.full((2, BK, self.s_max), SENTINEL, np.int32)
        self.src_plane = (self.step - max_input_len) % 2
        self.cache_indir[self.src_plane, :, :self.step] = rng.integers(0, K, (BK, self.step))
        self.temperature, self.repetition_penalty, self.diversity_rate = temperature, repetition_penalty, diversity_rate
        self.len_penalty, self.min_length = len_penalty, min_length
        self.stop_words = None if stop_words is None else np.ascontiguousarray(stop_words, np.int32)
        self.optional_last_tokens = None if optional_last_tokens is None else np.ascontiguousarray(optional_last_tokens, np.int32)

    def indir(self):
        B, K = self.B, self.K
        return (self.cache_indir[self.src_plane].reshape(B, K, -1).copy(), self.cache_indir[1 - self.src_plane].reshape(B, K, -1).copy())

    def reference(self):
        src, tgt = self.indir()
        return ref.beam_step(self.logits, self.K, self.step, self.max_input_len, self.input_lengths, self.end_id, self.output_ids,
                             self.parent_ids, self.finished, self.seq_len, self.cum_log_probs, src, tgt, temperature=self.temperature,
                             repetition_penalty=self.repetition_penalty, diversity_rate=self.diversity_rate, len_penalty=self.len_penalty,
                             min_length=self.min_length, stop_words=self.stop_words, optional_last_tokens=self.optional_last_tokens)


def beam_cases():
    cases = []
    add = cases.append
    # ---- the first step: every beam of a batch entry sees the same row, beams above 0 start at -1e20 ----
    for K, V, B in ((2, 4099, 2), (4, 4099, 2), (64, 70, 1), (64, 4099, 1)):
        row = qgauss(f"beam{V}", B, V)
        add(BeamCase(f"beam_first_step_K{K}_V{V}", np.repeat(row, K, axis=0), K, end_id=1))
    # ---- a later step, quantised logits, pairs of beams with the same row and the same score: the lower candidate index wins ----
    for K, V in ((2, 4099), (4, 4099), (64, 70), (64, 4099)):
        rows = np.repeat(qgauss(f"beamq{K}_{V}", K // 2, V), 2, axis=0)
        cum = np.repeat(-1.0 - 0.375 * np.arange(K // 2), 2)
        add(BeamCase(f"beam_equal_scores_K{K}_V{V}", rows, K, step=6, cum_log_probs=cum, end_id=1))
    add(BeamCase("beam_later_step_smooth_K4", smooth("beams", 8, 4099), 4, step=7, cum_log_probs=-0.25 * np.arange(8) - 1.0, end_id=1))
    # ---- one finished beam among live ones (it offers end_id at its own score), a row with fewer than K finite logits ----
    add(BeamCase("beam_finished_among_live_K4", qgauss("beamf", 8, 4099), 4, step=6, end_id=5, finished=[0, 1, 0, 0, 1, 0, 0, 1],
                 cum_log_probs=[-1.0, -3.0, -2.0, -2.5, -0.5, -9.0, -9.5, -30.0], seq_len=[5, 4, 5, 5, 3, 5, 5, 4]))
    few = qgauss("beamm", 4, 4099)
    few[1] = minus_inf_rows(1, 4099, (512, 513), (0.5, 0.25))[0]
    add(BeamCase("beam_few_finite_K4", few, 4, step=6, cum_log_probs=[-2.0, -0.5, -2.25, -3.0], end_id=1))
    few0 = np.repeat(minus_inf_rows(1, 4099, (512, 513), (0.5, 0.25)), 4, axis=0)
    add(BeamCase("beam_few_finite_first_step_K4", few0, 4, end_id=1))  # beam 0 runs out: the -1e20 beams follow, lowest index first
    few64 = qgauss("beamm64", 64, 70)
    few64[3, 10:] = -np.inf
    add(BeamCase("beam_few_finite_K64_V70", few64, 64, step=6, cum_log_probs=-1.0 - (np.arange(64) % 7) * 0.4375, end_id=1))
    # ---- penalties ----
    add(BeamCase("beam_len_penalty_diversity_K4", qgauss("beaml", 8, 4099), 4, step=7, cum_log_probs=-1.0 - 0.3125 * np.arange(8),
                 len_penalty=[0.7, 1.5], diversity_rate=[-0.3, -0.05], end_id=1, seq_len=[6, 5, 6, 6, 4, 6, 6, 6], finished=[0, 1, 0, 0, 0, 0, 0, 0]))
    bl = smooth("beamr", 8, 1000)
    bl[:, 11], bl[:, 12], bl[:, 14] = 0.0, -1.5, 7.0
    hist = {t: [tok] * 8 for t, tok in enumerate((14, 11, 12, 14, 13, 977, 14))}
    hist[6] = [14, 11, 12, 13, 14, 11, 12, 13]
    add(BeamCase("beam_repetition_temperature_min_length_K4", bl, 4, step=7, max_input_len=5, input_lengths=[5, 3], history=hist,
                 cum_log_probs=-1.0 - 0.3125 * np.arange(8), repetition_penalty=[1.3, 0.8], temperature=[0.7, 1.0], min_length=[4, 0],
                 end_id=14))
    opt = np.full((2, 6), -1, np.int32)
    opt[0, :3] = (512, 513, 129)
    opt[1, :5] = (7, 8, 9, 3000, 4098)
    add(BeamCase("beam_optional_first_step_K4", np.repeat(smooth("beamo", 2, 4099), 4, axis=0), 4, end_id=1, optional_last_tokens=opt))
    # ---- the stop word is followed along the parent chain: the new beam 0 descends from beam 1 ----
    g = smooth("beamsw", 4, 1000)
    g[0, 31] = g[1, 55] = g[2, 31] = g[3, 55] = 40.0
    sw = _stop(2, 4, {0: [[23, 55]], 1: [[99, 98], [24, 31]]})
    add(BeamCase("beam_stop_words_parent_chain_K2", g, 2, step=6, cum_log_probs=[-2.0, -1.0, -2.0, -1.0], end_id=1,
                 history={5: [99, 23, 24, 99]}, stop_words=sw))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


def oracle_step(case, seed):
    """orc.dynamic_decode on copies of the case's state (one call per row when every row has its own step)"""
    B = case.B
    ids, fin, slen = case.output_ids.copy(), case.finished.copy(), case.seq_len.copy()
    cum, draws = case.cum_log_probs.copy(), case.draw_counter.copy()
    want_lp = case.return_cum_log_probs or case.output_log_probs

    def arg(v, b):
        if v is None or np.ndim(v) == 0:
            return v
        return np.asarray(v).reshape(-1)[b:b + 1] if b is not None and np.size(v) > 1 else v

    def run(rows, step):
        b = rows.start if rows.stop - rows.start == 1 and B > 1 else None
        sel = (lambda v: v) if b is None else (lambda v: None if v is None else np.ascontiguousarray(v[rows]))
        n = rows.stop - rows.start
        samp = orc.Sampling(n, top_k=0 if case.top_k is None else arg(case.top_k, b), top_p=0.0 if case.top_p is None else arg(case.top_p, b),
                            temperature=1.0 if case.temperature is None else arg(case.temperature, b),
                            repetition_penalty=None if case.repetition_penalty is None else arg(case.repetition_penalty, b),
                            random_seed=case.seeds(seed)[rows], min_length=None if case.min_length is None else arg(case.min_length, b),
                            stop_words=sel(case.stop_words), optional_last_tokens=sel(case.optional_last_tokens),
                            return_cum_log_probs=1 if want_lp else 0)
        o_ids = np.ascontiguousarray(ids[:, rows])
        o_fin, o_len = np.ascontiguousarray(fin[rows]), np.ascontiguousarray(slen[rows])
        o_cum, o_draws = np.ascontiguousarray(cum[rows]), np.ascontiguousarray(draws[rows])
        orc.dynamic_decode(np.ascontiguousarray(case.logits[rows]).copy(), step, case.max_input_len, case.input_lengths[rows], samp,
                           case.end_id, o_ids, o_fin, o_len, o_cum, o_draws)
        ids[:, rows], fin[rows], slen[rows], cum[rows], draws[rows] = o_ids, o_fin, o_len, o_cum, o_draws

    if case.row_len is None:
        run(slice(0, B), case.step)
    else:
        # (a batch-wide penalty switch is the batch's: the case's rows all carry the same switches)
        for b in range(B):
            run(slice(b, b + 1), int(case.row_len[b]) + 1)
    if case.finish and case.step >= case.total_len:  # the length criterion is the finish step's, not orc.dynamic_decode's
        fin[:] = 1
    return dict(output_ids=ids, finished=fin, seq_len=slen, cum_log_probs=cum, draw_counter=draws)


def oracle_beam_step(case):
    ids, par = case.output_ids.copy(), case.parent_ids.copy()
    fin, slen, cum = case.finished.copy(), case.seq_len.copy(), case.cum_log_probs.copy()
    src, tgt = case.indir()
    bp = orc.BeamParams(case.B, temperature=case.temperature, repetition_penalty=case.repetition_penalty,
                        diversity_rate=case.diversity_rate, len_penalty=case.len_penalty, min_length=case.min_length,
                        stop_words=case.stop_words, optional_last_tokens=case.optional_last_tokens)
    orc.beam_search_step(case.logits.copy(), case.K, case.step, case.max_input_len, case.input_lengths, bp, case.end_id, ids, par, fin,
                         slen, cum, np.ascontiguousarray(src, np.int32), tgt)
    return dict(output_ids=ids, parent_ids=par, finished=fin, seq_len=slen, cum_log_probs=cum, tgt_indir=tgt)


# the first seed from each case's base that clears the margin (python -m tests.decode_cases)
SEEDS = {
    "qgauss_V5_k1": 4224872031,
    "qgauss_V5_k2": 1658535909,
    "qgauss_V5_k50": 1805157422,
    "qgauss_V5_k64": 1205343220,
    "qgauss_V5_k65": 819929954,
    "qgauss_V5_k1024": 3819765985,
    "qgauss_V5_p0.3": 3841799802,
    "qgauss_V5_p0.9": 69787492,
    "qgauss_V5_p1.0": 2083917303,
    "qgauss_V7_k1": 1373349588,
    "qgauss_V7_k2": 3369269102,
    "qgauss_V7_k50": 291034958,
    "qgauss_V7_k64": 1024999572,
    "qgauss_V7_k65": 1243574274,
    "qgauss_V7_k1024": 1949438408,
    "qgauss_V7_p0.3": 2838861681,
    "qgauss_V7_p0.9": 1239449199,
    "qgauss_V7_p1.0": 838774012,
    "qgauss_V100_k1": 3750861500,
    "qgauss_V100_k2": 1184418566,
    "qgauss_V100_k50": 1388278808,
    "qgauss_V100_k64": 2130699202,
    "qgauss_V100_k65": 167301972,
    "qgauss_V100_k1024": 3607911087,
    "qgauss_V100_p0.3": 729711635,
    "qgauss_V100_p0.9": 3417009421,
    "qgauss_V100_p1.0": 3015032734,
    "qgauss_V1000_k1": 1101504077,
    "qgauss_V1000_k2": 3635335159,
    "qgauss_V1000_k50": 2560327830,
    "qgauss_V1000_k64": 3034257228,
    "qgauss_V1000_k65": 3285985242,
    "qgauss_V1000_k1024": 3369866059,
    "qgauss_V1000_p0.3": 565448384,
    "qgauss_V1000_p0.9": 3244419038,
    "qgauss_V1000_p1.0": 3112121677,
    "qgauss_V2051_k1": 1273029,
    "qgauss_V2051_k2": 2568633727,
    "qgauss_V2051_k50": 2075737974,
    "qgauss_V2051_k64": 1475979436,
    "qgauss_V2051_k65": 553556026,
    "qgauss_V2051_k1024": 3447500185,
    "qgauss_V2051_p0.3": 2170408455,
    "qgauss_V2051_p0.9": 1636312857,
    "qgauss_V2051_p1.0": 429323658,
    "qgauss_V4099_k1": 1669831697,
    "qgauss_V4099_k2": 4203662763,
    "qgauss_V4099_k50": 4200906059,
    "qgauss_V4099_k64": 3592694417,
    "qgauss_V4099_k65": 2703432199,
    "qgauss_V4099_k1024": 2753726199,
    "qgauss_V4099_p0.3": 3652476820,
    "qgauss_V4099_p0.9": 962705034,
    "qgauss_V4099_p1.0": 1098867737,
    "qgauss_nocum_V4099_k2": 1183006682,
    "qgauss_nocum_V4099_k50": 3722113299,
    "qgauss_nocum_V4099_k1024": 2838133678,
    "qgauss_V4099_k50_p0.7": 3778663420,
    "smooth_V4099_k50": 2789726786,
    "smooth_V4099_p0.9": 1088499017,
    "plateau_one_slice_k50": 3808284604,
    "plateau_two_slices_k50": 2800534679,
    "plateau_top_two_slices_k50": 1368672694,
    "plateau_top_spread_k64": 1535177937,
    "plateau_top_spread_k65": 747095111,
    "all_equal_V4099_k2": 715259219,
    "all_equal_V4099_k50": 1238558805,
    "all_equal_V4099_k64": 1704099727,
    "all_equal_V4099_k65": 311775001,
    "all_equal_V4099_k1024": 1801629669,
    "all_equal_V4099_k1": 3014175977,
    "all_equal_min_length_k50": 1002994239,
    "all_equal_min_length_k1": 2925347631,
    "all_equal_V100864_k50": 1391943945,
    "all_equal_V1000_p0.9": 1004367080,
    "signed_zero_mm_p_V100_k2": 309790924,
    "signed_zero_p_m_p_V100_k2": 2707962034,
    "signed_zero_m_p_m_V100_k2": 1789842172,
    "signed_zero_V100_k1": 3797830934,
    "signed_zero_V100_p1.0": 4293562693,
    "signed_zero_mm_p_V4099_k2": 2171275718,
    "signed_zero_p_m_p_V4099_k2": 912607949,
    "signed_zero_m_p_m_V4099_k2": 2815090864,
    "signed_zero_V4099_k1": 1438193968,
    "signed_zero_V4099_p1.0": 1345466475,
    "minus_inf_M1_k1": 1419186992,
    "minus_inf_M1_k50": 3057302938,
    "minus_inf_M1_k1024": 1006714615,
    "minus_inf_M1_p0.9": 3371764424,
    "optional_M1_k50_first_step": 1589737744,
    "optional_M1_k1024_first_step": 3116883590,
    "optional_M1_p1.0_first_step": 1402686631,
    "optional_M1_k50_second_step": 3564655868,
    "minus_inf_M3_k1": 4271823803,
    "minus_inf_M3_k50": 3438997242,
    "minus_inf_M3_k1024": 2879270878,
    "minus_inf_M3_p0.9": 2234624963,
    "optional_M3_k50_first_step": 3647036531,
    "optional_M3_k1024_first_step": 3155408133,
    "optional_M3_p1.0_first_step": 2275925088,
    "optional_M3_k50_second_step": 4506683,
    "one_hot_k50": 3822776957,
    "one_hot_k1": 2986269575,
    "one_hot_p0.9": 4139949404,
    "flat_V2051_p0.9": 2872611753,
    "flat_V2051_p1.0": 3542499642,
    "flat_V4099_p0.9": 4090561082,
    "flat_V4099_p1.0": 2345652393,
    "flat_V1000_p1.0": 1942979069,
    "flat_V100864_p1.0": 45806982,
    "flat_two_levels_V4099_p1.0": 2567751784,
    "temperature_0.05_k50": 2298938062,
    "temperature_0.05_p0.9": 2764087962,
    "temperature_3.0_k50": 3372259948,
    "temperature_3.0_p0.9": 2623039430,
    "temperature_per_row_k50": 2107164503,
    "repetition_1.3_k50": 1245649107,
    "repetition_1.3_p0.9": 3339056729,
    "repetition_0.8_k50": 2610438774,
    "repetition_0.8_p0.9": 1634207237,
    "repetition_per_row_k50": 2545298391,
    "repetition_temperature_min_length_k50": 2452006715,
    "repetition_total_len_7680": 2693482588,
    "batch_1_k50": 620045411,
    "batch_1_k1": 1233154556,
    "batch_4_k50": 3960843027,
    "batch_4_k1": 2120122830,
    "batch_5_k50": 3514139299,
    "batch_5_k1": 3336758955,
    "finished_among_live_k50": 1358413142,
    "finished_among_live_k2_B4": 625941117,
    "finished_among_live_k1": 4207664767,
    "finished_among_live_p0.9": 1523403091,
    "batch_16_mixed": 3204169886,
    "row_len_no_finish": 2516045035,
    "stop_words_k1": 2399570153,
    "stop_words_k2": 370137427,
    "stop_words_all_finished_k1": 809551022,
    "end_id_all_finished_k1": 291927732,
    "length_criterion_k1": 2093981420,
    "length_criterion_p0.9": 1987925790,
    "first_step_padding_k50": 2530056255,
    "output_log_probs_k50": 3504557660,
}


if __name__ == "__main__":
    for c in sampling_cases():
        print(f'    "{c.name}": {c.find_seed()},')
