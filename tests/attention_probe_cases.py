"""Single-key probes of the decode attention: cases and helpers shared by test_attention_probe_reference.py (CPU: the oracle has
the property) and test_gpu_attention_probes.py (GPU: every decode path has it too).

The property.  In a model with ONE attention layer a prompt token j reaches a decode step's logits only through cached key / value j
of its own row.  So, against a base request, a request with one prompt token replaced must
  * `live`      (position < the row's length; observed on that row): change the logits of every decode step -- not bit-identical --
                and by the amount the oracle changes them (|d_gpu - d_oracle| <= LOGIT_FRAC * range);
  * `pad`       (length <= position < S; observed on every row) and
  * `other_row` (a live position of one row; observed on all the OTHER rows): change nothing, bit for bit.
A kernel that skips the last key of a chunk, reads a clamped row twice, lets a padding key in or reads a neighbour's cache block
breaks one of these, where the end-to-end bound LOGIT_FRAC alone is too coarse to see one key (median single-key change 8e-3 of
the logit range at 300 keys, smallest 2e-3).

Models (random_model(..., std=0.04)): `one` has num_layer 1; `iso0` / `iso1` have two layers of which only layer 0 / 1 is live -- the
other one has out_w = ffn2_w = ffn2_b = 0 and is, with the parallel residual, the identity on the residual stream (x + 0 + 0): the
per-layer cache offset.  The iso family stays fp16 (an all-zero weight column has int8 scale 0).

Step 0 of a request comes from the prompt phase; the comparisons are over the decode steps (index >= 1), and a step counts only
while every token generated before it is the same in both runs (and none is end_id).  Steps behind a flipped token are lost; the
tests cap the loss (MAX_LOST), and the seeds below are chosen so that the oracle stays under the cap:
`python -m tests.attention_probe_cases` prints every case's figures.

No GPU import here.
"""
import zlib

import numpy as np

from oracle import oracle as orc
from tests.helpers import quantize_layers, random_model, weight_list_to_layers

LOGIT_FRAC = 5e-3    # the project's end-to-end bound (tests/test_gpu_engine.py, tests/test_gpu_rows.py)
MIN_LIVE = 1e-3      # a condition on the INPUTS: the oracle's own change at the first decode step, as a fraction of the logit range;
                     # above one fp16 rounding (2**-11) of the final hidden state, below the 1.9e-3 measured at 300 keys
MAX_LOST = 0.10      # (probe, step) pairs lost to diverged histories; `live` probes that lose their first decode step
MIN_GAP = 2 * LOGIT_FRAC  # top-2 gap of every step of the BASE request, of the logit range: no engine within LOGIT_FRAC of the oracle
                     # can part from the base history (test_gpu_rows.py _follows accepts a flip below this gap), which would lose
                     # every probe of that row at once
MAX_FORWARDS = 64    # probed requests per case (one forward serves the `live` and the `other_row` probe of a position)
N_CAND, N_CAND_LAST = 8, 450  # replacement tokens to choose from per probed position / for a row's last prompt token

# the smallest shapes every path accepts (hidden 256 / 512); no path under test declined them
SHAPES = {
    64: dict(head_num=4, size_per_head=64, inter_size=1024, vocab_size=512, rotary_dim=16, start_id=0, end_id=2),
    128: dict(head_num=4, size_per_head=128, inter_size=2048, vocab_size=512, rotary_dim=32, start_id=0, end_id=2),
}
NUM_CU = 256  # workgroups of the persistent kernels' default grid on the target (only the persistent chunk below depends on it)


def persist_chunk(B, nh, dh, s_max, nb=0):
    """(nsplit, keys of a split chunk, long register form) of the one- / two-row kernel: persist_plan() in csrc/kernels_persist.hip"""
    nb = nb or NUM_CU
    short = 8 * (64 // (dh // 8)) * 8  # PS_NW * KPI * PS_UK keys: the short form's capacity
    chunk = lambda n: (-(-s_max // n) + 15) & ~15
    nsplit = min(nb // (B * nh), 16)
    ns = 1
    while ns < nsplit and chunk(ns) > short:
        ns += 1
    if chunk(ns) <= short:
        nsplit = min(nsplit, max(ns, 2))
    return nsplit, chunk(nsplit), chunk(nsplit) > short


def rows_block(dh):
    """keys of a block of the rows kernel's attention stream: RW_KVB * KPI (csrc/rows_device.hip.h)"""
    return 4 * (64 // (dh // 8))


class Case:
    """One base request and its probes.  lens: the rows' prompt lengths (padded to S = max(lens) with end_id); env: the engine's
    switches; path: the stats()["decode_path"] the GPU test must see ("batcher": the rows kernel over paged K/V, 3); units: the key
    counts whose multiples the probe positions of a long prompt surround; rows: the rows that are probed (None: all); positions:
    {row: [position, ...]} instead of the rule, for the cases whose oracle run is slow (every position below the row's length is a
    `live` probe, the others are `pad` probes)."""

    def __init__(self, name, family, dh, int8_mode, lens, out_len, path, env=None, units=(16,), rows=None, seed=None, page_tokens=0, positions=None, child=False):
        self._args = (name, family, dh, int8_mode, lens, out_len, path)
        self._kw = dict(env=env, units=units, rows=rows, page_tokens=page_tokens, positions=positions, child=child)
        self.child = child  # the GPU test runs the case in a child process: a switch that the library reads once per process
        self.name, self.family, self.dh, self.int8_mode = name, family, dh, int8_mode
        self.lens = np.asarray(lens, np.int32)
        self.B, self.S, self.out_len = len(lens), int(max(lens)), out_len
        seed = SEEDS.get(name, 0) if seed is None else seed
        self.path, self.env, self.units, self.seed, self.page_tokens = path, dict(env or {}), tuple(units), seed, page_tokens
        self.cfg = dict(SHAPES[dh], num_layer=1 if family == "one" else 2)
        assert family in ("one", "iso0", "iso1") and not (int8_mode and family != "one")
        rng = np.random.RandomState(zlib.crc32(name.encode()) % (1 << 31) + seed)
        self.ids = np.full((self.B, self.S), self.cfg["end_id"], np.int32)
        for b in range(self.B):
            self.ids[b, :self.lens[b]] = rng.randint(3, self.cfg["vocab_size"], size=self.lens[b])
        self.positions = positions
        self.probe_rows = sorted(positions) if positions else list(range(self.B)) if rows is None else list(rows)
        self.probes = self._probes(rng)
        # the replacement token of a probed position: one of the seeded candidates, never the token that is there -- the first one
        # with which the ORACLE's histories of the probed row stay together over the whole request (PICKS; without an entry the
        # first candidate).  Only the reference decides: what a kernel computes never enters the choice.  A row's LAST prompt token
        # decides its first generated token as well: there the search goes through N_CAND_LAST candidates (small requests only).
        self.cand = {}
        for _, row, pos in self.forwards():
            self.cand[(row, pos)] = [int(t) for t in rng.permutation(np.arange(3, self.cfg["vocab_size"])) if t != self.ids[row, pos]]
        self.set_picks(PICKS.get(name, "") if seed == SEEDS.get(name, 0) else "")

    def reseeded(self, seed):
        return Case(*self._args, seed=seed, **self._kw)

    def set_picks(self, picks):
        keys = [(r, p) for _, r, p in self.forwards()]
        picks = [int(d) for d in picks.split()] or [0] * len(keys)
        assert len(picks) == len(keys), (self.name, len(picks), len(keys))
        self.picks = " ".join(str(d) for d in picks)
        self._new = {k: self.cand[k][d] for k, d in zip(keys, picks)}

    # ---- probe positions ----
    def _positions(self, n, rng):
        """positions in [0, n): all of them up to 64 keys; else both ends, the two keys on either side of every multiple of a unit,
        five random ones"""
        if self.S <= 64:
            return list(range(n))
        pos = {0, 1, n - 1, n - 2}
        for u in self.units:
            for m in range(u, n, u):
                pos |= {m - 1, m}
        pos |= set(int(x) for x in rng.randint(0, n, size=5))
        return sorted(p for p in pos if 0 <= p < n)

    def _probes(self, rng):
        live, pad = [], []
        for row in self.probe_rows if self.positions else []:
            live += [(row, p) for p in self.positions[row] if p < self.lens[row]]
            pad += [(row, p) for p in self.positions[row] if p >= self.lens[row]]
        for row in [] if self.positions else self.probe_rows:
            live += [(row, p) for p in self._positions(int(self.lens[row]), rng)]
            tail = list(range(int(self.lens[row]), self.S))
            if len(tail) > 4:  # a padded tail: its first two and last keys, and one inside
                tail = sorted({tail[0], tail[1], tail[len(tail) // 2], tail[-1]})
            pad += [(row, p) for p in tail if self.path != "batcher"]  # (a request of the batcher has no padding)
        if len(live) + len(pad) > MAX_FORWARDS:
            # too many for one test: keep the pad probes, both ends of every row and the neighbours of the coarser units, and fill
            # up with a seeded choice of the others
            coarse = [u for u in self.units if u != 16] or [16]
            keep = [q for q in live if q[1] < 2 or q[1] >= self.lens[q[0]] - 2 or any((q[1] + 1) % u == 0 or q[1] % u == 0 for u in coarse)]
            if len(keep) + len(pad) > MAX_FORWARDS:
                keep = [keep[i] for i in sorted(rng.permutation(len(keep))[:MAX_FORWARDS - len(pad)])]
            rest = [q for q in live if q not in keep]
            room = MAX_FORWARDS - len(pad) - len(keep)
            live = sorted(keep + [rest[i] for i in rng.permutation(len(rest))[:room]])
        out = [(r, p, "live") for r, p in live] + [(r, p, "pad") for r, p in pad]
        if self.B > 1:
            out += [(r, p, "other_row") for r, p in live]
        return out

    def forwards(self):
        """the probed requests, one per (row, position): [(kinds, row, position)]"""
        seen = {}
        for row, pos, kind in self.probes:
            seen.setdefault((row, pos), []).append(kind)
        return [(tuple(k), r, p) for (r, p), k in seen.items()]

    def probed_ids(self, row, pos):
        ids = self.ids.copy()
        ids[row, pos] = self._new[(row, pos)]
        return ids

    def observed(self, row, kind):
        return [row] if kind == "live" else [b for b in range(self.B) if kind == "pad" or b != row]

    # ---- the model ----
    def weights(self):
        cfg = self.cfg
        w = random_model(cfg, seed=zlib.crc32(self.name.encode()) % 1000 + 17 * self.seed, std=0.04)
        if self.family != "one":
            L, dead = 2, 1 if self.family == "iso0" else 0
            for g in (4, 8, 9):  # out.kernel, ffn2.kernel, ffn2.bias (the out-projection has no bias in random_model)
                w[g * L + dead] = np.zeros_like(w[g * L + dead])
        return w

    def oracle(self):
        w = self.weights()
        layers, glob = weight_list_to_layers(self.cfg, w)
        if self.int8_mode:
            layers = quantize_layers(layers)
        return orc.Model(dict(self.cfg, fp16=1, int8_mode=self.int8_mode), layers, glob)

    def __repr__(self):
        return self.name


def oracle_run(model, case, ids):
    r = model.generate(ids, case.lens, case.out_len, return_logits=True)
    return dict(output_ids=r["output_ids"], logits=r["logits"])


def probe_report(base, probed, case, probe):
    """Per observed row of the probe: {row: [(step, max |logit delta|), ...]} over the decode steps (>= 1) at which the two runs'
    histories still agree: every token generated before the step is equal in both runs and none of them is end_id."""
    row, _, kind = probe
    out = {}
    for b in case.observed(row, kind):
        n = int(case.lens[b])
        gb, gp = base["output_ids"][b, n:n + case.out_len], probed["output_ids"][b, n:n + case.out_len]
        steps = []
        for t in range(1, case.out_len):
            if gb[t - 1] != gp[t - 1] or gb[t - 1] == case.cfg["end_id"]:
                break
            steps.append((t, float(np.abs(probed["logits"][t, b] - base["logits"][t, b]).max())))
        out[b] = steps
    return out


def lost_fraction(reports, case):
    """(fraction of (probe, observed row, decode step) pairs lost, fraction of `live` probes without their first decode step)"""
    pairs = got = live = live_lost = 0
    for (row, pos, kind), rep in reports:
        for b, steps in rep.items():
            pairs += case.out_len - 1
            got += len(steps)
        if kind == "live":
            live += 1
            live_lost += not rep[row]
    return 1.0 - got / max(pairs, 1), live_lost / max(live, 1)


def logit_range(logits_row):
    """the scale of the project's logit bounds: max |logit| of the reference row (tests/test_gpu_rows.py _follows)"""
    return float(np.abs(logits_row).max())


def base_gap(case, base):
    """smallest top-2 gap, as a fraction of the row's logit range, over the steps of the base request that produce a token a later
    step depends on -- of the probed rows (the other rows are compared with the engine's own base run only)"""
    for b in range(case.B):  # (a row that ends has no logits behind its end token: such a seed is not taken)
        n = int(case.lens[b])
        if case.cfg["end_id"] in base["output_ids"][b, n:n + case.out_len]:
            return 0.0
    gaps = []
    for b in case.probe_rows:
        for t in range(case.out_len - 1):
            top2 = np.sort(base["logits"][t, b])[-2:]
            gaps.append(float(top2[1] - top2[0]) / logit_range(base["logits"][t, b]))
    return min(gaps)


def reference_figures(case, model=None):
    """The oracle on the base request and on every probe: (base, {(row, pos): run}, reports, figures)."""
    model = model or case.oracle()
    base = oracle_run(model, case, case.ids)
    runs = {(r, p): oracle_run(model, case, case.probed_ids(r, p)) for _, r, p in case.forwards()}
    reports = [(pr, probe_report(base, runs[(pr[0], pr[1])], case, pr)) for pr in case.probes]
    first = [rep[pr[0]][0][1] / logit_range(base["logits"][1, pr[0]]) for pr, rep in reports if pr[2] == "live" and rep[pr[0]]]
    lost, live_lost = lost_fraction(reports, case)
    fig = dict(probes=len(case.probes), forwards=len(runs), lost=lost, live_lost=live_lost, min_live=min(first) if first else 0.0,
               min_gap=base_gap(case, base))
    return base, runs, reports, fig


_REFERENCE = {}


def reference(case):
    """reference_figures(case), computed once per process and left unchanged (both test files read it)"""
    if case.name not in _REFERENCE:
        _REFERENCE[case.name] = reference_figures(case)
    return _REFERENCE[case.name]


def _ragged(S, B, lo, seed):
    rng = np.random.RandomState(seed)
    lens = rng.randint(lo, S, size=B)
    lens[0] = S
    return [int(x) for x in lens]


def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    LAUNCHES = dict(FTCF_PERSIST="0", FTCF_STAGE_MAX_ROWS="4")
    # ---- the one- / two-row persistent kernel (PsAttn).  Short contexts take two splits (persist_plan(): the fewest splits whose
    # chunk fits a short trip, at least two; FTCF_PERSIST_NB=6 leaves one workgroup per head: ONE split, the cap of that grid).
    # s_max = S + out_len picks the chunk: 17..32 -> 16 keys, 33..64 -> 32.  chunk16: the prompt lies across the chunk edge (keys
    # 15 | 16 are prompt keys); chunk32: the context length sweeps 28..35 over the edge (chunk - 1, chunk, chunk + 1) while the
    # request runs.  Two rows: row 0's prompt across the edge, row 1's length sweeping over it, padding behind row 1 ----
    for dh in (64, 128):
        for i8 in (0, 1):
            add(f"persist1_dh{dh}_i{i8}_chunk16", "one", dh, i8, [20], 8, 1, units=(16, persist_chunk(1, 4, dh, 28)[1]))
            add(f"persist1_dh{dh}_i{i8}_chunk32", "one", dh, i8, [28], 8, 1, units=(16, persist_chunk(1, 4, dh, 36)[1]))
    add("persist1_dh64_i0_one_split", "one", 64, 0, [20], 7, 1, env=dict(FTCF_PERSIST_NB="6"))
    for dh in (64, 128):
        for i8 in (0, 1):
            add(f"persist2_dh{dh}_i{i8}_ragged", "one", dh, i8, [40, 27], 7, 1, units=(16, persist_chunk(2, 4, dh, 47)[1]))
    # the long register form (PS_UK_LONG): a chunk above 256 keys at size_per_head 128.  test_persistent_kernel_long_key_ranges
    # reaches it with FTCF_PERSIST_NB=24 on 4200 keys; with 4 heads 24 workgroups give six splits and the long form needs more than
    # 1536 keys, where one key's share (1 / 1536) puts the ORACLE's change below MIN_LIVE.  Ten workgroups and two rows leave one
    # split: the long form from 257 keys on.
    # Row r of a lane's registers holds keys 32 r + ...: rows 8..15 live in the second register batch, from key 256 on.
    add("persist2_dh128_long_form", "one", 128, 0, [262, 207], 5, 1, env=dict(FTCF_PERSIST_NB="10"),
        positions={0: [0, 1, 31, 32, 63, 64, 127, 128, 191, 192, 223, 224, 255, 256, 257, 260, 261],
                   1: [0, 31, 32, 100, 150, 205, 206, 207, 208, 261]})
    # ---- the per-stage launches (mmha_partial) ----
    add("launches1_dh64_short", "one", 64, 0, [27], 8, 0, env=LAUNCHES)
    # (three rows with the one- / two-row kernel off would go to the rows kernel: FTCF_ROWS=0 keeps them on the launches)
    add("launches3_dh128_i1_ragged", "one", 128, 1, [20, 9, 15], 7, 0, env=dict(LAUNCHES, FTCF_ROWS="0"))
    # 300 keys at size_per_head 64: five splits of 64 keys, the register form (mmha_pick_nsplit() keeps 64 keys or more per split).
    # With FTCF_MMHA_WGS=1 it is ONE split of 320 keys, above the 256 that a workgroup holds in registers: the looped form, rounds of
    # STEP = 256 keys, two in flight, the tail clamped to the last cached row.  The library reads that switch once per process.
    add("launches1_dh64_300keys", "one", 64, 0, [300], 5, 0, env=LAUNCHES, units=(16, 64))
    add("launches1_dh64_looped", "one", 64, 0, [300], 5, 0, env=dict(LAUNCHES, FTCF_MMHA_WGS="1"), units=(16, 256), child=True)
    # ---- the general path (launch_mmha behind the per-GEMM launches) ----
    # (a row's last prompt token decides its first generated token: that probe is lost, so the probed rows are not the short ones)
    add("general5_dh128_ragged", "one", 128, 0, [20, 7, 20, 3, 14], 7, 2, env=dict(FTCF_ROWS="0"), rows=[0, 2, 4])
    add("general5_dh64_i1_ragged", "one", 64, 1, [14, 5, 20, 20, 2], 7, 2, env=dict(FTCF_ROWS="0"), rows=[0, 2, 3])
    # ---- the rows kernel (RwAt<DH, false>).  Default grid: fewer (row, head) pairs than workgroups, every pair is shared by FX = 8
    # workgroups.  FTCF_ROWS_NB=26: rows_plan() shares a pair only when no workgroup holds a whole one, so the small grid is the
    # other form: two whole pairs + a third on 12 workgroups at 16 rows (FX = 1), the ring running on from pair to pair ----
    add("rows3_dh64_ragged", "one", 64, 0, [21, 9, 16], 7, 3, units=(16, 32))
    add("rows3_dh128_i1_ragged", "one", 128, 1, [21, 16, 5], 7, 3)
    add("rows5_dh128_ragged", "one", 128, 0, [20, 7, 20, 3, 14], 8, 3, rows=[0, 2, 4])
    add("rows5_dh64_i1_ragged", "one", 64, 1, [20, 20, 4, 15, 6], 8, 3, rows=[0, 1, 3])
    add("rows16_dh128_ragged", "one", 128, 0, _ragged(20, 16, 6, 5), 6, 3, rows=[0, 3])
    add("rows16_dh64_i1_small_grid", "one", 64, 1, _ragged(30, 16, 8, 6), 6, 3, env=dict(FTCF_ROWS_NB="26"), rows=[0, 9],
        units=(16, 32))
    # The ring in steady rotation: thirteen rows on 13 workgroups are four whole pairs each (FX = 1), workgroup 0 holds heads of
    # rows 0, 3, 6, 9.  225 keys and more are eight blocks of 32 per pair: streamer wave 0 takes blocks 0 and 7 of each of its four
    # pairs, T = 8 blocks through a ring of four slots -- the steady-rotation loop of RwAt::run, every slot refilled while the
    # stream runs on from pair to pair.  Probed: keys of blocks 0 and 7 (wave 0's) and of blocks between, of the first and the last
    # pair of workgroup 0.  (A wave with more than four blocks of ONE pair needs 29 blocks per pair: 449 keys at size_per_head 128,
    # 897 at 64, on seven rows or more -- there one key's share puts the oracle's change at or below MIN_LIVE and an oracle
    # request costs seconds: not reached here.)
    lens = [60] * 13
    lens[0] = lens[3] = lens[6] = 232
    lens[9] = 230
    add("rows13_dh64_small_grid_ring", "one", 64, 0, lens, 4, 3, env=dict(FTCF_ROWS_NB="13"),
        positions={0: [0, 1, 31, 32, 100, 170, 223, 224, 227, 228, 230, 231], 9: [5, 31, 32, 223, 224, 227, 228, 231]})
    # ---- the rows kernel over the batcher's page tables (RwAt<DH, true>): no padding there, every request has its own length ----
    add("paged3_dh128_pages16", "one", 128, 0, [37, 18, 30], 6, "batcher", env=dict(FTCF_BATCHER_ROWS="1"), units=(16,), page_tokens=16)
    add("paged4_dh64_i1_pages32", "one", 64, 1, [45, 31, 60, 14], 6, "batcher", env=dict(FTCF_BATCHER_ROWS="1"), units=(16, 32), page_tokens=32, rows=[0, 2])
    # ---- two layers, one of them live: the caches of layer 0 and of layer 1 ----
    for fam in ("iso0", "iso1"):
        add(f"persist2_dh128_{fam}", fam, 128, 0, [40, 27], 7, 1, units=(16, persist_chunk(2, 4, 128, 47)[1]))
        add(f"rows3_dh64_{fam}", fam, 64, 0, [20, 14, 7], 7, 3, units=(16, 32))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def find_picks(case):
    """per probed position the first candidate with which the oracle's histories of the probed row agree over every step (the one
    that keeps most steps where none does); pad positions take the first"""
    model = case.oracle()
    base = oracle_run(model, case, case.ids)
    picks = []
    for kinds, r, p in case.forwards():
        best, best_n = 0, -1
        for d in range(0 if "live" not in kinds else N_CAND_LAST if p == case.lens[r] - 1 and case.B * case.S <= 256 else N_CAND):
            ids = case.ids.copy()
            ids[r, p] = case.cand[(r, p)][d]
            n = len(probe_report(base, oracle_run(model, case, ids), case, (r, p, "live"))[r])
            if n > best_n:
                best, best_n = d, n
            if n == case.out_len - 1:
                break
        picks.append(str(best))
    return " ".join(picks)


# Pinned by `python -m tests.attention_probe_cases`: SEEDS -- the first seed (from 0; cases without an entry take 0) at which the
# oracle meets MIN_GAP and MIN_LIVE, loses at most half of MAX_LOST of the (probe, step) pairs and the first decode step of at most
# 7.5 % of the live probes; PICKS -- find_picks() at that seed, per probed request in the order of Case.forwards().
# test_attention_probe_reference.py checks the conditions on what is pinned here.
SEEDS = {
    "rows13_dh64_small_grid_ring": 3,
    "persist1_dh64_i0_chunk16": 3,
    "persist1_dh64_i0_chunk32": 2,
    "persist1_dh64_i1_chunk16": 9,
    "persist1_dh128_i0_chunk16": 21,
    "persist1_dh128_i0_chunk32": 4,
    "persist1_dh128_i1_chunk16": 10,
    "persist1_dh128_i1_chunk32": 2,
    "persist1_dh64_i0_one_split": 6,
    "persist2_dh64_i0_ragged": 1,
    "persist2_dh64_i1_ragged": 1,
    "persist2_dh128_long_form": 16,
    "launches3_dh128_i1_ragged": 19,
    "general5_dh64_i1_ragged": 5,
    "general5_dh128_ragged": 1,
    "rows3_dh64_ragged": 9,
    "rows3_dh128_i1_ragged": 4,
    "rows5_dh128_ragged": 4,
    "rows5_dh64_i1_ragged": 3,
    "rows16_dh128_ragged": 2,
    "rows16_dh64_i1_small_grid": 2,
    "paged3_dh128_pages16": 2,
    "paged4_dh64_i1_pages32": 2,
    "persist2_dh128_iso0": 2,
    "rows3_dh64_iso0": 1,
    "persist2_dh128_iso1": 1,
    "rows3_dh64_iso1": 5,
}
PICKS = {
    "rows13_dh64_small_grid_ring": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0",
    "launches1_dh64_looped": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0",
    "persist1_dh64_i0_chunk16": "0 1 0 1 1 1 0 0 0 1 0 0 0 2 1 0 4 2 0 24",
    "persist2_dh128_i0_ragged": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 2 0 0 0 0 2 0 1 0 0 0 0 1 0 0 0 3 0 0 0 0 0",
    "persist1_dh64_i0_chunk32": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0",
    "persist1_dh64_i1_chunk16": "0 0 0 0 0 0 0 0 0 0 2 0 0 0 0 0 0 0 0 3",
    "persist1_dh64_i1_chunk32": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 1 0",
    "persist1_dh128_i0_chunk16": "0 0 0 0 0 0 0 0 0 0 0 0 1 0 0 0 0 0 0 5",
    "persist1_dh128_i0_chunk32": "0 0 0 1 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0",
    "persist1_dh128_i1_chunk16": "0 0 0 0 0 0 0 0 0 0 1 0 0 0 0 0 0 0 0 14",
    "persist1_dh128_i1_chunk32": "0 0 0 0 0 0 0 0 2 0 2 2 0 1 0 0 0 0 0 0 0 0 0 0 0 0 0 35",
    "persist1_dh64_i0_one_split": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 10",
    "persist2_dh64_i0_ragged": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 1 0 0 2 0 0 1 0 1 0 0 0 0 5 1 0 0 0 0 0 0",
    "persist2_dh64_i1_ragged": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 1 0 0 0 0 0 0 0 18 0 1 4 0 5 0 0 0 0 0 2 0 0 0 0 0 1 0 0 4 0 0 0 0 0 0 0",
    "persist2_dh128_i1_ragged": "1 0 2 0 0 0 0 0 0 0 0 0 0 0 0 1 0 1 0 1 1 1 3 0 0 0 1 0 0 0 0 0 0 0 0 0 0 0 1 1 1 0 1 0 0 1 5 3 2 1 0 4 0 3 0 0 1 1 1 6 0 0 0 0",
    "persist2_dh128_long_form": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 2 0 0 0 0 0 0 0 0 0 0",
    "launches1_dh64_short": "0 1 0 0 1 0 0 0 1 0 4 0 0 0 0 0 0 0 1 2 0 0 0 0 0 1 50",
    "launches3_dh128_i1_ragged": "1 0 0 0 0 0 0 0 0 0 1 0 0 0 1 1 0 0 0 31 2 0 4 1 7 6 0 1 20 3 1 2 0 2 1 1 0 0 0 0 1 0 1 0 0 0 0 0 0 0 0 0",
    "launches1_dh64_300keys": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0",
    "general5_dh64_i1_ragged": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 1 0 0 0 2 0 1 1 0 0 0 0 0 2 0 4 0 18 0 0 1 1 0 2 0 0 2 3 0 1 0 2 0 0 0 0 1 25 0 0 0 0",
    "general5_dh128_ragged": "1 1 0 0 0 0 0 0 4 3 4 0 0 0 2 2 0 0 6 329 1 0 0 7 0 0 0 2 0 1 0 1 1 1 0 0 0 0 0 0 0 0 0 0 0 0 0 2 0 0 0 0 0 0 0 0 0 0",
    "rows3_dh64_ragged": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 2 0 0 1 0 0 0 0 0 1 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0",
    "rows3_dh128_i1_ragged": "0 1 0 2 1 1 0 0 0 0 0 0 0 0 4 0 6 0 0 0 0 0 0 0 0 0 0 0 0 2 0 0 0 0 0 0 0 5 2 1 0 0 0 0 0 0 0 0 0 0",
    "rows5_dh128_ragged": "0 0 1 0 0 3 0 0 0 1 0 0 0 0 0 2 1 0 0 249 0 0 0 0 0 0 0 0 0 0 0 0 2 0 0 0 1 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0",
    "rows5_dh64_i1_ragged": "0 0 0 0 0 0 0 0 0 2 0 0 0 0 0 0 0 0 0 0 0 0 0 0 1 0 0 1 1 0 4 2 0 0 0 0 1 0 0 26 1 1 0 1 2 0 1 0 0 0 1 0 0 2 0 0 0 0 0",
    "rows16_dh128_ragged": "0 0 0 0 0 0 6 0 1 0 4 0 1 0 3 0 2 0 1 0 1 0 0 0 2 0 0 0 0 1 0 0 0 0 0 0",
    "rows16_dh64_i1_small_grid": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 1 7 3 4 0 0 0 0 0 0 0 0",
    "paged3_dh128_pages16": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 1 2 19 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0",
    "paged4_dh64_i1_pages32": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 175 0 0 0 0 2 0 0 0 0 0 0 0 0 0 0 0 1 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0",
    "persist2_dh128_iso0": "0 0 0 0 0 0 1 0 4 0 0 0 0 0 0 0 0 0 0 0 0 0 1 0 0 0 1 0 0 0 0 1 0 0 31 3 2 2 0 0 0 0 0 2 0 0 1 0 1 0 0 0 0 0 0 1 0 0 1 0 0 0 0 0",
    "rows3_dh64_iso0": "0 0 0 0 0 0 1 0 0 0 0 0 1 0 0 6 0 0 2 0 0 0 0 1 0 2 0 0 0 0 0 0 0 0 0 0 6 0 0 0 0 0 0 0 0 0 0 0 0",
    "persist2_dh128_iso1": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 3 1 1 0 2 3 0 0 0 0 0 0 0 4 6 2 0 6 0 1 0 0 0 0 0 0",
    "rows3_dh64_iso1": "0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 2 2 0 0 0 0 0 0 3 0 2 0 0 0 3 3 0 0 5 0 0 0 0 0 0 0 0 0 0",
}


if __name__ == "__main__":
    import sys
    import time
    only = sys.argv[1:]
    for c in cases():
        if only and not any(o in c.name for o in only):
            continue
        for seed in range(0, 24):
            cs = c.reseeded(seed)
            t0 = time.time()
            gap = base_gap(cs, oracle_run(cs.oracle(), cs, cs.ids))
            if gap < MIN_GAP:
                print(f'# {c.name} seed {seed}: min_gap {gap:.4f}', file=sys.stderr, flush=True)
                continue
            cs.set_picks(find_picks(cs))
            _, _, _, fig = reference_figures(cs)
            # (the search asks for less than the caps: an engine may lose a probe of its own at a near tie of a probed request)
            ok = fig["min_live"] >= MIN_LIVE and fig["lost"] <= MAX_LOST / 2 and fig["live_lost"] <= 0.075
            print(f'# {c.name} seed {seed}: {fig} {time.time() - t0:.1f}s {"OK" if ok else ""}', file=sys.stderr, flush=True)
            if ok:
                print(f'SEED "{c.name}": {seed},\nPICK "{c.name}": "{cs.picks}",', flush=True)
                break
