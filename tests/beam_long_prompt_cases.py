"""Beam-search requests whose prompts are longer than one KV split of the decode attention (64 keys), shared by
tests/test_gpu_beam_long_prompts.py, its child process (tests/beam_long_prompt_worker.py) and tools/pick_beam_prompt_seeds.py.

The prompt of a request is random tokens from a seed.  The seed of each request is the one of 20 (0 .. 19) at which the oracle
alone reorders beams within the first steps and keeps the largest smallest selection gap (selection_gaps()): the comparison of
GPU and oracle logits stops at the first step where the two searches select differently, so a prompt whose candidates are far
apart is compared for longer.  tools/pick_beam_prompt_seeds.py prints the gaps; SEEDS records its choice."""
import numpy as np

from oracle import oracle as orc
from tests.helpers import load_tiny, quantize_layers, random_model, weight_list_to_layers
from tests.test_gpu_beam import MID, _replay

LOGIT_FRAC = 5e-3  # the project's end-to-end bound: max |gpu - oracle| logit as a fraction of the oracle's largest

# name -> model, int8_mode, B, K, S, lens, out_len (rows x heads and the split count mmha_pick_nsplit() gives them in the comment)
REQUESTS = {
    "a": dict(model="tiny", int8_mode=0, B=1, K=4, S=200, lens=(200,), out=8),          # 4 x 4, 4 splits
    "b": dict(model="tiny", int8_mode=0, B=2, K=3, S=330, lens=(330, 293), out=8),      # 6 x 4, 6 splits
    "d": dict(model="tiny", int8_mode=0, B=1, K=3, S=70, lens=(70,), out=60),           # 3 splits, half of all keys generated
    "e_fp16": dict(model="mid", int8_mode=0, B=1, K=4, S=200, lens=(200,), out=8),      # 4 x 8, dh 128, 4 splits
    "e_int8": dict(model="mid", int8_mode=1, B=1, K=4, S=200, lens=(200,), out=8),
    "f2": dict(model="tiny", int8_mode=0, B=1, K=2, S=200, lens=(200,), out=8),         # run after "a" on the same engine
}
# the best of seeds 0 .. 19 (tools/pick_beam_prompt_seeds.py); the smallest selection gap of the oracle's search with it, in units
# of log-probability: a 0.0899, b 0.0659, d 0.0169 (60 steps), e_fp16 0.0790, e_int8 0.0565, f2 0.3031
SEEDS = {"a": 8, "b": 3, "d": 8, "e_fp16": 6, "e_int8": 14, "f2": 7}

_models = {}


def model(name):
    """(cfg, weight list, oracle layers, oracle globals) of "tiny" (the golden model) or "mid" (random, dh 128)"""
    if name not in _models:
        if name == "tiny":
            cfg, w, _ = load_tiny()
        else:
            cfg, w = MID, random_model(MID, seed=31, std=0.04)
        layers, glob = weight_list_to_layers(cfg, w)
        _models[name] = (cfg, w, layers, glob)
    return _models[name]


def prompt(name, seed=None):
    """(ids [B, S] padded with end_id, lens [B]) of a request"""
    r = REQUESTS[name]
    cfg = model(r["model"])[0]
    rng = np.random.RandomState(1000 * sorted(REQUESTS).index(name) + (SEEDS[name] if seed is None else seed))
    ids = np.full((r["B"], r["S"]), cfg["end_id"], dtype=np.int32)
    for b, n in enumerate(r["lens"]):
        ids[b, :n] = rng.randint(3, cfg["vocab_size"], size=n)
    return ids, np.asarray(r["lens"], dtype=np.int32)


def oracle_run(name, seed=None):
    """the oracle's beam search of a request, with the raw logits of every step"""
    r = REQUESTS[name]
    cfg, _, layers, glob = model(r["model"])
    if r["int8_mode"]:
        layers = quantize_layers(layers)
    ids, lens = prompt(name, seed)
    return orc.Model(dict(cfg, fp16=1, int8_mode=r["int8_mode"]), layers, glob).generate_beam(ids, lens, r["out"], r["K"],
                                                                                               return_logits=True)


def replay(name, logits, seed=None):
    """the logits of every step pushed through the oracle's beam-search layer -> (output_ids, trace) of tests/test_gpu_beam._replay"""
    r = REQUESTS[name]
    ids, lens = prompt(name, seed)
    o_ids, _, _, trace = _replay(model(r["model"])[0], ids, lens, r["out"], r["K"], logits, orc.BeamParams(r["B"]))
    return o_ids, trace


def selection_gaps(name, logits, trace):
    """per executed step the smallest distance between neighbours among the best K + 1 candidates of any batch entry (candidate =
    a live slot's cumulative log-probability + the log-soft-max of its logits; a finished slot's own score): a logit error of
    that size can change what the step selects or the order it selects it in."""
    r = REQUESTS[name]
    K, gaps = r["K"], []
    for t in range(len(trace["ids"])):
        lg = logits[t].astype(np.float64)
        lp = lg - lg.max(axis=1, keepdims=True)
        lp -= np.log(np.exp(lp).sum(axis=1, keepdims=True))
        g = np.inf
        for e in range(r["B"]):
            cand = []
            for s in range(e * K, (e + 1) * K):
                cand.append(np.array([trace["cum"][t][s]]) if trace["finished"][t][s] else trace["cum"][t][s] + lp[s])
            top = np.sort(np.concatenate(cand))[::-1][:K + 1]
            g = min(g, float(np.min(top[:-1] - top[1:])))
        gaps.append(g)
    return gaps


def reorders(trace, K, first=4):
    """whether some slot selected within the first steps continues another slot's history (parent != its own index)"""
    par = trace["parents"][1:first]  # (step 0 expands beam 0 only)
    return bool((par % K != np.arange(par.shape[1]) % K).any())
