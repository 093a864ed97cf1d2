"""The requests of tests/test_gpu_speculative_sampled.py (speculative decoding of top-k sampled requests)
and the rule that makes them fair.  A sampled run with speculation must give the plain sampled run's tokens for the same seed;
the two take different GEMM forms (a pass runs the burst GEMMs), so their logits differ as tests/test_gpu_log_probs.py bounds
(GEMM_FORM_TOL, atol 5e-3), and a draw that lands within that of a bucket boundary may fall either way in either run.  Every
entry of CASES is a request whose every step is STABLE on the CPU oracle's logits (tests/test_speculative_sampled_host.py
replays them): no step's draw is near a boundary and no pick is near its neighbours in value.

A step, restated from kernels_sampling.hip / oracle/ftcf_oracle.c: the temperature-scaled logits sorted by value descending, index
ascending; c_j = the cumulative sums of exp(l - l_max) over the top k; x = u * p_topk * c_k with u = uniform(seed, 0, step
index); the pick is the first j with x <= c_j.  Stable: min_j |x - c_j| / c_k >= MARGIN over the k - 1 interior boundaries and
the pick's logit differs from both sorted neighbours (the (k + 1)-th included) by >= MARGIN.  MARGIN = 1e-2 is twice the atol of
GEMM_FORM_TOL: a logit error eps moves a boundary by at most eps / 2 of c_k.  That bound is one on the model's logits; the walk
sees them multiplied by 1 / T, and an error eps with them, so under a temperature T < 1 both thresholds are MARGIN / T (the first
table, picked with MARGIN alone, had the engine's own PLAIN run leave the oracle's tokens at T = 0.3, golden prompt, fp16, seed 0,
token 11)."""
import numpy as np

MARGIN = 1e-2
OUT_LEN = 16
M64 = (1 << 64) - 1


def splitmix64(z):
    z = (z + 0x9e3779b97f4a7c15) & M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def uniform(seed, row, draw):
    """ftcf_uniform (sampling_device.hip.h) = orc_uniform (oracle/ftcf_oracle.c): (0, 1], a float32"""
    z = splitmix64((seed & M64) ^ splitmix64((row * 0x632be59bd9b4e019 + draw) & M64))
    return np.float32((z >> 40) + 1) * np.float32(1.0 / 16777216.0)


def repeating_prompt(V, seed=1):
    """tests/test_gpu_speculative.py repeating_prompt: a random block twice, then its first tokens"""
    blk = np.random.RandomState(seed).randint(3, V, size=12).tolist()
    return blk + blk + blk[:4]


def p_topk_of(top_p):
    """the p of the top-k layer (engine.hip.h route_sampling_args): a top-k row without a p samples from all of its k"""
    return 1.0 if top_p == 0.0 else min(max(top_p, 0.0), 1.0)


def step_walk(logits, k, temperature, top_p, seed, draw):
    """One step restated -> (token, stable, the pick's place in the sorted order)."""
    l = np.asarray(logits, np.float32)
    if temperature != 1.0:
        l = l * (np.float32(1.0) / (np.float32(temperature) + np.float32(1e-6)))
    order = np.lexsort((np.arange(l.size), -l.astype(np.float64)))
    top = l[order[:k + 1]].astype(np.float64)
    c = np.cumsum(np.exp(top[:k] - top[0]))
    x = float(uniform(seed, 0, draw)) * p_topk_of(top_p) * c[-1]
    pick = next((j for j in range(k) if x <= c[j]), k - 1)
    margin = np.abs(x - c[:k - 1]).min() / c[-1] if k > 1 else 1.0
    gaps = [abs(top[pick] - top[j]) for j in (pick - 1, pick + 1) if 0 <= j < top.size]
    need = MARGIN / min(1.0, temperature)
    stable = margin >= need and min(gaps) >= need
    return int(order[pick]), bool(stable), pick


def replay(model, prompt, case):
    """The case on the oracle -> (generated tokens, [stable per step], [the pick's place per step]); asserts that the restated
    walk gives the oracle's token at every step."""
    from oracle import oracle as orc
    _, _, k, temperature, top_p, seed = case
    samp = orc.Sampling(1, top_k=k, top_p=top_p, temperature=temperature, random_seed=seed)
    o = model.generate(np.array([prompt], np.int32), [len(prompt)], OUT_LEN, sampling=samp, return_logits=True)
    n = int(o["sequence_lengths"][0])
    gen = o["output_ids"][0, len(prompt):n].tolist()
    stable, places = [], []
    for i, tok in enumerate(gen):
        t, ok, place = step_walk(o["logits"][i, 0], k, temperature, top_p, seed, i)
        assert t == tok, (case, i, t, tok)
        stable.append(ok)
        places.append(place)
    return gen, stable, places


# (prompt, int8_mode, top_k, temperature, top_p, random_seed): every step stable, at least one pick that is not the arg max,
# and on the repeating prompt at least one n-gram draft accepted (K = 4, N = 3)
CASES = [
    ("golden", 0, 2, 1.0, 0.0, 2), ("golden", 0, 4, 1.0, 0.0, 2), ("golden", 0, 50, 1.0, 0.0, 2), ("golden", 0, 50, 0.3, 0.0, 16),
    ("golden", 0, 50, 1.0, 0.7, 2), ("golden", 0, 64, 0.5, 0.0, 4),
    ("repeating", 0, 2, 1.0, 0.0, 8), ("repeating", 0, 4, 1.0, 0.0, 4), ("repeating", 0, 50, 1.0, 0.0, 12), ("repeating", 0, 50, 0.3, 0.0, 72),
    ("repeating", 0, 50, 1.0, 0.7, 6), ("repeating", 0, 64, 0.5, 0.0, 21),
    ("golden", 1, 2, 1.0, 0.0, 4), ("golden", 1, 4, 1.0, 0.0, 0), ("golden", 1, 50, 1.0, 0.0, 2), ("golden", 1, 50, 0.3, 0.0, 24),
    ("golden", 1, 50, 1.0, 0.7, 2), ("golden", 1, 64, 0.5, 0.0, 10),
    ("repeating", 1, 2, 1.0, 0.0, 8), ("repeating", 1, 4, 1.0, 0.0, 6), ("repeating", 1, 50, 1.0, 0.0, 12), ("repeating", 1, 50, 0.3, 0.0, 72),
    ("repeating", 1, 50, 1.0, 0.7, 6), ("repeating", 1, 64, 0.5, 0.0, 18),
]


def prompt_of(name, cfg, z):
    return z["prompt"].tolist() if name == "golden" else repeating_prompt(cfg["vocab_size"])
