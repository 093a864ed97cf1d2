"""Picks the prompt seed of every request of tests/beam_long_prompt_cases.py on the CPU: of seeds 0 .. 19, those at which the oracle's
own search reorders beams within its first steps, and of these the one with the largest smallest selection gap.
python tools/pick_beam_prompt_seeds.py [request ...] prints one line per (request, seed) and the choice."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import beam_long_prompt_cases as cases  # noqa: E402


def main(names):
    for name in names or sorted(cases.REQUESTS):
        K, best = cases.REQUESTS[name]["K"], None
        for seed in range(20):
            o = cases.oracle_run(name, seed)
            _, trace = cases.replay(name, o["logits"], seed)
            gaps = cases.selection_gaps(name, o["logits"], trace)
            ok = cases.reorders(trace, K)
            print(f"{name} seed {seed:2d}: steps {len(gaps)}, reorders early {ok}, smallest gap {min(gaps):.4f} (first steps {min(gaps[:4]):.4f})",
                  flush=True)
            if ok and (best is None or min(gaps) > best[1]):
                best = (seed, min(gaps))
        print(f"{name}: seed {best[0]} (smallest gap {best[1]:.4f})", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
