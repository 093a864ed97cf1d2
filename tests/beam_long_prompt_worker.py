"""Child process of test_gpu_beam_long_prompts.py for a request under a switch the library reads once per process (FTCF_MMHA_WGS):
python -m tests.beam_long_prompt_worker REQUEST OUT.npz runs the request on a fresh engine (the switch comes with the environment)
and stores its tokens and the logits of every step."""
import sys

import numpy as np


def run(gh, name, op=None):
    """a request of tests/beam_long_prompt_cases.py through the engine -> run_op_beam's dict (with logits) and the engine"""
    from tests import beam_long_prompt_cases as cases
    r = cases.REQUESTS[name]
    cfg, w = cases.model(r["model"])[:2]
    op = op or gh.make_op(cfg, w, int8_mode=r["int8_mode"])
    ids, lens = cases.prompt(name)
    res = gh.run_op_beam(op, ids, lens, r["out"], cfg["vocab_size"], r["K"], return_logits=True)
    assert op.stats()["decode_path"] == 2  # beams read K/V through the cache indirection: the general path
    return res, op


def main(name, out):
    from tests import gpu_helpers as gh
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    res, _ = run(gh, name)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
