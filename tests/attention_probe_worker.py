"""Child process of test_gpu_attention_probes.py for the cases whose switches the library reads once per process (FTCF_MMHA_WGS):
python -m tests.attention_probe_worker CASE OUT.npz runs the case's base request twice and every probed request on one engine
(the switches come with the environment) and stores the logits, tokens and decode paths."""
import sys

import numpy as np


def collect(gh, op, case):
    """{"base", "again": run_op dicts, "probed": {(row, pos): run_op dict}, "paths": the decode_path after every request}"""
    V = case.cfg["vocab_size"]
    paths = []

    def run(ids):
        r = gh.run_op(op, ids, case.lens, case.out_len, V, top_k=1)
        paths.append(op.stats()["decode_path"])
        return dict(logits=r["logits"], output_ids=r["output_ids"])

    res = dict(base=run(case.ids), again=run(case.ids))
    res["probed"] = {(r, p): run(case.probed_ids(r, p)) for _, r, p in case.forwards()}
    res["paths"] = paths
    return res


def main(name, out):
    from tests import attention_probe_cases as apc
    from tests import gpu_helpers as gh
    from fastertransformer4codefuse_amd import capi
    capi.require_gpu()
    case = [c for c in apc.cases() if c.name == name][0]
    res = collect(gh, gh.make_op(case.cfg, case.weights(), int8_mode=case.int8_mode), case)
    flat = {"paths": np.asarray(res["paths"])}
    for k in ("base", "again"):
        flat[k + ".logits"], flat[k + ".output_ids"] = res[k]["logits"], res[k]["output_ids"]
    for (r, p), v in res["probed"].items():
        flat[f"p{r}_{p}.logits"], flat[f"p{r}_{p}.output_ids"] = v["logits"], v["output_ids"]
    np.savez(out, **flat)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
