"""Writes tests/golden/holdout_folds_table.json: the cross-validated lambda path of tests/holdout_folds_restatement.py on the
four table inputs of tests/test_holdout_cpu.py (96 x 128, scale 2, 6 frames, BTV(2, 0.5); 5 folds, mask seed 1, no final
solve), and the same path with the observations moved by 1e-13 * standard_normal (default_rng(99)) -- what separates two
orders of a sum.  Per input, row and fold: the score, the held-out count and the solve's counts (IRLS rounds, inner
iterations, evaluations), and whether the counts are STABLE (equal in the two runs); per row the mean, the standard error
over the folds and how far each MOVES (relative); the rows chosen under both rules in both runs.
tests/test_gpu_holdout_folds.py holds the GPU path to these; tests/test_holdout_folds_cpu.py re-measures them.
   python tests/golden/make_holdout_folds_table.py     (about ten minutes; ALGLIB through oracle/_ref when that is built)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import oracle as orc  # noqa: E402
import holdout_folds_restatement as hfr  # noqa: E402
import test_holdout_cpu as cpu  # noqa: E402
import test_holdout_folds_cpu as folds_cpu  # noqa: E402


def run(P, y, delta, name):
    rows = folds_cpu.run_path(P, y, delta, name)["rows"]
    mean, se = [r["mean"] for r in rows], [r["se"] for r in rows]
    return dict(scores=[[float(f["score"]) for f in r["folds"]] for r in rows],
                counts=[[[f["report"].irls_rounds, f["report"].cg_iterations, f["report"].nfev] for f in r["folds"]] for r in rows],
                held=[[float(f["sums"][0][3]) for f in r["folds"]] for r in rows],
                pooled=[[float(v) for v in r["pooled"]] for r in rows], mean=mean, se=se,
                chosen_min=hfr.choose_folds(mean, se, hfr.RULE_MIN)[0], chosen_one_se=hfr.choose_folds(mean, se, hfr.RULE_ONE_SE)[0])


def main():
    P, inputs = cpu._inputs()
    out = {"solver": "ALGLIB (oracle/_ref)" if orc.have_ref() else "the oracle's mincg", "amplitude": 1e-13, "inputs": {}}
    for name, (y, delta) in inputs.items():
        a = run(P, y, delta, name)
        b = run(P, y + 1e-13 * np.random.default_rng(99).standard_normal(y.shape), delta, name)
        rec = {"lambda": cpu.LAMBDA, "scales": cpu.SCALES[name], "folds": folds_cpu.FOLDS, "mask_seed": folds_cpu.SEEDS[name],
               "huber_delta": delta}
        rec.update(a)
        rec.update({"chosen_min_moved": b["chosen_min"], "chosen_one_se_moved": b["chosen_one_se"],
                    "stable": [[ca == cb for ca, cb in zip(ra, rb)] for ra, rb in zip(a["counts"], b["counts"])],
                    "mean_move": [abs(u - v) / u for u, v in zip(a["mean"], b["mean"])],
                    "se_move": [abs(u - v) / u for u, v in zip(a["se"], b["se"])]})
        out["inputs"][name] = rec
        print(name, "min", rec["chosen_min"], rec["chosen_min_moved"], "one_se", rec["chosen_one_se"], rec["chosen_one_se_moved"],
              "stable", [sum(r) for r in rec["stable"]], "mean", ["%.1e" % v for v in rec["mean_move"]],
              "se", ["%.1e" % v for v in rec["se_move"]], flush=True)
    with open(os.path.join(HERE, "holdout_folds_table.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
