"""Writes tests/golden/holdout_table.json: the lambda path of tests/holdout_restatement.py on the four table inputs of
tests/test_holdout_cpu.py (96 x 128, scale 2, 6 frames, BTV(2, 0.5), 10 % held out, no final solve), and the same path with
the observations moved by 1e-13 * standard_normal (default_rng(99)) -- what separates two orders of a sum.  Per input and
row: the score, the solve's counts (IRLS rounds, inner iterations, evaluations), whether the counts are STABLE (equal in
the two runs) and the score's SENSITIVITY |score - moved score| / score.  tests/test_gpu_holdout.py holds the GPU path to
these; tests/test_holdout_cpu.py re-measures the scores and the chosen rows.
   python tests/golden/make_holdout_table.py        (about two minutes; ALGLIB through oracle/_ref when that is built)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import oracle as orc  # noqa: E402
import holdout_restatement as hr  # noqa: E402
import robust_restatement as rr  # noqa: E402
import test_holdout_cpu as cpu  # noqa: E402


def run(P, y, delta, name):
    kind, _, rng_, decay = P["reg"]
    res = hr.lambda_path(P["model"], y, rr.bilinear(y[0], P["s"]), (kind, cpu.LAMBDA, rng_, decay), cpu.SCALES[name], 0.1,
                         cpu.SEEDS[name], huber_delta=delta, final_solve=False)
    rows = res["rows"]
    return ([float(r["score"]) for r in rows], [[r["report"].irls_rounds, r["report"].cg_iterations, r["report"].nfev] for r in rows],
            [[float(v) for v in r["sums"][0]] for r in rows], res["chosen"])


def main():
    P, inputs = cpu._inputs()
    out = {"solver": "ALGLIB (oracle/_ref)" if orc.have_ref() else "the oracle's mincg", "amplitude": 1e-13, "inputs": {}}
    for name, (y, delta) in inputs.items():
        scores, counts, sums, chosen = run(P, y, delta, name)
        moved = y + 1e-13 * np.random.default_rng(99).standard_normal(y.shape)
        scores2, counts2, _, chosen2 = run(P, moved, delta, name)
        out["inputs"][name] = {
            "lambda": cpu.LAMBDA, "scales": cpu.SCALES[name], "mask_seed": cpu.SEEDS[name], "huber_delta": delta,
            "scores": scores, "counts": counts, "sums": sums, "chosen": chosen, "chosen_moved": chosen2,
            "stable": [a == b for a, b in zip(counts, counts2)],
            "sensitivity": [abs(a - b) / a for a, b in zip(scores, scores2)]}
        print(name, chosen, chosen2, out["inputs"][name]["stable"], ["%.1e" % v for v in out["inputs"][name]["sensitivity"]], flush=True)
    with open(os.path.join(HERE, "holdout_table.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
