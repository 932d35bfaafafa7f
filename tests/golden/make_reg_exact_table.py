"""Writes tests/golden/reg_exact_table.json: the solves of tests/reg_exact_restatement.py (table_inputs: 96 x 128, scale 2,
6 frames, noise sigma 0.01, BTV decay 0.5, started at the bilinear upsample of frame 0) with the reference's regulariser
gradient and with the exact one, for R 1 .. 3 at lambda 0.005 and 0.02, by CG and by L-BFGS -- results only.  Every solve
runs three more times with the observations moved by 1e-13 * standard_normal (default_rng(99), (100), (101)), which is what
separates two orders of a sum: per solve the PSNR, the counts (IRLS rounds, inner iterations, evaluations), whether the
counts are STABLE (equal in all four runs) and the furthest the PSNR moved.  tests/test_reg_exact_cpu.py pins the gains;
tests/test_gpu_reg_exact.py holds the GPU solves to the rows.
   python tests/golden/make_reg_exact_table.py        (minutes; ALGLIB through oracle/_ref when that is built)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import oracle as orc  # noqa: E402
import reg_exact_restatement as rx  # noqa: E402


def main():
    inp = rx.table_inputs()
    moved = [inp["y"] + 1e-13 * np.random.default_rng(seed).standard_normal(inp["y"].shape) for seed in (99, 100, 101)]
    out = {"solver": "ALGLIB (oracle/_ref)" if orc.have_ref() else "the oracle's mincg", "amplitude": 1e-13,
           "start_psnr": float(orc.psnr(inp["gt"], inp["x0"])), "decay": rx.TABLE_DECAY, "rows": []}
    for R, lam in rx.TABLE_ROWS:
        row = {"range": R, "lambda": lam}
        for solver in ("cg", "lbfgs"):
            for name, mode in (("reference", rx.REFERENCE), ("exact", rx.EXACT)):
                psnr, counts = rx.table_solve(inp, R, lam, mode, solver=solver)
                again = [rx.table_solve(inp, R, lam, mode, y=y, solver=solver) for y in moved]
                stable = all(c == counts for _, c in again)
                by = max(abs(psnr - q) for q, _ in again)
                row[solver + "_" + name] = {"psnr": psnr, "counts": counts, "stable": stable, "psnr_moved_by": by}
                print(R, lam, solver, name, "%.3f" % psnr, counts, stable, "%.1e" % by, flush=True)
        out["rows"].append(row)
    with open(os.path.join(HERE, "reg_exact_table.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
