"""L-BFGS against CG on one GPU: the IRLS solve of the cfg2 class (16 frames, 4x -> 2048^2, blur 3 / 1.0, BTV) in f64 and
f32 and of the cfg3 geometry (16 frames RGB, 4x -> 4096^2, BTV), m = 5, synthetic data of SURVEY.md section 8(d)
(bench.synth_ground_truth, frames from the library's own image model plus 5/255 Gaussian noise, bilinear x0).

    python tools/lbfgs_timing.py                 solves: evaluations and iterations to the IRLS stop, PSNR, loop ms per
                                                 evaluation and per iteration, for both solvers
    python tools/lbfgs_timing.py --passes        per-pass kernel time of k_lbfgs_update / k_lbfgs_direction at a full ring
                                                 (L = m = 5), from `rocprofv3 --kernel-trace --stats` around a child
                                                 process that makes one 60-iteration L-BFGS run per case, and the
                                                 achieved bytes/s from the byte formula below

Bytes per pass (n unknowns, e bytes per element, L live slots, a full ring):
    k_lbfgs_update     reads x, x_k, g, g_k and the L - 1 other slots' s and y, writes s_p and y_p:  (2 L + 4) n e
    k_lbfgs_direction  reads g and L slots' s and y, writes dn:                                      (2 L + 2) n e"""
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "super-resolution_amd", "python"))

M = 5
CASES = {
    "cfg2_f64": dict(W=2048, C=1, K=16, s=4, blur=(3, 1.0), dtype=0),
    "cfg2_f32": dict(W=2048, C=1, K=16, s=4, blur=(3, 1.0), dtype=1),
    "cfg3_f64": dict(W=4096, C=3, K=16, s=4, blur=(0, 0.0), dtype=0),
}


def pass_bytes(kind, n, es, L=M):
    return (2 * L + 4) * n * es if kind == "update" else (2 * L + 2) * n * es


def make_case(srmap, ctx, cf):
    import bench
    W, C, K, s = cf["W"], cf["C"], cf["K"], cf["s"]
    shifts = [[k % s, (k // s) % s] for k in range(K)]
    gt = bench.synth_ground_truth(W, W, C)
    gen = srmap.Problem(ctx, W, W, C, K, s, shifts, cf["blur"][0], cf["blur"][1], srmap.F64)
    rng = np.random.default_rng(777)
    lr = np.stack([gen.apply(gt, k) for k in range(K)])
    lr = lr + (5.0 / 255.0) * rng.standard_normal(lr.shape)
    x0 = np.stack([bench.bilinear_upsample(lr[0, c:c + 1], s)[0] for c in range(C)])
    del gen
    return gt, lr, x0, shifts


def solve(srmap, ctx, cf, lr, x0, shifts, solver):
    W, C, K, s = cf["W"], cf["C"], cf["K"], cf["s"]
    p = srmap.Problem(ctx, W, W, C, K, s, shifts, cf["blur"][0], cf["blur"][1], cf["dtype"])
    p.set_observations(lr)
    p.add_regularizer(srmap.REG_BTV, 0.01, 3, 0.5)
    p.set_solver(solver, M)
    t0 = time.perf_counter()
    x, rep = p.solve(x0)
    return x, rep, time.perf_counter() - t0


def psnr(gt, x):
    mse = np.mean((np.asarray(gt) - np.asarray(x)) ** 2)
    return float(10 * np.log10(1.0 / mse))


def run_solves(names):
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    import srmap
    ctx = srmap.Context(0)
    out = {}
    for name in names:
        cf = CASES[name]
        gt, lr, x0, shifts = make_case(srmap, ctx, cf)
        solve(srmap, ctx, dict(cf, W=256, C=1), lr[:, :1, :64, :64], x0[:1, :256, :256], shifts, srmap.SOLVER_LBFGS)  # warm-up
        rec = {"psnr_x0": psnr(gt, x0)}
        for label, solver in (("cg", srmap.SOLVER_CG), ("lbfgs", srmap.SOLVER_LBFGS)):
            x, rep, wall = solve(srmap, ctx, cf, lr, x0, shifts, solver)
            rec[label] = dict(irls_rounds=rep.irls_rounds, iterations=rep.cg_iterations, evaluations=rep.evaluations,
                              final_cost=rep.final_cost, psnr=psnr(gt, x), loop_ms=rep.loop_seconds * 1e3,
                              ms_per_evaluation=rep.loop_seconds * 1e3 / max(1, rep.evaluations),
                              ms_per_iteration=rep.loop_seconds * 1e3 / max(1, rep.cg_iterations),
                              waits=rep.waits, wall_s=wall)
            print("%-9s %-5s IRLS %2d  its %4d  evals %5d  PSNR %.4f dB (x0 %.4f)  loop %9.2f ms  %.3f ms/eval  %.3f ms/it" % (
                name, label, rep.irls_rounds, rep.cg_iterations, rep.evaluations, rec[label]["psnr"], rec["psnr_x0"],
                rec[label]["loop_ms"], rec[label]["ms_per_evaluation"], rec[label]["ms_per_iteration"]), flush=True)
        out[name] = rec
    return out


def child_passes(names):
    """Runs under rocprofv3: one long L-BFGS run per case (no IRLS re-weighting, no stopping rule but maxits), so that
    the ring fills and the full-ring instances (L = m) are sampled many times at sustained clocks."""
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    import srmap
    ctx = srmap.Context(0)
    for name in names:
        cf = CASES[name]
        gt, lr, x0, shifts = make_case(srmap, ctx, cf)
        W, C, K, s = cf["W"], cf["C"], cf["K"], cf["s"]
        p = srmap.Problem(ctx, W, W, C, K, s, shifts, cf["blur"][0], cf["blur"][1], cf["dtype"])
        p.set_observations(lr)
        p.add_regularizer(srmap.REG_BTV, 0.01, 3, 0.5)
        _, its, nfev, term, _ = p.lbfgs_trace(x0, M, 0.0, 0.0, 0.0, 60)
        print("done", name, its, nfev, term, flush=True)


def run_passes(names):
    out = {}
    for name in names:
        cf = CASES[name]
        with tempfile.TemporaryDirectory() as d:
            cmd = ["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
                   "-d", d, "-o", "kt", "--", sys.executable, os.path.abspath(__file__), "--child", name]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-2000:])
                raise SystemExit("rocprofv3 run failed (%d)" % r.returncode)
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            rows = list(csv.DictReader(open(files[0])))
        n = cf["C"] * cf["W"] * cf["W"]
        es = 8 if cf["dtype"] == 0 else 4
        T = "double" if cf["dtype"] == 0 else "float"
        rec = {}
        for kind in ("update", "direction"):
            pat = re.compile(r"k_lbfgs_%s<%s, ?\d+, ?%d>" % (kind, T, M))
            sel = [r for r in rows if pat.search(r["Name"])]
            if not sel:
                continue
            calls = sum(int(r["Calls"]) for r in sel)
            avg_ns = sum(float(r["TotalDurationNs"]) for r in sel) / calls
            b = pass_bytes(kind, n, es)
            rec[kind] = dict(calls=calls, avg_us=avg_ns / 1e3, bytes=b, tb_per_s=b / avg_ns / 1e3)
            print("%-9s k_lbfgs_%-9s L=%d  %6d calls  %8.1f us  %7.1f MB  %.2f TB/s" % (
                name, kind, M, calls, avg_ns / 1e3, b / 1e6, b / avg_ns / 1e3), flush=True)
        out[name] = rec
    return out


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        child_passes(args[1:])
        return
    passes = "--passes" in args
    names = [a for a in args if a in CASES] or list(CASES)
    res = run_passes(names) if passes else run_solves(names)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
