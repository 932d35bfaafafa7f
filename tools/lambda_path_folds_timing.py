"""Cross-validated lambda path: a whole 5-fold, 8-row path against the same 40 solves and 40 scores run by hand from host
arrays, and one set_holdout_fold against one set_holdout.
   python tools/lambda_path_folds_timing.py
One process; host clock (every call timed is complete on return), after a warm-up run of the path, the minimum of 3
repetitions of the path and of the hand-run in alternation; the setters after a warm-up at sustained clocks, the minimum of
5 repetitions of 50 calls, with the spread (max - min) of the five.  At cfg2's geometry (2048 x 2048 HR, 16 frames, scale 4)
and at 1024 x 1024 / 8 frames / scale 2, f64 and f32, sub-pixel shifts, blur 3.  The figures of
profiles/r30_lambda_path_folds.txt."""
import os, sys, time
import numpy as np, torch
torch.cuda.init(); torch.zeros(1, device="cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "super-resolution_amd", "python")):
    sys.path.insert(0, d)
import srmap

ts = torch.cuda.Stream()
stream = ts.cuda_stream


def timed(fn, n=50):
    for _ in range(3): fn()
    tr = time.perf_counter()  # sustained clocks first (as bench.py)
    while time.perf_counter() - tr < 0.1:
        for _ in range(10): fn()
    reps = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(n): fn()
        reps.append(1e6 * (time.perf_counter() - t0) / n)
    return min(reps), max(reps) - min(reps)


rng = np.random.default_rng(1)
torch.manual_seed(1)
ctx = srmap.Context(0)
SCALES = [2.0 ** -j for j in range(8)]
FOLDS, SEED = 5, 1
for lr, K, s in ((512, 16, 4), (512, 8, 2)):
    for dtype, tname, tdt in ((srmap.F64, "f64", torch.float64), (srmap.F32, "f32", torch.float32)):
        W = lr * s
        shifts = [[k % s + np.round(rng.uniform(-.5, .5) * 32) / 32, (k // s) % s + np.round(rng.uniform(-.5, .5) * 32) / 32] for k in range(K)]
        p = srmap.Problem(ctx, W, W, 1, K, s, shifts, 3, 1.0, dtype)
        y = torch.rand((K, 1, lr, lr), dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        p.set_observations_device(y.data_ptr(), stream)
        # the setters: both re-form the factor 1 - h and are complete on return
        p.set_holdout(0.2, SEED)
        t_fr, sp_fr = timed(lambda: p.set_holdout(0.2, SEED))
        p.set_holdout_fold(FOLDS, 2, SEED)
        t_fold, sp_fold = timed(lambda: p.set_holdout_fold(FOLDS, 2, SEED))
        p.set_holdout(0)
        print("%s HR %d^2 x %d frames: set_holdout_fold %.1f us (spread %.1f) | set_holdout %.1f us (spread %.1f)"
              % (tname, W, K, t_fold, sp_fold, t_fr, sp_fr), flush=True)
        # the path against its 40 solves and scores by hand
        p.add_regularizer(srmap.REG_BTV, 0.08, 2, 0.5)
        x0 = np.full((1, W, W), 0.5)
        o = srmap.default_irls_options()
        o.max_num_irls_iterations, o.max_num_solver_iterations = 3, 10
        p.solve_lambda_path_folds(x0, SCALES, folds=FOLDS, seed=SEED, options=o, final_solve=False)  # warm-up: code objects, allocations
        best_path, best_hand = None, None
        for _ in range(3):
            p.set_regularizer_lambda(0, 0.08)
            t0 = time.perf_counter()
            _, table, fold_table, chosen, _ = p.solve_lambda_path_folds(x0, SCALES, folds=FOLDS, seed=SEED, options=o, final_solve=False)
            t_path = time.perf_counter() - t0
            t0 = time.perf_counter()
            hand = np.zeros((len(SCALES), FOLDS))
            for j, sc_ in enumerate(SCALES):
                p.set_regularizer_lambda(0, 0.08 * sc_)
                for f in range(FOLDS):
                    p.set_holdout_fold(FOLDS, f, SEED)
                    xj, rep = p.solve(x0, o)
                    hand[j, f] = p.holdout_score(xj, 0.0)[0][0]
            t_hand = time.perf_counter() - t0
            p.set_holdout(0)
            assert np.array_equal(hand, fold_table[:, :, 1])  # the same bits: the path is these calls
            best_path = t_path if best_path is None else min(best_path, t_path)
            best_hand = t_hand if best_hand is None else min(best_hand, t_hand)
        print("%s HR %d^2 x %d frames: 5-fold 8-row path %.2f ms | its 40 solves and scores by hand (host x0 in, host x out and in) %.2f ms | "
              "path - by hand %.2f ms (39 uploads of x0, 40 downloads and 40 uploads of x not made) | %d evaluations, chosen row %d, least mean at row %d"
              % (tname, W, K, 1e3 * best_path, 1e3 * best_hand, 1e3 * (best_path - best_hand), int(table[:, 9].sum()), chosen,
                 int(np.argmin(table[:, 1]))), flush=True)
        del p
