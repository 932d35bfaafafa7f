"""Hold-out validation: one score call against a cost-only data evaluation, set_holdout against set_data_prior_device, and
a whole 8-row lambda path against the sum of its rows' solves run by hand.
   python tools/lambda_path_timing.py
One process; host clock around n calls (the score and the setters are complete on return; the evaluation is enqueued and
waited for once), after a warm-up at sustained clocks, the minimum of 5 repetitions.  At cfg2's geometry (2048 x 2048 HR,
16 frames, scale 4) and at 1024 x 1024 / 8 frames / scale 2, f64 and f32, sub-pixel shifts, blur 3.  The yardstick of the
score is a cost-only SRMAP_TERM_DATA evaluation of the same problem in the same run: by bytes the score is that forward pass
plus one LR-sized read stream (two with a prior).  The figures of profiles/r25_lambda_path.txt."""
import os, sys, time
import numpy as np, torch
torch.cuda.init(); torch.zeros(1, device="cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "super-resolution_amd", "python")):
    sys.path.insert(0, d)
import srmap

ts = torch.cuda.Stream()
stream = ts.cuda_stream


def timed(fn, n=50, sync=True):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    tr = time.perf_counter()  # sustained clocks first (as bench.py)
    while time.perf_counter() - tr < 0.1:
        for _ in range(10): fn()
        torch.cuda.synchronize()
    best = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(n): fn()
        if sync: torch.cuda.synchronize()
        best.append(1e6 * (time.perf_counter() - t0) / n)
    return min(best)


rng = np.random.default_rng(1)
torch.manual_seed(1)
ctx = srmap.Context(0)
SCALES = [2.0 ** -j for j in range(8)]
for lr, K, s in ((512, 16, 4), (512, 8, 2)):
    for dtype, tname, tdt in ((srmap.F64, "f64", torch.float64), (srmap.F32, "f32", torch.float32)):
        W = lr * s
        shifts = [[k % s + np.round(rng.uniform(-.5, .5) * 32) / 32, (k // s) % s + np.round(rng.uniform(-.5, .5) * 32) / 32] for k in range(K)]
        p = srmap.Problem(ctx, W, W, 1, K, s, shifts, 3, 1.0, dtype)
        x = torch.rand((1, W, W), dtype=tdt, device="cuda")
        y = torch.rand((K, 1, lr, lr), dtype=tdt, device="cuda")
        prior = (torch.rand((K, 1, lr, lr), device="cuda") < 0.9).to(tdt)
        torch.cuda.synchronize()
        p.set_observations_device(y.data_ptr(), stream)
        lr_mb = y.numel() * y.element_size() / 1e6
        fwd = lambda: p.eval_device(x.data_ptr(), None, srmap.TERM_DATA, stream=stream)
        fwd_wait = lambda: p.eval_device(x.data_ptr(), None, srmap.TERM_DATA, want_cost=True, stream=stream)
        for with_prior in (False, True):
            p.set_holdout(0)
            p.set_data_prior(prior if with_prior else None, stream)
            t_prior = "%.1f us" % timed(lambda: p.set_data_prior(prior, stream), sync=False) if with_prior else "-"
            p.set_holdout(0.1, 1)
            t_set = timed(lambda: p.set_holdout(0.1, 1), sync=False)  # re-forms the factor and the product: complete on return
            t_fwd, t_fwd_wait = timed(fwd), timed(fwd_wait, sync=False)
            t_score = timed(lambda: p.holdout_score(x, 0.0, stream), sync=False)
            t_huber = timed(lambda: p.holdout_score(x, 0.05, stream), sync=False)
            sc, sums = p.holdout_score(x, 0.0, stream)
            print("%s HR %d^2 x %d frames (LR stack %.1f MB), prior %d: score %.1f us (Huber rho %.1f us) | cost-only data evaluation "
                  "%.1f us enqueued, %.1f us waited for | score / waited evaluation %.2f | set_holdout %.1f us, "
                  "set_data_prior_device %s | held out %d, score %.6e"
                  % (tname, W, K, lr_mb, with_prior, t_score, t_huber, t_fwd, t_fwd_wait, t_score / t_fwd_wait, t_set, t_prior,
                     int(sums[0, 3]), sc[0]), flush=True)
        # the path against its rows by hand
        p.set_data_prior(None)
        p.add_regularizer(srmap.REG_BTV, 0.08, 2, 0.5)
        x0 = np.full((1, W, W), 0.5)
        o = srmap.default_irls_options()
        o.max_num_irls_iterations, o.max_num_solver_iterations = 3, 10
        p.solve_lambda_path(x0, SCALES, o, final_solve=False)  # warm-up: code objects, allocations
        best_path, best_hand = None, None
        for _ in range(3):
            p.set_regularizer_lambda(0, 0.08)
            t0 = time.perf_counter()
            _, table, chosen, _ = p.solve_lambda_path(x0, SCALES, o, final_solve=False)
            t_path = time.perf_counter() - t0
            t_hand = 0.0
            for sc_ in SCALES:
                p.set_regularizer_lambda(0, 0.08 * sc_)
                t0 = time.perf_counter()
                xj, rep = p.solve(x0, o)
                t_hand += time.perf_counter() - t0
            best_path = t_path if best_path is None else min(best_path, t_path)
            best_hand = t_hand if best_hand is None else min(best_hand, t_hand)
        print("%s HR %d^2 x %d frames: 8-row path %.2f ms | its 8 solves by hand (host x0 in, host x out) %.2f ms | path - solves "
              "%.2f ms (8 scores, 8 lambda setters, minus 7 uploads and 8 downloads of x) | %d evaluations, chosen row %d"
              % (tname, W, K, 1e3 * best_path, 1e3 * best_hand, 1e3 * (best_path - best_hand), int(table[:, 8].sum()), chosen), flush=True)
        del p
