"""Residual scale: the Huber re-weighting step with a fixed delta and in the MAD scale mode, the select on its own, and a
whole Huber solve in both modes.
   python tools/residual_scale_timing.py [--no-solves]
One process; host clock around n enqueued calls and one synchronisation, after a warm-up at sustained clocks, the minimum
of 5 repetitions.  At cfg2's LR geometry (512 x 512, 16 frames, scale 4) and at 1024 x 1024 / 8 frames / scale 2, f64 and
f32, sub-pixel shifts, blur 3.  The select has no entry point of its own that does not also run the forward pass and
wait for the host, so "select alone" is the MAD step minus the fixed step of the same run, not a measurement in isolation.
The figures of profiles/r23_residual_scale.txt."""
import os, sys, time
import numpy as np, torch
torch.cuda.init(); torch.zeros(1, device="cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "super-resolution_amd", "python")):
    sys.path.insert(0, d)
import srmap

ts = torch.cuda.Stream()
stream = ts.cuda_stream


def timed(fn, n=100):
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
        torch.cuda.synchronize()
        best.append(1e6 * (time.perf_counter() - t0) / n)
    return min(best)


rng = np.random.default_rng(1)
torch.manual_seed(1)
ctx = srmap.Context(0)
for lr, K, s in ((512, 16, 4), (1024, 8, 2)):
    for dtype, tname, tdt in ((srmap.F64, "f64", torch.float64), (srmap.F32, "f32", torch.float32)):
        W = lr * s
        shifts = [[k % s + np.round(rng.uniform(-.5, .5) * 32) / 32, (k // s) % s + np.round(rng.uniform(-.5, .5) * 32) / 32] for k in range(K)]
        p = srmap.Problem(ctx, W, W, 1, K, s, shifts, 3, 1.0, dtype)
        x = torch.rand((1, W, W), dtype=tdt, device="cuda")
        y = torch.rand((K, 1, lr, lr), dtype=tdt, device="cuda")
        prior = (torch.rand((K, 1, lr, lr), device="cuda") < 0.9).to(tdt)
        torch.cuda.synchronize()
        p.set_observations_device(y.data_ptr(), stream)
        p.set_data_loss(srmap.DATA_LOSS_HUBER, 0.1)
        step = lambda: p.update_data_weights_device(x.data_ptr(), stream)
        fwd = lambda: p.eval_device(x.data_ptr(), None, srmap.TERM_DATA, stream=stream)
        lr_bytes = y.numel() * y.element_size()
        passes = 3 if dtype == srmap.F32 else 6
        for with_prior in (False, True):
            p.set_data_prior(prior if with_prior else None, stream)
            p.set_huber_scale(srmap.HUBER_DELTA_FIXED, 0.0, 0.0)
            t_fixed, t_fwd = timed(step), timed(fwd)
            p.set_huber_scale(srmap.HUBER_DELTA_MAD, 1.345, 1e-4)
            t_mad = timed(step)
            mode, delta, scales, counts = p.huber_delta()
            t_sel = t_mad - t_fixed
            sel_bytes = passes * lr_bytes * (2 if with_prior else 1)
            w_bytes = lr_bytes * (3 if with_prior else 2)
            # (a cost-only data evaluation is no yardstick for the forward half of the step: it carries its cost reduction)
            print("%s LR %d^2 x %d frames, prior %d: fixed step %.1f us (cost-only data evaluation %.1f us; weight pass %.1f MB) "
                  "| MAD step %.1f us | select alone (the difference: %d launches) %.1f us for %.1f MB algorithmic = %.2f "
                  "TB/s | MAD step / fixed step %.2f (select / weight pass by bytes, on paper: %.1f) | delta %.6f, n %d" % (
                      tname, lr, K, with_prior, t_fixed, t_fwd, w_bytes / 1e6, t_mad, 2 * passes + 1, t_sel, sel_bytes / 1e6,
                      sel_bytes / t_sel / 1e6, t_mad / t_fixed, sel_bytes / w_bytes, delta, int(counts[0])), flush=True)
        p.set_data_prior(None)
        if "--no-solves" not in sys.argv:
            p.add_regularizer(srmap.REG_BTV, 0.005, 2, 0.5)
            x0 = np.full((1, W, W), 0.5)
            o = srmap.default_irls_options()
            o.max_num_irls_iterations, o.max_num_solver_iterations = 5, 20
            for name, mode in (("fixed 0.1", srmap.HUBER_DELTA_FIXED), ("MAD", srmap.HUBER_DELTA_MAD)):
                p.set_huber_scale(mode, 1.345, 1e-4)
                p.solve(x0, o)  # warm-up: code objects, allocations
                best = None
                for _ in range(5):
                    _, rep = p.solve(x0, o)
                    ms = 1e3 * rep.loop_seconds / rep.evaluations
                    best = ms if best is None else min(best, ms)
                print("%s LR %d^2 x %d frames: Huber solve, delta %-9s %d rounds / %d iterations / %d evaluations, %.4f ms / "
                      "evaluation (loop time, min of 5)" % (tname, lr, K, name, rep.irls_rounds, rep.cg_iterations,
                                                            rep.evaluations, best), flush=True)
        del p
