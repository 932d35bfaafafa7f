"""Robust data term: evaluation and re-weighting times at cfg2 geometry, and the Huber solve on the three small inputs.
   python tools/robust_timing.py [--hr 2048] [--no-solves]
Device events around repeated evaluations on one stream, after a warm-up at sustained clocks (as tools/subpixel_timing.py);
the figures of profiles/r08_robust.txt."""
import os, sys, time
import numpy as np, torch
torch.cuda.init(); torch.zeros(1, device="cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "super-resolution_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)
import srmap

W = int(sys.argv[sys.argv.index("--hr") + 1]) if "--hr" in sys.argv else 2048
s, K = 4, 16
ts = torch.cuda.Stream()  # a stream of its own: the events and every library call go there
stream = ts.cuda_stream


def timed(fn, n=300):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    tr = time.perf_counter()  # sustained clocks first (as bench.py)
    while time.perf_counter() - tr < 0.1:
        for _ in range(10): fn()
        torch.cuda.synchronize()
    best = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ts)
        for _ in range(n): fn()
        e1.record(ts)
        torch.cuda.synchronize()
        best.append(1e3 * e0.elapsed_time(e1) / n)
    return min(best), max(best)


rng = np.random.default_rng(1)
torch.manual_seed(1)
for dtype, tname, tdt in ((srmap.F64, "f64", torch.float64), (srmap.F32, "f32", torch.float32)):
    for name, frac in (("integer", False), ("sub-pixel", True)):
        shifts = [[k % s + (np.round(rng.uniform(-.5, .5) * 32) / 32 if frac else 0),
                   (k // s) % s + (np.round(rng.uniform(-.5, .5) * 32) / 32 if frac else 0)] for k in range(K)]
        ctx = srmap.Context(0)
        p = srmap.Problem(ctx, W, W, 1, K, s, shifts, 3, 1.0, dtype)
        y = torch.rand((K, 1, W // s, W // s), dtype=tdt, device="cuda")
        wts = 2 * torch.rand((K, 1, W // s, W // s), dtype=tdt, device="cuda")
        x = torch.rand((1, W, W), dtype=tdt, device="cuda"); g = torch.empty_like(x)
        torch.cuda.synchronize()
        p.set_observations_device(y.data_ptr(), stream)
        r = p.add_regularizer(srmap.REG_BTV, 0.01, 3, 0.5)
        p.update_irls_weights_device(r, x.data_ptr(), stream)
        ev = lambda: p.eval_device(x.data_ptr(), g.data_ptr(), srmap.TERM_ALL, stream=stream)
        t_plain = timed(ev)
        p.set_data_weights_device(wts.data_ptr(), stream)
        t_w = timed(ev)
        p.set_data_loss(srmap.DATA_LOSS_HUBER, 0.1)
        t_up = timed(lambda: p.update_data_weights_device(x.data_ptr(), stream))
        t_fwd = timed(lambda: p.eval_device(x.data_ptr(), None, srmap.TERM_DATA, stream=stream))
        lr_bytes = y.numel() * y.element_size()
        print("%s %-9s shifts %dx%d: unweighted %.1f-%.1f us | weighted %.1f-%.1f us / evaluation | Huber re-weighting "
              "(forward + k_huber_weights) %.1f-%.1f us, cost-only data evaluation (the forward kernel + the cost reduction) %.1f-%.1f us, "
              "difference %.1f us for %.1f MB read + %.1f MB written" % (
                  tname, name, W, W, t_plain[0], t_plain[1], t_w[0], t_w[1], t_up[0], t_up[1], t_fwd[0], t_fwd[1],
                  t_up[0] - t_fwd[0], lr_bytes / 1e6, lr_bytes / 1e6), flush=True)
        del p, ctx

if "--no-solves" not in sys.argv:
    import oracle as orc
    import robust_restatement as rr
    proto = rr.prototype_inputs()
    ctx = srmap.Context(0)
    print("input            | bilinear | L2 dB (rounds / iterations / evaluations) | Huber 0.02 | Huber 0.05 | Huber 0.02 ms / evaluation")
    for name, y, _ in proto["inputs"]:
        x0 = rr.bilinear(y[0], proto["s"])
        row = []
        for delta in (None, 0.02, 0.05):
            p = srmap.Problem(ctx, proto["W"], proto["H"], 1, proto["K"], proto["s"], proto["shifts"], 3, 1.0, srmap.F64)
            p.set_observations(y)
            p.add_regularizer(*proto["reg"])
            if delta is not None:
                p.set_data_loss(srmap.DATA_LOSS_HUBER, delta)
            p.solve(x0)  # warm-up: code objects, allocations
            x, rep = p.solve(x0)
            row.append((orc.psnr(proto["gt"], x), rep.irls_rounds, rep.cg_iterations, rep.evaluations, 1e3 * rep.loop_seconds / rep.evaluations))
        print("%-16s | %.2f | %.3f (%d / %d / %d) | %.3f (%d / %d / %d) | %.3f (%d / %d / %d) | %.4f" % (
            (name, orc.psnr(proto["gt"], x0)) + row[0][:4] + row[1][:4] + row[2][:4] + (row[1][4],)), flush=True)
