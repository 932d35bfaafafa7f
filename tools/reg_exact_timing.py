"""The exact regulariser gradient at cfg2's geometry (2048 x 2048 HR, 16 frames, scale 4, blur 3; BTV 3 and BTV 2) and at
1024 x 1024 / 8 frames / scale 2, f64 and f32:
   python tools/reg_exact_timing.py
  (a) the regulariser pass (SRMAP_TERM_REG under SRMAP_IMPL_DIRECT: clear g, values pass, gradient kernel, cost reduction)
      with k_btv_gradient_exact4, with the Exact leg of k_reg_gradient_direct on the SAME input in the same run (x one
      element off the 4-element boundary sends the launcher to the generic leg: reg_gradient_host.hpp), and in the
      reference's mode; the values pass alone (srmap_update_irls_weights_device: k_btv_values_strip at R 3, the streaming
      yardstick).  The passes differ in the gradient kernel only, so their differences are the kernels' differences; the
      gradient kernel itself is bounded from above by pass - values pass (the clear and the reduction stay in).
      Algorithmic bytes of the gradient: x, values, weights, g read and g written.
  (b) a whole evaluation with exact BTV (tiles for the data term + the direct passes) against the reference mode's
      tile-fused evaluation;
  (c) a whole solve from the bilinear start: evaluations x time, exact against reference.
One process; host clock around n enqueued calls waited for once, after a warm-up at sustained clocks, the minimum of 5
repetitions.  Every yardstick is a figure of the same run.  The figures of profiles/r31_reg_exact.txt."""
import os, sys, time
import numpy as np, torch
torch.cuda.init(); torch.zeros(1, device="cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "super-resolution_amd", "python")):
    sys.path.insert(0, d)
import srmap
import bench

ts = torch.cuda.Stream()
stream = ts.cuda_stream


def timed(fn, n=30):
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


def main():
    rng = np.random.default_rng(1)
    torch.manual_seed(1)
    ctx = srmap.Context(0)
    for lr, K, s, R in ((512, 16, 4, 3), (512, 16, 4, 2), (512, 8, 2, 3)):
        for dtype, tname, tdt in ((srmap.F64, "f64", torch.float64), (srmap.F32, "f32", torch.float32)):
            W = lr * s
            n = W * W
            es = 8 if dtype == srmap.F64 else 4
            shifts = [[k % s, (k // s) % s] for k in range(K)]
            gt = torch.rand((1, W, W), dtype=tdt, device="cuda")
            buf = torch.empty(n + 4, dtype=tdt, device="cuda")   # x twice: on the 4-element boundary and one element off it
            x = buf[:n].view(1, W, W); x.copy_(gt)
            buf2 = torch.empty(n + 4, dtype=tdt, device="cuda")
            x_off = buf2[1:n + 1].view(1, W, W); x_off.copy_(gt)
            g = torch.empty((1, W, W), dtype=tdt, device="cuda")
            y = torch.rand((K, 1, lr, lr), dtype=tdt, device="cuda")
            torch.cuda.synchronize()
            assert x.data_ptr() % (4 * es) == 0 and x_off.data_ptr() % (4 * es) != 0 and g.data_ptr() % (4 * es) == 0
            tag = "%s HR %d^2 x %d frames, scale %d, BTV %d" % (tname, W, K, s, R)

            def problem(mode, impl):
                p = srmap.Problem(ctx, W, W, 1, K, s, shifts, 3, 1.0, dtype)
                p.set_observations_device(y.data_ptr(), stream)
                p.add_regularizer(srmap.REG_BTV, 0.01, R, 0.5)
                p.update_irls_weights_device(0, x.data_ptr(), stream)   # weights present, as in a solve
                p.set_regularizer_gradient(0, mode)
                p.set_impl(impl)
                return p

            # (a) the regulariser pass
            pe, pr = problem(srmap.REG_GRADIENT_EXACT, srmap.IMPL_DIRECT), problem(srmap.REG_GRADIENT_REFERENCE, srmap.IMPL_DIRECT)
            t_fast = timed(lambda: pe.eval_device(x.data_ptr(), g.data_ptr(), srmap.TERM_REG, stream=stream))
            g_fast = g.clone()
            t_gen = timed(lambda: pe.eval_device(x_off.data_ptr(), g.data_ptr(), srmap.TERM_REG, stream=stream))
            torch.cuda.synchronize()
            same = bool(torch.equal(g_fast, g))
            t_ref = timed(lambda: pr.eval_device(x.data_ptr(), g.data_ptr(), srmap.TERM_REG, stream=stream))
            t_val = timed(lambda: pe.update_irls_weights_device(0, x.data_ptr(), stream))
            gb = 5 * n * es / 1e9
            print("%s (a) regulariser pass: exact4 %.1f us | generic exact leg %.1f us | reference mode %.1f us | values pass alone "
                  "%.1f us (%.2f TB/s of x read + values written) | exact4 - generic %.1f us | gradient kernel <= pass - values: exact4 "
                  "%.1f us (>= %.2f TB/s of %.1f MB), generic %.1f us (>= %.2f TB/s) | the two legs give %s bits"
                  % (tag, t_fast, t_gen, t_ref, t_val, 2 * n * es / 1e9 / (t_val * 1e-6) / 1e3, t_fast - t_gen, t_fast - t_val,
                     gb / ((t_fast - t_val) * 1e-6) / 1e3, gb * 1e3, t_gen - t_val, gb / ((t_gen - t_val) * 1e-6) / 1e3,
                     "the same" if same else "different"), flush=True)
            del pe, pr
            # (b) a whole evaluation
            pe, pr = problem(srmap.REG_GRADIENT_EXACT, srmap.IMPL_AUTO), problem(srmap.REG_GRADIENT_REFERENCE, srmap.IMPL_AUTO)
            t_e = timed(lambda: pe.eval_device(x.data_ptr(), g.data_ptr(), srmap.TERM_ALL, stream=stream))
            t_r = timed(lambda: pr.eval_device(x.data_ptr(), g.data_ptr(), srmap.TERM_ALL, stream=stream))
            print("%s (b) evaluation: exact (impl %d: tiles + direct passes) %.1f us | reference (impl %d: tile-fused) %.1f us | ratio %.2f"
                  % (tag, pe.active_impl(), t_e, pr.active_impl(), t_r, t_e / t_r), flush=True)
            # (c) a whole solve on a scene: smooth ground truth, the frames through the model's own forward operator + noise
            v, u = np.meshgrid(np.linspace(0, 1, W), np.linspace(0, 1, W), indexing="ij")
            scene = (0.5 + 0.25 * np.sin(2 * np.pi * 2 * u) * np.cos(2 * np.pi * 3 * v) + 0.2 * ((u - .5) ** 2 + (v - .5) ** 2 < .08))[None]
            frames = np.stack([pr.apply(scene, k) for k in range(K)]) + 0.01 * rng.standard_normal((K, 1, lr, lr))
            x0 = bench.bilinear_upsample(frames[0], s)
            res = {}
            for name, p in (("reference", pr), ("exact", pe)):
                p.set_observations(frames)
                p.set_irls_weights(0, None)
                p.solve(x0)  # warm-up: code objects, allocations
                best, rep, xs = None, None, None
                for _ in range(2):
                    p.set_irls_weights(0, None)
                    t0 = time.perf_counter()
                    xs, rep = p.solve(x0)
                    dt = time.perf_counter() - t0
                    best = dt if best is None else min(best, dt)
                mse = float(np.mean((xs - scene) ** 2))
                res[name] = (best, rep.evaluations, 10 * np.log10(1.0 / mse))
            print("%s (c) solve: reference %.1f ms = %d evaluations x %.1f us, %.2f dB | exact %.1f ms = %d evaluations x %.1f us, %.2f dB | "
                  "exact / reference: time %.2f, evaluations %.2f"
                  % (tag, 1e3 * res["reference"][0], res["reference"][1], 1e6 * res["reference"][0] / res["reference"][1], res["reference"][2],
                     1e3 * res["exact"][0], res["exact"][1], 1e6 * res["exact"][0] / res["exact"][1], res["exact"][2],
                     res["exact"][0] / res["reference"][0], res["exact"][1] / res["reference"][1]), flush=True)
            del pe, pr


if __name__ == "__main__":
    main()
