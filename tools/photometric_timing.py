"""Photometric frame model (srmap_problem_set_photometric, srmap_fit_photometric): what one fit and one normalise pass cost,
next to the forward kernel on the same problem.
   python tools/photometric_timing.py
At bench.py's cfg2 geometry (2048 x 2048, scale 4) and at 1024 x 1024 (scale 2), 8 frames, f64 and f32, with sub-pixel
shifts (k_forward_direct's table kind) and with affine matrices (its affine kind), blur 3 / sigma 1, one process.  Host wall
clock around the blocking call on a device tensor (min of 5, after a warm-up at sustained clocks):
  one fit      the whole call with apply = 0: its allocations, ONE launch of k_photometric_sums, the
               reduce, the copy of K x 6 doubles, the stream wait and the host solve;
  normalise    the whole srmap_problem_set_photometric call on a problem that already holds parameters: the drain, the
               copy of K x 2 doubles, ONE launch of k_photometric_normalise and the stream wait;
  forward      the cost-only data evaluation of the same problem through the direct family (k_forward_direct, table or
               affine kind, + the cost reduction), by device events: the yardstick -- the sums pass issues that kernel's
               loads plus the y / w stream.  The forward kernels are the parent commit's, instance for instance
               (profiles/r13_photometric_resources.txt);
  bytes        algorithmic bytes: a fit reads x once and y (and w, when weights are set) once per frame; a normalise pass
               reads y and writes it once; and the rates over the WHOLE call, which are therefore not kernel rates.
The kernels of a blocking call cannot be timed from outside it: run this script under `rocprofv3 --kernel-trace --stats --
python tools/photometric_timing.py` for the kernels' own averages.  The figures of profiles/r13_photometric.txt."""
import os, sys, time
import numpy as np, torch
torch.cuda.init(); torch.zeros(1, device="cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "super-resolution_amd", "python")):
    sys.path.insert(0, d)
import srmap

ts = torch.cuda.Stream()
stream = ts.cuda_stream


def best(fn, n=5):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out)


def events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ts)
    for _ in range(n): fn()
    e1.record(ts)
    torch.cuda.synchronize()
    return 1e-3 * e0.elapsed_time(e1) / n  # s


def texture(rng, H, W):
    coarse = rng.random((H // 8 + 2, W // 8 + 2))
    r, c = np.arange(H) / 8.0, np.arange(W) / 8.0
    r0, c0 = r.astype(int), c.astype(int)
    a, b = (c - c0)[None, :], (r - r0)[:, None]
    g = (1 - b) * ((1 - a) * coarse[r0][:, c0] + a * coarse[r0][:, c0 + 1]) + b * ((1 - a) * coarse[r0 + 1][:, c0] + a * coarse[r0 + 1][:, c0 + 1])
    yy, xx = np.mgrid[0:H, 0:W]
    return 0.6 * g + 0.2 + 0.1 * np.sin(0.21 * xx) * np.cos(0.17 * yy)


ctx = srmap.Context(0)
K = 8
shifts = [[0, 0], [1.25, .75], [.5, 1], [1, .25], [-.75, 1.5], [.25, -1], [1.5, -.5], [-.25, .75]]
truth = np.stack([[1, 1.08, .94, 1.05, .90, 1.03, 1.1, .97], [0, .03, -.02, .01, .04, -.03, .02, -.01]], axis=1)
for label, W, H, s in (("cfg2 2048 x 2048, scale 4", 2048, 2048, 4), ("1024 x 1024, scale 2", 1024, 1024, 2)):
    rng = np.random.default_rng(1)
    xh = texture(rng, H, W)[None]
    for motion in ("shifts", "affine"):
        for dname, dtype, tdt, esz in (("f64", srmap.F64, torch.float64, 8), ("f32", srmap.F32, torch.float32, 4)):
            p = srmap.Problem(ctx, W, H, 1, K, s, shifts, 3, 1.0, dtype)
            p.set_impl(srmap.IMPL_DIRECT)
            if motion == "affine":
                th = np.deg2rad(np.linspace(-1, 1, K))
                p.set_affine_motion(np.stack([[[np.cos(t), -np.sin(t), sh[0]], [np.sin(t), np.cos(t), sh[1]]] for t, sh in zip(th, shifts)]))
            lr = (K, 1, H // s, W // s)
            y = truth[:, 0].reshape(-1, 1, 1, 1) * np.stack([p.apply(xh, k) for k in range(K)]) + truth[:, 1].reshape(-1, 1, 1, 1) \
                + 0.01 * rng.standard_normal(lr)
            p.set_observations(y)
            x = torch.from_numpy(xh).to(device="cuda", dtype=tdt)
            torch.cuda.synchronize()
            fwd = lambda: p.eval_device(x.data_ptr(), None, srmap.TERM_DATA, stream=stream)
            t0 = time.perf_counter()  # sustained clocks first (as bench.py)
            while time.perf_counter() - t0 < 0.2:
                fwd()
            torch.cuda.synchronize()
            t_fwd = min(events(fwd, 20) for _ in range(5))
            nlr = int(np.prod(lr))
            for weighted in (False, True):
                if weighted:
                    p.set_data_weights(0.5 + rng.random(lr))
                    t_fwd_w = min(events(fwd, 20) for _ in range(5))
                call = lambda: p.fit_photometric(x, gauge_frame=-1, apply=False, stream=stream)
                for _ in range(2): call()
                gb, q, _ = call()
                t_fit = best(call)
                nbytes = (W * H + nlr * (2 if weighted else 1)) * esz
                err = np.abs(gb - truth).max(axis=0)
                print("%s, %d frames, %s, %s, %s: fit %.3f ms whole call (statuses %s, gain / bias error %.1e / %.1e) | algorithmic "
                      "%.1f MB = %.3f TB/s | forward (%s, cost only) %.1f us | fit / forward %.1f x" % (
                          label, K, motion, dname, "weighted" if weighted else "unweighted", 1e3 * t_fit, sorted(set(q[:, 3].astype(int))),
                          err[0], err[1], nbytes / 1e6, nbytes / t_fit / 1e12, "k_forward_direct, affine kind" if motion == "affine" else "k_forward_direct",
                          1e6 * (t_fwd_w if weighted else t_fwd), t_fit / (t_fwd_w if weighted else t_fwd)), flush=True)
            p.set_data_weights(None)
            p.set_photometric(truth)
            norm = lambda: p.set_photometric(truth)
            for _ in range(2): norm()
            t_norm = best(norm)
            nb = 2 * nlr * esz
            print("%s, %d frames, %s, %s: normalise %.3f ms whole call | algorithmic %.1f MB = %.3f TB/s" % (
                label, K, motion, dname, 1e3 * t_norm, nb / 1e6, nb / t_norm / 1e12), flush=True)
            del p
