"""Calibration fit of the blur kernel (srmap_fit_blur): what one fit costs, next to the forward kernel on the same problem.
   python tools/blur_fit_timing.py
At bench.py's cfg2 geometry (2048 x 2048, scale 4) and at 1024 x 1024 (scale 2), 8 frames with sub-pixel shifts, f64 and
f32, ksize 3 / 5 / 7, one process.  x is a texture, the frames are the library's own model of x under a rotated anisotropic
5 x 5 PSF plus sigma 0.01 noise.  Host wall clock around the blocking call on a device tensor (min of 5, after a warm-up at
sustained clocks):
  one fit      the whole call with apply = 0: its allocations, ONE launch of k_blur_fit_sums, the reduce, the copy of P
               doubles, the stream wait and the host solve;
  forward      the cost-only data evaluation of the same problem (k_forward_direct + the cost reduction), by device
               events.  On paper a fit reads x about ksize^2 times per observation through the caches and does
               ksize^4 / 2 f64 multiply-adds per observation in phase 2, so ksize 7 is arithmetic-bound, not a stream;
  bytes        algorithmic bytes of one fit: x once per frame, y once (no weights are set here); and the rate;
  custom 5x5   one cost + gradient evaluation with a free-form 5 x 5 kernel next to the created 5 x 5 Gaussian, both through
               the direct kernels (SRMAP_IMPL_DIRECT): the same code, so the same time.
The kernels of a blocking call cannot be timed from outside it: run this script under `rocprofv3 --kernel-trace --stats --
python tools/blur_fit_timing.py` for k_blur_fit_sums' own average.  The figures of profiles/r12_blur_fit.txt."""
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


def psf(ksize=5, su=1.5, sv=0.7, angle=0.5):
    hb = (ksize - 1) // 2
    yy, xx = np.mgrid[-hb:hb + 1, -hb:hb + 1].astype(float)
    u, v = np.cos(angle) * xx + np.sin(angle) * yy, -np.sin(angle) * xx + np.cos(angle) * yy
    k = np.exp(-0.5 * ((u / su) ** 2 + (v / sv) ** 2))
    return k / k.sum()


ctx = srmap.Context(0)
K = 8
shifts = [[0, 0], [1.25, .75], [.5, 1], [1, .25], [-.75, 1.5], [.25, -1], [1.5, -.5], [-.25, .75]]
for label, W, H, s in (("cfg2 2048 x 2048, scale 4", 2048, 2048, 4), ("1024 x 1024, scale 2", 1024, 1024, 2)):
    rng = np.random.default_rng(1)
    xh = texture(rng, H, W)[None]
    truth = psf()
    for dname, dtype, tdt, esz in (("f64", srmap.F64, torch.float64, 8), ("f32", srmap.F32, torch.float32, 4)):
        p = srmap.Problem(ctx, W, H, 1, K, s, shifts, 5, 1.3, dtype)
        p.set_impl(srmap.IMPL_DIRECT)
        p.set_blur_kernel(truth)
        y = np.stack([p.apply(xh, k) for k in range(K)]) + 0.01 * rng.standard_normal((K, 1, H // s, W // s))
        p.set_observations(y)
        x = torch.from_numpy(xh).to(device="cuda", dtype=tdt)
        g = torch.empty_like(x)
        torch.cuda.synchronize()
        fwd = lambda: p.eval_device(x.data_ptr(), None, srmap.TERM_DATA, stream=stream)
        full = lambda: p.eval_device(x.data_ptr(), g.data_ptr(), srmap.TERM_DATA, stream=stream)
        t0 = time.perf_counter()  # sustained clocks first (as bench.py)
        while time.perf_counter() - t0 < 0.2:
            fwd()
        torch.cuda.synchronize()
        t_fwd_custom = min(events(fwd, 20) for _ in range(5))
        t_full_custom = min(events(full, 20) for _ in range(5))
        p.set_blur_kernel(None)
        t_fwd_gauss = min(events(fwd, 20) for _ in range(5))
        t_full_gauss = min(events(full, 20) for _ in range(5))
        p.set_blur_kernel(truth)
        nbytes = K * (W * H + (H // s) * (W // s)) * esz
        print("%s, %d frames, %s: direct-family data evaluation, free-form 5 x 5 / Gaussian 5 x 5: cost only %.1f / %.1f us, cost + "
              "gradient %.1f / %.1f us" % (label, K, dname, 1e6 * t_fwd_custom, 1e6 * t_fwd_gauss, 1e6 * t_full_custom, 1e6 * t_full_gauss))
        for ksize in (3, 5, 7):
            call = lambda: p.fit_blur(x, ksize=ksize, apply=False, stream=stream)
            for _ in range(2): call()
            taps, q, _ = call()
            t_fit = best(call)
            err = float(np.max(np.abs(taps - truth))) if ksize == 5 else float("nan")
            nobs = K * (H // s) * (W // s)
            flops = nobs * (ksize ** 2 + 1) * (ksize ** 2 + 2)  # one multiply-add per pair and observation, both counted
            print("  fit ksize %d: %.3f ms whole call (status %d, E %.4g -> %.4g, largest tap error %.2e) | algorithmic %.1f MB = "
                  "%.3f TB/s | phase 2 %.2f Gflop = %.2f Tflop/s f64 | fit / forward %.1f x" % (
                      ksize, 1e3 * t_fit, int(q[4]), q[0], q[1], err, nbytes / 1e6, nbytes / t_fit / 1e12, flops / 1e9,
                      flops / t_fit / 1e12, t_fit / t_fwd_custom), flush=True)
        del p
