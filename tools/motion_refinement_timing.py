"""Joint motion refinement (srmap_refine_motion): what a pass and a whole call cost, next to the affine forward kernel alone.
   python tools/motion_refinement_timing.py
At bench.py's cfg2 geometry (2048 x 2048, scale 4, blur 3) and at 1024 x 1024 (scale 2, blur 3), 8 frames, f64 and f32, one
process.  x is a texture, the frames are the library's own affine model of x (rotations of up to 2 degrees about the centre
plus sub-pixel shifts) plus sigma 0.01 noise, the start is 0.3 px off.  Host wall clock around the blocking calls on device
tensors (min of 5, after a warm-up at sustained clocks):
  one pass     (call with max_iterations = 20 and step_tolerance = 0 - call with max_iterations = 0) / 20 when every frame
               runs all 20 trial passes; a pass INCLUDES its table upload, its K x 28 double download and the stream wait;
  whole call   default options from the 0.3 px start, and the passes it took;
  forward      the cost-only data evaluation of the same problem and matrices (k_forward_direct, affine kind, + the cost reduction), by
               device events: about 2 x this is what a pass should cost on paper (the same loads plus y / w, about twice
               the f64 arithmetic);
  bytes        algorithmic bytes of one pass per frame: x once, y (and w when weighted) once; and the rate over all frames;
  host share   the part of a pass's wall time that is not kernel time.  The kernels of a blocking call cannot be timed from
               outside it: run this script under `rocprofv3 --kernel-trace --stats -- python
               tools/motion_refinement_timing.py` and hold k_refine_sums' average against the pass's wall time here.
               Without a trace the script reports the bound 1 - 2 x forward / pass (the pass kernel at its paper cost).
The figures of profiles/r11_motion_refinement.txt."""
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


def rotation(deg, shift, W, H):
    th = np.deg2rad(deg)
    L = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    return np.hstack([L, (c - L @ c + np.asarray(shift, dtype=float))[:, None]])


ctx = srmap.Context(0)
K = 8
for label, W, H, s in (("cfg2 2048 x 2048, scale 4", 2048, 2048, 4), ("1024 x 1024, scale 2", 1024, 1024, 2)):
    rng = np.random.default_rng(1)
    xh = texture(rng, H, W)[None]
    truth = np.stack([rotation(0.0 if k == 0 else rng.uniform(-2, 2), (0, 0) if k == 0 else rng.uniform(-2, 2, 2), W, H) for k in range(K)])
    start = truth.copy()
    start[1:, :, 2] += np.array([0.3, -0.2])
    for dname, dtype, tdt, esz in (("f64", srmap.F64, torch.float64, 8), ("f32", srmap.F32, torch.float32, 4)):
        p = srmap.Problem(ctx, W, H, 1, K, s, None, 3, 1.0, dtype)
        p.set_affine_motion(truth)
        y = np.stack([p.apply(xh, k) for k in range(K)]) + 0.01 * rng.standard_normal((K, 1, H // s, W // s))
        p.set_observations(y)
        p.set_affine_motion(start)
        x = torch.from_numpy(xh).to(device="cuda", dtype=tdt)
        torch.cuda.synchronize()
        call = lambda **kw: p.refine_motion(x, apply=False, stream=stream, **kw)
        fwd = lambda: p.eval_device(x.data_ptr(), None, srmap.TERM_DATA, stream=stream)
        for _ in range(3): call(max_iterations=0); fwd()
        t0 = time.perf_counter()  # sustained clocks first (as bench.py)
        while time.perf_counter() - t0 < 0.2:
            call(max_iterations=0)
        got, q, _ = call()
        t_whole = best(call)
        t0p = best(lambda: call(max_iterations=0))
        q20 = call(max_iterations=20, step_tolerance=0.0)[1]
        t20 = best(lambda: call(max_iterations=20, step_tolerance=0.0))
        ran = q20[1:, 2] - 1  # trial passes per frame; the lockstep runs max(ran) passes
        per = (t20 - t0p) / max(1.0, ran.max())
        t_fwd = min(events(fwd, 20) for _ in range(5))
        nbytes = (W * H + (H // s) * (W // s)) * esz
        corners = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], dtype=float)
        err = max(np.max(np.hypot(*((corners @ (got[k, :, :2] - truth[k, :, :2]).T) + got[k, :, 2] - truth[k, :, 2]).T)) for k in range(1, K))
        print("%s, %d frames, %s: whole call %.2f ms (passes per frame %s, status %s, worst corner error %.4f px)" % (
            label, K, dname, 1e3 * t_whole, q[1:, 2].astype(int).tolist(), q[1:, 3].astype(int).tolist(), err))
        print("  one pass %.1f us over %d frames still active at most (trial passes per frame in the 20-pass call: %s); call with the "
              "initial pass only %.2f ms" % (1e6 * per, K - 1, ran.astype(int).tolist(), 1e3 * t0p))
        print("  algorithmic bytes per frame and pass %.2f MB; all %d frames: %.3f TB/s | forward alone (k_forward_direct, affine kind, + cost "
              "reduction, %d frames) %.1f us = %.3f TB/s | pass / forward %.2f x | host share at least %.0f %% if the pass kernel "
              "costs 2 x forward" % (nbytes / 1e6, K - 1, (K - 1) * nbytes / per / 1e12, K, 1e6 * t_fwd, K * nbytes / t_fwd / 1e12,
                                     per / t_fwd, 100 * max(0.0, 1 - 2 * t_fwd * (K - 1) / K / per)), flush=True)
        del p
