"""Affine registration (srmap_register_affine): where the time goes, next to the translational estimator.
   python tools/affine_registration_timing.py [--size 1024] [--frames 8]
A textured size x size frame and frames - 1 copies rotated by up to 2 degrees about the centre, scaled by up to 1 % and
shifted by up to 6 px (bilinear, zero outside).  Reported, host wall clock around the blocking C calls (min of 5):
  whole call   upload of the stack, pyramids, seed, all Gauss-Newton passes, residual pass; and the passes it took;
  per level    the level's images registered alone (max_levels = 1, started at the converged matrices taken down to that
               level, step_tolerance = 0 so that exactly max_iterations passes run): (time of 21 passes - time of 1) / 20 =
               one pass INCLUDING its table upload, its 26 x (frames - 1) double download and the stream wait;
  bytes        algorithmic bytes of one pass: two f64 images read per frame (the template and the frame), and the rate;
  translational  srmap_register_translational on the same stack.
The kernels' own durations come from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python
tools/affine_registration_timing.py): k_affine_gn_sums' average against the per-pass wall time above says whether the
pass or the per-iteration host round trip dominates.  The figures of profiles/r10_affine_registration.txt."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "super-resolution_amd", "python")):
    sys.path.insert(0, d)
import srmap


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def texture(rng, H, W):
    coarse = rng.random((H // 8 + 2, W // 8 + 2))
    r, c = np.arange(H) / 8.0, np.arange(W) / 8.0
    r0, c0 = r.astype(int), c.astype(int)
    a, b = (c - c0)[None, :], (r - r0)[:, None]
    g = (1 - b) * ((1 - a) * coarse[r0][:, c0] + a * coarse[r0][:, c0 + 1]) + b * ((1 - a) * coarse[r0 + 1][:, c0] + a * coarse[r0 + 1][:, c0 + 1])
    yy, xx = np.mgrid[0:H, 0:W]
    return 0.6 * g + 0.2 + 0.1 * np.sin(0.21 * xx) * np.cos(0.17 * yy)


def rotation(deg, shift, W, H, scale):
    th = np.deg2rad(deg)
    L = scale * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    return np.hstack([L, (c - L @ c + np.asarray(shift, dtype=float))[:, None]])


def warp(img, M):
    """Frame with the content of img at p sitting at M p: bilinear sample of img at M^-1 q, zero outside."""
    H, W = img.shape
    Li = np.linalg.inv(M[:, :2])
    qy, qx = np.mgrid[0:H, 0:W].astype(float)
    sx = Li[0, 0] * (qx - M[0, 2]) + Li[0, 1] * (qy - M[1, 2])
    sy = Li[1, 0] * (qx - M[0, 2]) + Li[1, 1] * (qy - M[1, 2])
    ok = (sx >= 0) & (sx < W - 1) & (sy >= 0) & (sy < H - 1)
    x0, y0 = np.where(ok, np.floor(sx), 0).astype(int), np.where(ok, np.floor(sy), 0).astype(int)
    fx, fy = sx - x0, sy - y0
    v = (1 - fy) * ((1 - fx) * img[y0, x0] + fx * img[y0, x0 + 1]) + fy * ((1 - fx) * img[y0 + 1, x0] + fx * img[y0 + 1, x0 + 1])
    return np.where(ok, v, 0.0)


def down2(a):
    h2, w2 = a.shape[1] // 2, a.shape[2] // 2
    a = a[:, :2 * h2, :2 * w2]
    return 0.25 * ((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + (a[:, 1::2, 0::2] + a[:, 1::2, 1::2]))


def to_coarser(M):
    M = M.copy()
    half = np.array([0.5, 0.5])
    for k in range(len(M)):
        M[k, :, 2] = 0.5 * (M[k, :, 2] - half + M[k, :, :2] @ half)
    return M


def best(fn, n=5):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


N, K = arg("--size", 1024), arg("--frames", 8)
rng = np.random.default_rng(1)
img = texture(rng, N, N)
mats = np.stack([rotation(0, (0, 0), N, N, 1.0)] + [rotation(rng.uniform(-2, 2), rng.uniform(-6, 6, 2), N, N, rng.uniform(0.99, 1.01))
                                                     for _ in range(K - 1)])
stack = np.stack([img] + [warp(img, mats[k]) for k in range(1, K)])
ctx = srmap.Context(0)
got, q = ctx.register_affine(stack, with_quality=True)  # warm-up and the answer
corners = np.array([[0, 0], [N - 1, 0], [0, N - 1], [N - 1, N - 1]], dtype=float)
err = max(np.max(np.hypot(*((corners @ (got[k, :, :2] - mats[k, :, :2]).T) + got[k, :, 2] - mats[k, :, 2]).T)) for k in range(1, K))
print("%d x %d, %d frames (f64): worst corner error %.4f px, passes per frame %s" % (N, N, K, err, q[1:, 3].astype(int).tolist()))
t_all = best(lambda: ctx.register_affine(stack))
t_tr = best(lambda: ctx.register_translational(stack))
print("  whole call %.2f ms (%d passes at most per frame over all levels) | translational estimator %.2f ms" % (
    1e3 * t_all, int(q[1:, 3].max()), 1e3 * t_tr))
level, init, lvl = stack, got.copy(), 0
while True:
    h, w = level.shape[1:]
    lv, ini = level, init
    t1 = best(lambda: ctx.register_affine(lv, init=ini, max_levels=1, max_iterations=1, step_tolerance=0.0))
    t21 = best(lambda: ctx.register_affine(lv, init=ini, max_levels=1, max_iterations=21, step_tolerance=0.0))
    per = (t21 - t1) / 20
    nbytes = (K - 1) * 2 * w * h * 8
    print("  level %d  %4d x %4d: one pass %.1f us, %.2f MB algorithmic, %.3f TB/s | call with 1 pass %.2f ms" % (
        lvl, w, h, 1e6 * per, nbytes / 1e6, nbytes / per / 1e12, 1e3 * t1), flush=True)
    if min(w, h) < 64 or lvl >= 11:
        break
    level, init, lvl = down2(level), to_coarser(init), lvl + 1
