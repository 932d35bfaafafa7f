"""Dense flow registration (srmap_register_flow): where the time goes, next to the affine registration on the same stack.
   python tools/flow_registration_timing.py [--size 1024] [--frames 8] [--scale 2]
A textured size x size frame and frames - 1 copies deformed by a sub-pixel shift plus a smooth sinusoid of amplitude 1.5 px
(bilinear, zero outside).  Reported, host wall clock around the blocking C calls (min of 5):
  whole call   upload of the stack, pyramids, gradients, all passes, the output field, its copy to the host -- at hr_scale 1
               and at --scale;
  per level    the level's images registered alone (max_levels = 1): (time of 21 passes - time of 1) / 20 = one warp pass
               (k_flow_lk_pass + k_flow_smooth; nothing returns to the host between passes);
  bytes        algorithmic bytes of one pass per frame: I_0, its two gradient planes, I_k and the two planes of u read, two
               planes written, then two read and two written by the box mean = 10 f64 planes, and the rate;
  upsampling   whole call at --scale minus whole call at hr_scale 1: k_flow_resample to the HR grid, k_flow_maxdiff over
               it AND the larger copy of the field to pageable host memory, which dominates;
  affine       srmap_register_affine on the same stack in the same process.
The kernels' own durations come from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python
tools/flow_registration_timing.py).  The figures of profiles/r15_flow_registration.txt."""
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


def field(k, H, W):
    qy, qx = np.mgrid[0:H, 0:W].astype(float)
    j = k % 5
    return np.stack([0.7 * j - 2.0 + 1.5 * np.sin(2 * np.pi * qy / (64.0 + 8 * j) + 0.9 * k),
                     1.1 - 0.4 * j + 1.5 * np.sin(2 * np.pi * qx / (96.0 - 8 * j) + 1.7 * k)])


def warp(img, u):
    """I_k(q) = img(q + u(q)), bilinear, zero where a tap is outside."""
    H, W = img.shape
    qy, qx = np.mgrid[0:H, 0:W].astype(float)
    sx, sy = qx + u[0], qy + u[1]
    ok = (sx >= 0) & (sx < W - 1) & (sy >= 0) & (sy < H - 1)
    x0, y0 = np.where(ok, np.floor(sx), 0).astype(int), np.where(ok, np.floor(sy), 0).astype(int)
    fx, fy = sx - x0, sy - y0
    v = (1 - fy) * ((1 - fx) * img[y0, x0] + fx * img[y0, x0 + 1]) + fy * ((1 - fx) * img[y0 + 1, x0] + fx * img[y0 + 1, x0 + 1])
    return np.where(ok, v, 0.0)


def down2(a):
    h2, w2 = a.shape[1] // 2, a.shape[2] // 2
    a = a[:, :2 * h2, :2 * w2]
    return 0.25 * ((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + (a[:, 1::2, 0::2] + a[:, 1::2, 1::2]))


def best(fn, n=5):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


N, K, S = arg("--size", 1024), arg("--frames", 8), arg("--scale", 2)
rng = np.random.default_rng(1)
img = texture(rng, N, N)
truth = np.stack([np.zeros((2, N, N))] + [field(k, N, N) for k in range(1, K)])
stack = np.stack([img] + [warp(img, truth[k]) for k in range(1, K)])
ctx = srmap.Context(0)
flow, valid, q = ctx.register_flow(stack)  # warm-up and the answer
b = 16
epe = [float(np.mean(np.hypot(flow[k, 0] - truth[k, 0], flow[k, 1] - truth[k, 1])[b:-b, b:-b])) for k in range(1, K)]
print("%d x %d, %d frames (f64): mean endpoint error %.4f px (worst frame %.4f), valid fraction %.3f, largest dx + dy %.3f" % (
    N, N, K, np.mean(epe), max(epe), q[1:, 1].min(), q[:, 2].max()))
t_1 = best(lambda: ctx.register_flow(stack))
t_s = best(lambda: ctx.register_flow(stack, hr_scale=S))
ctx.register_affine(stack)
t_aff = best(lambda: ctx.register_affine(stack))
print("  whole call %.2f ms at hr_scale 1, %.2f ms at hr_scale %d (upsampling, its check and the larger copy: %.2f ms for %.1f MB)" % (
    1e3 * t_1, 1e3 * t_s, S, 1e3 * (t_s - t_1), (K - 1) * 2 * N * N * (S * S - 1) * 8 / 1e6))
print("  affine registration of the same stack %.2f ms: flow / affine = %.2f (hr_scale 1)" % (1e3 * t_aff, t_1 / t_aff))
level, lvl, total = stack, 0, 0.0
while True:
    h, w = level.shape[1:]
    lv = level
    t1 = best(lambda: ctx.register_flow(lv, max_levels=1, warps=1))
    t21 = best(lambda: ctx.register_flow(lv, max_levels=1, warps=21))
    per = (t21 - t1) / 20
    total += 8 * per
    nbytes = (K - 1) * 10 * w * h * 8
    print("  level %d  %4d x %4d: one pass %.1f us, %.2f MB algorithmic, %.3f TB/s | call with 1 pass %.2f ms" % (
        lvl, w, h, 1e6 * per, nbytes / 1e6, nbytes / per / 1e12, 1e3 * t1), flush=True)
    if min(w, h) < 32 or lvl >= 11:
        break
    level, lvl = down2(level), lvl + 1
print("  8 passes at every level: %.2f ms of the whole call's %.2f ms" % (1e3 * total, 1e3 * t_1))
