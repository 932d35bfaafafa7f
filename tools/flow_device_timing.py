"""Flow registration of a problem's frames: the route through the host against the two device-resident routes.
   python tools/flow_device_timing.py [--size 512] [--frames 16] [--scale 4]
A textured size x size frame and frames - 1 copies deformed by a sub-pixel shift plus a smooth sinusoid of amplitude 0.4 px,
all cut from a larger canvas (tools/flow_registration_timing.py's texture), set as the observations of a one-channel problem of each dtype.
Three routes in one process, host wall clock around a synchronise, min of 5:
  1. host     srmap_register_flow from pageable host doubles, then srmap_problem_set_flow of the field it returns and
              srmap_set_data_weights of the masks -- the route of the parent commit;
  2. device   srmap_register_flow_device on a device copy of the stack into device buffers (no install: what a caller that
              keeps the field on the device pays for the estimate);
  3. problem  srmap_problem_register_flow: the plane from the problem's observation buffer, the field installed as the
              motion, the masks as the data prior; also without the prior, and srmap_problem_set_flow_device of a
              field that is already on the device alone (the seed and domain check the install pays for).
The yardstick of routes 2 and 3 is route 1 in the same run.  The figures of profiles/r16_flow_device.txt."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "super-resolution_amd", "python")):
    sys.path.insert(0, d)
import torch
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
    return np.stack([0.3 * j - 0.6 + 0.4 * np.sin(2 * np.pi * qy / (64.0 + 8 * j) + 0.9 * k),
                     0.5 - 0.2 * j + 0.4 * np.sin(2 * np.pi * qx / (96.0 - 8 * j) + 1.7 * k)])


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


def best(fn, n=5):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts)


n, K, S = arg("--size", 512), arg("--frames", 16), arg("--scale", 4)
rng = np.random.default_rng(1)
pad = 16  # frames cut from a larger canvas: no black border, whose estimate the flow model refuses
canvas = texture(rng, n + 2 * pad, n + 2 * pad)
stack = np.stack([canvas] + [warp(canvas, field(k, n + 2 * pad, n + 2 * pad)) for k in range(1, K)])[:, pad:-pad, pad:-pad]
ctx = srmap.Context(0)
print("LR %d x %d, %d frames, scale %d (HR %d x %d)" % (n, n, K, S, n * S, n * S))
for dtype, name, tt in ((srmap.F64, "f64", torch.float64), (srmap.F32, "f32", torch.float32)):
    p = srmap.Problem(ctx, n * S, n * S, 1, K, S, None, 3, 1.0, dtype)
    p.set_observations(stack[:, None])
    plane = np.ascontiguousarray(stack.astype(np.float32 if dtype == srmap.F32 else np.float64).astype(np.float64))

    def host_route():
        flow, valid, q = ctx.register_flow(plane, hr_scale=S)
        p.set_flow(flow)
        p.set_data_weights(valid[:, None])
        return q

    dev_in = torch.tensor(plane, device="cuda")
    dev_flow = torch.empty((K, 2, n * S, n * S), dtype=torch.float64, device="cuda")
    dev_valid = torch.empty((K, n, n), dtype=torch.float64, device="cuda")
    q1 = host_route()
    q2 = ctx.register_flow(dev_in, hr_scale=S, flow_out=dev_flow, valid_out=dev_valid)
    p.set_data_weights(None)
    q3 = p.register_flow()
    assert np.array_equal(q1, q2) and np.array_equal(q1, q3), "the three routes register the same doubles"
    t_reg = best(lambda: ctx.register_flow(plane, hr_scale=S))
    t1 = best(host_route)
    p.set_data_weights(None)
    t2 = best(lambda: ctx.register_flow(dev_in, hr_scale=S, flow_out=dev_flow, valid_out=dev_valid))
    t3 = best(lambda: p.register_flow())
    t3n = best(lambda: p.register_flow(prior=False))
    field_dev = dev_flow.to(tt)
    t_set = best(lambda: p.set_flow(field_dev))
    print("  %s  1. host route %.2f ms (srmap_register_flow alone %.2f ms) | 2. register_flow_device %.2f ms (%.1fx) | "
          "3. problem_register_flow %.2f ms (%.1fx; without the prior %.2f ms; set_flow of a device field alone %.2f ms); "
          "largest dx + dy %.3f"
          % (name, 1e3 * t1, 1e3 * t_reg, 1e3 * t2, t1 / t2, 1e3 * t3, t1 / t3, 1e3 * t3n, 1e3 * t_set, q1[:, 2].max()), flush=True)
