"""Displacement-field motion model: data-term evaluation times next to the affine kernels, in one process.
   python tools/flow_timing.py            (f64 and f32, both geometries; the figures of profiles/r14_flow.txt)
At bench.py's cfg2 geometry (2048 x 2048, 16 frames, scale 4, blur 3) and at 1024 x 1024, 8 frames, scale 2: the SAME motion
(rotations of up to 2 degrees about the centre plus sub-pixel shifts) once as matrices (the affine instances of k_forward_direct
+ k_gather_sampled) and once as the field u(q) = F^-1(q) - q (their flow instances), alternating, after a warm-up at sustained clocks.
Per problem: the cost-only data evaluation (forward kernel + cost reduction), the data evaluation with its gradient
(+ gather kernel), their difference (the gather), and the whole evaluation with the BTV regulariser.  Algorithmic bytes:
forward = x + observations read, residuals written (+ the field, K * 2 * H * W, for the flow); gather = residuals read,
gradient written (+ the seeds, K * H * W * 4, and the field once, for the flow).  Set time: the whole of
Problem.set_flow(device tensor) -- the copy, k_flow_seed, k_flow_check, the three count reductions and the read-back --
by the host clock.  Device events on one stream otherwise."""
import os, sys, time
import numpy as np, torch
torch.cuda.init(); torch.zeros(1, device="cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "super-resolution_amd", "python")):
    sys.path.insert(0, d)
import srmap

ts = torch.cuda.Stream()
stream = ts.cuda_stream


def warm(fns):
    for fn in fns:
        for _ in range(3): fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()  # sustained clocks first (as bench.py)
    while time.perf_counter() - t0 < 0.2:
        for fn in fns:
            for _ in range(5): fn()
        torch.cuda.synchronize()


def once(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ts)
    for _ in range(n): fn()
    e1.record(ts)
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n  # us


def rotation(deg, shift, W, H):
    th = np.deg2rad(deg)
    L = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    return np.hstack([L, (c - L @ c + np.asarray(shift, dtype=float))[:, None]])


ctx = srmap.Context(0)
for f32 in (False, True):
    dtype, tdt, esz = (srmap.F32, torch.float32, 4) if f32 else (srmap.F64, torch.float64, 8)
    rng = np.random.default_rng(1)
    torch.manual_seed(1)
    for label, W, H, K, s, n in (("cfg2 2048 x 2048, 16 frames, scale 4", 2048, 2048, 16, 4, 40),
                                 ("1024 x 1024, 8 frames, scale 2", 1024, 1024, 8, 2, 100)):
        shifts = [[k % s + np.round(rng.uniform(-.5, .5) * 32) / 32, (k // s) % s + np.round(rng.uniform(-.5, .5) * 32) / 32] for k in range(K)]
        mats = np.stack([rotation(0.0 if k == 0 else rng.uniform(-2, 2), shifts[k], W, H) for k in range(K)])
        field = torch.from_numpy(srmap.flow_from_affine(mats, H, W)).to(tdt).to("cuda").contiguous()
        y = torch.rand((K, 1, H // s, W // s), dtype=tdt, device="cuda")
        x = torch.rand((1, H, W), dtype=tdt, device="cuda")
        g = torch.empty_like(x)
        torch.cuda.synchronize()
        probs, t_set = {}, []
        for name in ("flow", "affine"):
            p = srmap.Problem(ctx, W, H, 1, K, s, shifts, 3, 1.0, dtype)
            if name == "affine":
                p.set_affine_motion(mats)
            else:
                for _ in range(4):
                    t0 = time.perf_counter()
                    p.set_flow(field, stream)
                    t_set.append(1e6 * (time.perf_counter() - t0))
            p.set_observations_device(y.data_ptr(), stream)
            r = p.add_regularizer(srmap.REG_BTV, 0.01, 3, 0.5)
            p.update_irls_weights_device(r, x.data_ptr(), stream)
            probs[name] = p
        kinds = {"forward": lambda p: p.eval_device(x.data_ptr(), None, srmap.TERM_DATA, stream=stream),
                 "forward + gather": lambda p: p.eval_device(x.data_ptr(), g.data_ptr(), srmap.TERM_DATA, stream=stream),
                 "whole (with BTV)": lambda p: p.eval_device(x.data_ptr(), g.data_ptr(), srmap.TERM_ALL, stream=stream)}
        fns = {(pn, kn): (lambda p=p, k=k: k(p)) for pn, p in probs.items() for kn, k in kinds.items()}
        warm(list(fns.values()))
        t = {key: [] for key in fns}
        for _ in range(5):  # alternating: every pass times every (problem, kind) once
            for key, fn in fns.items():
                t[key].append(once(fn, n))
        N, nl = W * H, K * (H // s) * (W // s)
        extra = {"flow": (2 * K * N * esz, K * N * 4 + 2 * K * N * esz), "affine": (0, 0)}
        print("%s, %s" % (label, "f32" if f32 else "f64"))
        res = {}
        for pn in probs:
            b_fwd, b_gat = (N + 2 * nl) * esz + extra[pn][0], (nl + N) * esz + extra[pn][1]
            fw, fg, al = (min(t[(pn, kn)]) for kn in kinds)
            fwx, fgx, alx = (max(t[(pn, kn)]) for kn in kinds)
            ga = fg - fw
            res[pn] = (fw, ga, fg, al)
            print("  %-7s forward %.1f-%.1f us (%.2f MB, %.2f TB/s) | gather (difference) %.1f us (%.2f MB, %.2f TB/s) | "
                  "forward + gather %.1f-%.1f us | whole evaluation with BTV %.1f-%.1f us" % (
                      pn, fw, fwx, b_fwd / 1e6, b_fwd / fw / 1e6, ga, b_gat / 1e6, b_gat / max(ga, 1e-9) / 1e6, fg, fgx, al, alx), flush=True)
        a, d = res["flow"], res["affine"]
        print("  flow / affine: forward %.2f x, gather %.2f x, forward + gather %.2f x, whole %.2f x" % (
            a[0] / d[0], a[1] / d[1], a[2] / d[2], a[3] / d[3]))
        print("  set_flow (copy, seed, check, reductions, read-back; host clock): first %.0f us, then %.0f-%.0f us for %.1f MB of field" % (
            t_set[0], min(t_set[1:]), max(t_set[1:]), 2 * K * N * esz / 1e6), flush=True)
        del probs, fns, field
