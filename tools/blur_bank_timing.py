"""Blur-kernel bank (srmap_problem_set_blur_bank): what an evaluation costs with a bank, next to the SAME taps as one free-form
kernel (srmap_problem_set_blur_kernel) in the same process -- the yardstick is that free-form evaluation.
   python tools/blur_bank_timing.py
At bench.py's cfg2 geometry (2048 x 2048, scale 4) and at 1024 x 1024 (scale 2), 8 frames with sub-pixel shifts, one
channel, f64 and f32, a 5 x 5 kernel.  Three blurs on one problem: the free-form kernel T, a per-frame bank whose entries all
equal T (the same loads plus one uniform offset: equal time is the expectation, and the results are bit-identical), and a
per-frame bank of different entries.  By device events (min of 5 groups of 20, after a warm-up at sustained clocks):
  cost + gradient   one data evaluation through the direct kernels (k_forward_direct, k_gather_direct, the reduction);
  forward           the cost-only evaluation (k_forward_direct + the reduction);
  gather            their difference: k_gather_direct alone.
And host wall clock (min of 5) around one srmap_fit_blur_bank next to one srmap_fit_blur, apply = 0, ksize 5: the bank fit
launches k_blur_fit_sums over (chunks, frames, channels) and solves K systems instead of one.
The figures of profiles/r17_blur_bank.txt."""
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
    T = psf()
    equal = np.broadcast_to(T, (K, 5, 5)).copy()
    mixed = np.stack([psf(angle=0.4 * k, su=1.0 + 0.1 * k) for k in range(K)])
    for dname, dtype, tdt in (("f64", srmap.F64, torch.float64), ("f32", srmap.F32, torch.float32)):
        p = srmap.Problem(ctx, W, H, 1, K, s, shifts, 5, 1.3, dtype)
        p.set_blur_bank(mixed, srmap.BLUR_PER_FRAME)
        y = np.stack([p.apply(xh, k) for k in range(K)]) + 0.01 * rng.standard_normal((K, 1, H // s, W // s))
        p.set_observations(y)
        x = torch.from_numpy(xh).to(device="cuda", dtype=tdt)
        g = torch.empty_like(x)
        torch.cuda.synchronize()
        fwd = lambda: p.eval_device(x.data_ptr(), None, srmap.TERM_DATA, stream=stream)
        full = lambda: p.eval_device(x.data_ptr(), g.data_ptr(), srmap.TERM_DATA, stream=stream)
        t0 = time.perf_counter()  # sustained clocks first (as bench.py)
        while time.perf_counter() - t0 < 0.2:
            full()
        torch.cuda.synchronize()
        t = {}
        # two rounds, interleaved: the second shows the run-to-run spread of the same measurement
        for rnd in (0, 1):
            for name, setter in (("kernel", lambda: p.set_blur_kernel(T)), ("equal bank", lambda: p.set_blur_bank(equal, srmap.BLUR_PER_FRAME)),
                                 ("mixed bank", lambda: p.set_blur_bank(mixed, srmap.BLUR_PER_FRAME))):
                setter()
                for _ in range(5): full()
                t[name, rnd] = (min(events(full, 20) for _ in range(5)), min(events(fwd, 20) for _ in range(5)))
        print("%s, %d frames, %s, 5 x 5: cost + gradient / forward / gather (difference), us, two rounds" % (label, K, dname))
        for name in ("kernel", "equal bank", "mixed bank"):
            print("  %-10s %s | ratio to the kernel of the same round: %s" % (
                name, "   ".join("%7.1f / %7.1f / %7.1f" % (1e6 * t[name, r][0], 1e6 * t[name, r][1], 1e6 * (t[name, r][0] - t[name, r][1])) for r in (0, 1)),
                "   ".join("%.3f / %.3f" % (t[name, r][0] / t["kernel", r][0], t[name, r][1] / t["kernel", r][1]) for r in (0, 1))), flush=True)
        p.set_blur_kernel(T)
        one = lambda: p.fit_blur(x, ksize=5, apply=False, stream=stream)
        bank = lambda: p.fit_blur_bank(x, srmap.BLUR_PER_FRAME, ksize=5, apply=False, stream=stream)
        for _ in range(2): one(); bank()
        t_one, t_bank = best(one), best(bank)
        status = bank()[1][:, 4]
        print("  fit ksize 5: srmap_fit_blur %.3f ms, srmap_fit_blur_bank (per frame) %.3f ms whole call, ratio %.2f; entries fitted "
              "%d of %d" % (1e3 * t_one, 1e3 * t_bank, t_bank / t_one, int(np.sum(status == 0)), K), flush=True)
        del p
