"""The free-form blur kernel and its calibration fit on the GPU (include/srmap.h: srmap_problem_set_blur_kernel,
srmap_fit_blur; k_blur_fit_sums of csrc/blur_fit.hip, k_fit_reduce of csrc/motion_fit.hip) against the numpy restatement
(tests/blur_kernel_restatement.py), against an existing kernel (the data cost of srmap_eval) and against itself.

Bars.  Evaluations: the project's per-element bars, 1e-12 (f64) and 2e-5 (f32), every comparison through parity_log.  Fit
sums, f64: each block of the Gram (G, b, y.y) is held to 100 x the restatement's own sensitivity to the ORDER of its sums,
floor 1e-13 of the block's largest magnitude (section 3.8's bar); f32: 2e-5 of the block's largest magnitude against the
restatement given the f32-rounded inputs (an f32 affine problem rounds its sample weights to f32).  Taps: 100 x the
restatement's order sensitivity of the taps, floor 1e-10."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as orc

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import blur_kernel_restatement as bk  # noqa: E402
import parity_log as pl  # noqa: E402
import robust_restatement as rr  # noqa: E402
import test_blur_kernel_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu

LIBDIR = os.path.join(ROOT, "super-resolution_amd", "lib")


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


def f32r(a):
    return None if a is None else np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def make_motion(kind, rng, K, W, H):
    """(restatement motion, shifts for the problem or None, affine matrices or None)."""
    if kind == "none":
        return None, None, None
    if kind == "integer":
        sh = [[0, 0], [2, -1], [-3, 1], [1, 4], [-2, -2]][:K]
        return ("shifts", sh), sh, None
    if kind == "subpixel":
        sh = [[0, 0], [1.25, -.75], [-.5, 2.03125], [.40625, .1875], [-1.59375, .5]][:K]
        return ("shifts", sh), sh, None
    mats = np.stack([ar.random_matrix(rng, ar.MAX_DEVIATION, shift=2.0, at_bound=True) if k % 2 else ar.random_matrix(rng, 0.2, shift=2.0)
                     for k in range(K)])
    return ("affine", mats), None, mats


def make_weights(kind, rng, shape):
    if kind is None:
        return None
    if kind == "random":
        return 0.1 + rng.random(shape)
    w = (rng.random(shape) < 0.7).astype(np.float64)
    w[1] = 0.0
    return w


def make_taps(rng, ksize, negative):
    """Asymmetric taps: random, with negative entries when asked; no normalisation."""
    return rng.uniform(-0.5, 1.0, (ksize, ksize)) if negative else rng.random((ksize, ksize)) / ksize


def make_problem(sr, ctx, lr_shape, s, C, K, dtype, shifts, mats, blur=(0, 0.0)):
    h, w = lr_shape
    p = sr.Problem(ctx, w * s, h * s, C, K, s, shifts, blur[0], blur[1], sr.F32 if dtype == "f32" else sr.F64)
    if mats is not None:
        p.set_affine_motion(mats)
    return p


# ------------------------------------------------------------------------------------------- evaluation parity
# LR shape, scale, ksize, negative taps, C, motion, weights, terms, cost-row band
EVAL_CASES = [
    ((5, 7), 2, 7, False, 1, "none", None, "DATA", False),       # the image is narrower than the kernel's reach
    ((7, 5), 2, 7, True, 3, "subpixel", "random", "DATA", False),
    ((7, 5), 3, 5, True, 1, "integer", "mask", "ALL", False),
    ((35, 67), 2, 5, False, 3, "affine", "random", "ALL", False),
    ((35, 67), 4, 3, True, 1, "subpixel", None, "DATA", True),
    ((9, 13), 3, 1, True, 1, "affine", None, "DATA", False),
    ((35, 67), 2, 3, True, 1, "integer", None, "ALL", False),
    ((35, 67), 3, 5, False, 1, "none", "mask", "DATA", True),
]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", EVAL_CASES, ids=lambda c: "%dx%d_s%d_k%d%s_C%d_%s_%s_%s%s" % (c[0] + c[1:3] + ("n" if c[3] else "",) + c[4:8] + ("_band" if c[8] else "",)))
def test_evaluation_matches_the_restatement(sr, ctx, case, dtype):
    (h, w), s, ksize, negative, Cn, mkind, wkind, terms, band = case
    K, H, W = 3, h * s, w * s
    rng = np.random.default_rng(100 * h + w + ksize)
    motion, shifts, mats = make_motion(mkind, rng, K, W, H)
    taps = make_taps(rng, ksize, negative)
    x, y, r = rng.random((Cn, H, W)), rng.random((K, Cn, h, w)), rng.random((Cn, h, w))
    wts = make_weights(wkind, rng, y.shape)
    regw = 0.5 + rng.random(x.shape)
    tol = 1e-12 if dtype == "f64" else 2e-5
    p = make_problem(sr, ctx, (h, w), s, Cn, K, dtype, shifts, mats, blur=(3, 1.0))  # created with another blur size
    p.set_blur_kernel(taps)
    assert p.active_impl() == sr.IMPL_DIRECT and np.array_equal(p.blur_kernel(), taps)
    p.set_observations(y)  # the kernel persists across the observation and weight calls
    if wts is not None:
        p.set_data_weights(wts)
    rows = None
    if band:
        rows = (2 * s, (h - 1) * s)
        p.set_cost_rows(*rows)
    model = bk.BlurKernelModel(s, K, H, W, taps, motion)
    f_ref, g_ref = model.data_term(y, wts, x, cost_rows=rows)
    if terms == "ALL":
        p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
        p.set_irls_weights(0, regw)
        ref = orc.Problem(model, y)
        ref.add_regularizer(orc.REG_BTV, 0.01, 2, 0.6)
        ref.set_irls_weights(0, regw)
        fr, gr = ref.reg_term(0, x)
        f_ref, g_ref = f_ref + fr, g_ref + gr.reshape(g_ref.shape)
    assert np.array_equal(p.blur_kernel(), taps)
    f, g = p.eval(x, terms=sr.TERM_ALL if terms == "ALL" else sr.TERM_DATA)
    ef = pl.note(abs(f - f_ref) / max(1.0, abs(f_ref)), "cost")
    eg = pl.relerr(g, g_ref)
    ea = max(pl.relerr(p.apply(x, k), model.apply(x, k)) for k in range(K))
    et = max(pl.relerr(p.apply_transpose(r, k), model.apply_transpose(r, k)) for k in range(K))
    print("%s %s: cost %.2e gradient %.2e apply %.2e apply_transpose %.2e (bar %.0e)" % (case, dtype, ef, eg, ea, et, tol))
    assert max(ef, eg, ea, et) <= tol


# ------------------------------------------------------------------------------------------- round trips
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("blur", [(3, 1.0), (5, 1.3)])
def test_gaussian_round_trip_is_bit_identical(sr, ctx, blur, dtype):
    s, h, w, K, Cn = 2, 40, 72, 3, 1
    rng = np.random.default_rng(4)
    shifts = [[0, 0], [1.25, -.75], [-.5, 1.5]]
    x, y = rng.random((Cn, h * s, w * s)), rng.random((K, Cn, h, w))
    p = make_problem(sr, ctx, (h, w), s, Cn, K, dtype, shifts, None, blur)
    p.set_observations(y)
    p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
    auto_impl = p.active_impl()
    assert auto_impl == (sr.IMPL_TILED if blur[0] == 3 else sr.IMPL_DIRECT)
    auto = p.eval(x)
    p.set_impl(sr.IMPL_DIRECT)
    direct = p.eval(x)
    gauss = p.blur_kernel()
    assert gauss.shape == (blur[0], blur[0]) and np.max(np.abs(gauss - bk.gaussian_taps(*blur))) <= 1e-16
    p.set_blur_kernel(gauss)  # the Gaussian as a free-form kernel: the same direct evaluation, bit for bit
    custom = p.eval(x)
    assert custom[0] == direct[0] and np.array_equal(custom[1], direct[1])
    p.set_impl(sr.IMPL_AUTO)
    assert p.active_impl() == sr.IMPL_DIRECT
    p.set_blur_kernel(rng.random((7, 7)))
    assert p.blur_kernel().shape == (7, 7)
    p.set_blur_kernel(None)  # restores the created blur and its size: the default evaluation again, the tile family included
    assert p.active_impl() == auto_impl and np.array_equal(p.blur_kernel(), gauss)
    again = p.eval(x)
    assert again[0] == auto[0] and np.array_equal(again[1], auto[1])
    p.set_impl(sr.IMPL_DIRECT)
    again = p.eval(x)
    assert again[0] == direct[0] and np.array_equal(again[1], direct[1])


def test_status_answers(sr, ctx):
    s, h, w, K, Cn = 2, 40, 72, 2, 1
    H, W = h * s, w * s
    rng = np.random.default_rng(8)
    x, y = rng.random((Cn, H, W)), rng.random((K, Cn, h, w))
    p = make_problem(sr, ctx, (h, w), s, Cn, K, "f64", [[0, 0], [1, 1]], None, (3, 1.0))
    p.set_observations(y)
    good = rng.random((5, 5))
    p.set_blur_kernel(good)
    before = p.eval(x)
    nan = good.copy()
    nan[2, 3] = np.nan
    inf = good.copy()
    inf[0, 0] = np.inf
    for taps, status in ((rng.random((9, 9)), sr.EUNSUPPORTED), (rng.random((4, 4)), sr.EINVAL), (nan, sr.EINVAL), (inf, sr.EINVAL)):
        with pytest.raises(sr.SrmapError) as e:
            p.set_blur_kernel(taps)
        assert e.value.status == status
        after = p.eval(x)  # a refused call leaves the problem its blur
        assert np.array_equal(p.blur_kernel(), good) and after[0] == before[0] and np.array_equal(after[1], before[1])
    assert sr.load().srmap_problem_set_blur_kernel(p.handle, 0, good.ctypes.data_as(sr.c_double_p)) == sr.EINVAL
    for kw, status in ((dict(ksize=9), sr.EUNSUPPORTED), (dict(ksize=4), sr.EINVAL), (dict(ridge=-1.0), sr.EINVAL),
                       (dict(ridge=np.nan), sr.EINVAL), (dict(struct_size=8), sr.EINVAL)):
        with pytest.raises(sr.SrmapError) as e:
            p.fit_blur(x, **kw)
        assert e.value.status == status, kw
        assert np.array_equal(p.blur_kernel(), good)
    empty = make_problem(sr, ctx, (h, w), s, Cn, K, "f64", None, None)
    with pytest.raises(sr.SrmapError) as e:
        empty.fit_blur(x)
    assert e.value.status == sr.EINVAL and "no observations" in str(e.value)
    # the tile family does not cover a free-form kernel
    p.set_impl(sr.IMPL_TILED)
    with pytest.raises(sr.SrmapError) as e:
        p.eval(x)
    assert e.value.status == sr.EUNSUPPORTED
    p.set_impl(sr.IMPL_AUTO)
    assert p.active_impl() == sr.IMPL_DIRECT

    # sharded over two ranks: refused before any exchange
    class NoExchange:
        class ReduceOp:
            SUM, MAX = 0, 1
        calls = []

        def all_reduce(self, *a, **k):
            self.calls.append("all_reduce")

        def isend(self, *a, **k):
            self.calls.append("isend")

        def irecv(self, *a, **k):
            self.calls.append("irecv")

    fake = NoExchange()
    comm = sr.Comm(ctx, 0, 2, backend="host", dist=fake)

    def upload(a):
        ptr = C.c_void_p()
        ctx.check(sr.load().srmap_device_alloc(ctx._h, a.size * 8, C.byref(ptr)))
        ctx.check(sr.load().srmap_upload(p.handle, np.ascontiguousarray(a).ctypes.data_as(sr.c_double_p), ptr, a.size))
        return ptr

    xd, gd = upload(x), upload(x)
    for mode in (sr.SHARD_FRAMES, sr.SHARD_ROWS, sr.SHARD_CHANNELS):
        sd = sr.ShardDesc()
        sd.mode = mode
        sd.own_row0, sd.own_row1, sd.own_ch0, sd.own_ch1 = 0, H, 0, 1
        with pytest.raises(sr.SrmapError) as e:
            p.solve(x, comm=comm, shard=sd)
        assert e.value.status == sr.EUNSUPPORTED
        with pytest.raises(sr.SrmapError) as e:
            p.eval_sharded_device(comm, sd, xd.value, gd.value)
        assert e.value.status == sr.EUNSUPPORTED
    assert fake.calls == []
    for ptr in (xd, gd):
        ctx.check(sr.load().srmap_device_free(ctx._h, ptr))
    p.set_blur_kernel(None)  # with the created blur the same sharded call is accepted again as far as the first exchange
    assert p.active_impl() == sr.IMPL_TILED


@pytest.mark.parametrize("solver", ["cg", "lbfgs", "split_channels", "huber"])
def test_solvers_and_refinement_honour_the_kernel(sr, ctx, solver):
    """A short solve with a free-form kernel lowers the cost of the SAME objective the evaluation reports; the traces and
    srmap_refine_motion run."""
    s, h, w, K, Cn = 2, 12, 17, 3, 2
    rng = np.random.default_rng(6)
    motion, shifts, _ = make_motion("subpixel", rng, K, w * s, h * s)
    taps = bk.streak_psf(5)
    gt = rng.random((Cn, h * s, w * s))
    model = bk.BlurKernelModel(s, K, h * s, w * s, taps, motion)
    y = np.stack([model.apply(gt, k) for k in range(K)])
    p = make_problem(sr, ctx, (h, w), s, Cn, K, "f64", shifts, None, (3, 1.0))
    p.set_blur_kernel(taps)
    p.set_observations(y)
    p.add_regularizer(sr.REG_BTV, 0.001, 2, 0.5)
    x0 = rr.bilinear(y[0], s)
    f0, _ = p.eval(x0)
    o = sr.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = 2, 10
    if solver == "lbfgs":
        p.set_solver(sr.SOLVER_LBFGS, 5)
    if solver == "split_channels":
        o.split_channels = 1
    if solver == "huber":
        p.set_data_loss(sr.DATA_LOSS_HUBER, 0.05)
    x, rep = p.solve(x0, o)
    assert np.array_equal(p.blur_kernel(), taps)
    if solver == "huber":
        p.set_data_loss(sr.DATA_LOSS_L2)
        p.set_data_weights(None)
    p.clear_regularizers()
    p.add_regularizer(sr.REG_BTV, 0.001, 2, 0.5)
    f1, _ = p.eval(x)
    ref1, _ = model.data_term(y, None, x, want_grad=False)
    d1, _ = p.eval(x, terms=sr.TERM_DATA, want_grad=False)
    print("%s: cost %.6f -> %.6f in %d evaluations; data cost vs the restatement %.2e" % (solver, f0, f1, rep.evaluations, abs(d1 - ref1) / max(1, ref1)))
    assert f1 < f0 and pl.note(abs(d1 - ref1) / max(1.0, abs(ref1)), "data cost after the solve") <= 1e-12
    if solver == "cg":
        for tr in (p.cg_trace(x0, maxits=3)[4], p.lbfgs_trace(x0, maxits=3)[4]):
            assert abs(tr[0] - f0) <= 1e-12 * f0 and tr[-1] < f0
        mats, q, _ = p.refine_motion(gt, max_iterations=0, apply=False)
        d0, _ = p.eval(gt, terms=sr.TERM_DATA, want_grad=False)
        # the refinement's energy at shifts_xy's affine twin equals the evaluation's where the shifts are multiples of 1/32 px
        assert abs(s * s * np.sum(q[:, 0]) - d0) <= 1e-9 * max(1.0, d0)
        p.set_affine_motion(mats)  # the kernel persists across the motion call
        assert np.array_equal(p.blur_kernel(), taps) and p.active_impl() == sr.IMPL_DIRECT


# ------------------------------------------------------------------------------------------- the fit's sums
# LR shape, scale, ksize, motion, weights, K, C
SUMS_CASES = [
    ((5, 7), 2, 7, "none", None, 2, 1),          # fewer observations than one tile
    ((5, 7), 2, 1, "subpixel", "random", 2, 3),
    ((7, 5), 3, 3, "affine", "mask", 5, 1),
    ((70, 129), 2, 5, "subpixel", "random", 2, 1),  # 71 tiles: the last chunk is half a chunk
    ((70, 129), 2, 3, "affine", None, 5, 3),
    ((70, 129), 2, 7, "none", "mask", 2, 1),
    ((140, 129), 2, 7, "integer", "random", 2, 2),  # 283 tiles: three tiles per chunk, the last chunk one
    ((17, 33), 4, 5, "affine", "random", 5, 3),
]


def sums_bars(x, y, wts, motion, ksize, s, f32):
    """(reference sums, bar per entry) in the packed layout."""
    n = ksize * ksize
    G = {o: bk.gram(x, y, wts, motion, ksize, s, o) for o in (("natural",) if f32 else ("natural", "reversed", "transposed"))}
    ref, bar = G["natural"], np.zeros((n + 1, n + 1))
    for sl in ((slice(0, n), slice(0, n)), (slice(0, n), slice(n, n + 1)), (slice(n, n + 1), slice(n, n + 1))):
        big = np.max(np.abs(ref[sl]))
        if f32:
            bar[sl] = 2e-5 * big
        else:
            sens = max(np.max(np.abs(G[o][sl] - ref[sl])) for o in ("reversed", "transposed"))
            bar[sl] = max(100 * sens, 1e-13 * big)
    return bk.pack(ref), bk.pack(bar)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", SUMS_CASES, ids=lambda c: "%dx%d_s%d_k%d_%s_%s_K%d_C%d" % (c[0] + c[1:]))
def test_fit_sums_match_the_restatement(sr, ctx, case, dtype):
    (h, w), s, ksize, mkind, wkind, K, Cn = case
    H, W = h * s, w * s
    rng = np.random.default_rng(1000 * h + 10 * w + Cn + K)
    motion, shifts, mats = make_motion(mkind, rng, K, W, H)
    x, y = rng.random((Cn, H, W)), rng.random((K, Cn, h, w))
    wts = make_weights(wkind, rng, y.shape)
    f32 = dtype == "f32"
    p = make_problem(sr, ctx, (h, w), s, Cn, K, dtype, shifts, mats, (3, 1.0))
    p.set_observations(y)
    if wts is not None:
        p.set_data_weights(wts)
    taps, q, ne = p.fit_blur(x, ksize=ksize, apply=False)
    again = p.fit_blur(x, ksize=ksize, apply=False)
    assert all(np.array_equal(a, b) for a, b in zip((taps, q, ne), again))  # bit-identical run to run
    if f32:
        x, y, wts = f32r(x), f32r(y), f32r(wts)
    ref, bar = sums_bars(x, y, wts, motion, ksize, s, f32)
    dev = np.abs(ne - ref)
    worst = float(np.max(dev / np.where(bar > 0, bar, 1.0)))
    pl.note(worst, "largest deviation / bar")
    print("%s %s: largest deviation / bar %.3f%s" % (case, dtype, worst, " (within a factor 3 of the f32 bar)" if f32 and worst > 1 / 3 else ""))
    assert np.all(dev <= bar), (int(np.argmax(dev - bar)), dev.max(), bar)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mkind", ["none", "integer", "subpixel", "affine"])
def test_the_energy_at_the_current_kernel_is_the_data_cost_of_eval(sr, ctx, mkind, weighted):
    """An existing kernel as the checker: at f64, s^2 E(kernel in force) from the sums equals srmap_eval's DATA cost."""
    s, (h, w), K, Cn = 2, (24, 33), 3, 2
    rng = np.random.default_rng(12)
    motion, shifts, mats = make_motion(mkind, rng, K, w * s, h * s)
    x, y = rng.random((Cn, h * s, w * s)), rng.random((K, Cn, h, w))
    p = make_problem(sr, ctx, (h, w), s, Cn, K, "f64", shifts, mats, (3, 1.0))
    p.set_observations(y)
    if weighted:
        p.set_data_weights(0.1 + rng.random(y.shape))
    for taps in (None, make_taps(rng, 5, True)):
        if taps is not None:
            p.set_blur_kernel(taps)
        _, q, _ = p.fit_blur(x, apply=False)
        cost, _ = p.eval(x, terms=sr.TERM_DATA, want_grad=False)
        mine = s * s * q[0]
        print("%s weighted %s ksize %d: s^2 E %.15e, eval %.15e, relative difference %.2e"
              % (mkind, weighted, p.blur_kernel().shape[0], mine, cost, abs(mine - cost) / cost))
        assert pl.note(abs(mine - cost) / cost, "s^2 E vs eval") <= 1e-12
        # a larger fit sees the same kernel zero-padded: the same energy
        _, q7, _ = p.fit_blur(x, ksize=7, apply=False)
        assert abs(q7[0] - q[0]) <= 1e-11 * q[0]


# ------------------------------------------------------------------------------------------- whole fits
@pytest.fixture(scope="module")
def table():
    return bk.table_inputs()


@pytest.mark.parametrize("opts", [dict(), dict(sum_to_one=False), dict(ridge=1e-3), dict(ridge=1e-2, sum_to_one=False), dict(ksize=3), dict(ksize=7)],
                         ids=lambda o: "_".join("%s%s" % kv for kv in o.items()) or "defaults")
def test_whole_fit_matches_the_restatement(sr, ctx, table, opts):
    T = table
    gt, _, y = T["scenes"]["calibration"]
    ksize = opts.get("ksize", 5)
    p = make_problem(sr, ctx, (T["H"] // T["s"], T["W"] // T["s"]), T["s"], T["C"], T["K"], "f64", T["shifts"], None, T["guess"])
    p.set_observations(y)
    kw = dict(opts, ksize=ksize)
    taps, q, ne = p.fit_blur(gt, apply=False, **kw)
    cur = bk.gaussian_taps(*T["guess"])
    ref = {o: bk.fit_blur(gt, y, None, T["motion"], ksize, T["s"], cur, kw.get("sum_to_one", True), kw.get("ridge", 0.0), order=o)
           for o in ("natural", "reversed", "transposed")}
    sens = max(np.max(np.abs(ref[o][0] - ref["natural"][0])) for o in ("reversed", "transposed"))
    bar = max(100 * sens, 1e-10)
    dev = float(np.max(np.abs(taps - ref["natural"][0])))
    print("%s: taps GPU - restatement %.2e (bar %.2e), E %.6f -> %.6f (restatement %.6f -> %.6f), pivots %.3e ... %.3e, sum - 1 = %.1e"
          % (kw, dev, bar, q[0], q[1], ref["natural"][1][0], ref["natural"][1][1], q[2], q[3], taps.sum() - 1))
    assert pl.note(dev / bar, "taps deviation / bar") <= 1.0
    assert q[4] == 0 and np.allclose(q[:2], ref["natural"][1][:2], rtol=1e-9, atol=0) and np.allclose(q[2:4], ref["natural"][1][2:4], rtol=1e-5, atol=0)
    if kw.get("sum_to_one", True):
        assert abs(taps.sum() - 1.0) <= 1e-14
    assert q[1] <= q[0] or kw.get("ridge", 0.0) > 0


def test_fit_invariants(sr, ctx, table):
    T = table
    gt, _, y = T["scenes"]["calibration"]
    lr = (T["H"] // T["s"], T["W"] // T["s"])
    p = make_problem(sr, ctx, lr, T["s"], T["C"], T["K"], "f64", T["shifts"], None, T["guess"])
    p.set_observations(y)
    p.add_regularizer(*T["reg"])
    before = p.eval(gt)
    created = p.blur_kernel()
    a = p.fit_blur(gt, ksize=5, apply=False)
    after = p.eval(gt)
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and p.active_impl() == sr.IMPL_TILED  # apply=False: untouched
    # a device tensor of the problem's dtype is the same call
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(gt)).to("cuda")
    torch.cuda.synchronize()
    d = p.fit_blur(xd, ksize=5, apply=False)
    assert all(np.array_equal(u, v) for u, v in zip(a, d))
    # every weight 0: status 3, the kernel stays
    p.set_data_weights(np.zeros_like(y))
    taps, q, ne = p.fit_blur(gt, ksize=5, apply=True)
    assert q[4] == 3 and not ne.any() and np.array_equal(taps, bk.resize_kernel(created, 5))
    assert np.array_equal(p.blur_kernel(), created) and created.shape == (3, 3)
    p.set_data_weights(None)
    # apply=True installs what set_blur_kernel(taps) would
    b = p.fit_blur(gt, ksize=5, apply=True)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and np.array_equal(p.blur_kernel(), a[0]) and p.active_impl() == sr.IMPL_DIRECT
    other = make_problem(sr, ctx, lr, T["s"], T["C"], T["K"], "f64", T["shifts"], None, T["guess"])
    other.set_observations(y)
    other.add_regularizer(*T["reg"])
    other.set_blur_kernel(a[0])
    u, v = p.eval(gt), other.eval(gt)
    assert u[0] == v[0] and np.array_equal(u[1], v[1]) and u[0] < before[0]
    # fitting again from the fitted kernel: E at the start is E at the previous result
    c = p.fit_blur(gt, apply=False)
    assert abs(c[1][0] - a[1][1]) <= 1e-9 * a[1][1] and np.max(np.abs(c[0] - a[0])) <= 1e-9


# ------------------------------------------------------------------------------------------- end to end
def test_calibration_pair_to_fit_to_solve_of_the_second_scene(sr, ctx, table):
    """fit_blur on the calibration pair, then the solve of the SECOND scene with the fitted kernel: the rounds / iterations /
    evaluations the CPU test pins, the PSNR within 0.01 dB of the pinned figure."""
    T = table
    gt, _, y = T["scenes"]["calibration"]
    gt2, _, y2 = T["scenes"]["second"]
    p = make_problem(sr, ctx, (T["H"] // T["s"], T["W"] // T["s"]), T["s"], T["C"], T["K"], "f64", T["shifts"], None, T["guess"])
    p.set_observations(y)
    taps, q, _ = p.fit_blur(gt, ksize=5)
    err = float(np.max(np.abs(taps - T["psf"])))
    print("fitted on the GPU: largest tap error %.4f (pinned %.4f), E %.4f -> %.4f" % (err, cpu.NOISY_TAP_ERROR, q[0], q[1]))
    assert err <= cpu.NOISY_TAP_BAR
    p.set_observations(y2)  # the kernel persists
    p.add_regularizer(*T["reg"])
    o = sr.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = cpu.SOLVE_CAPS
    x, rep = p.solve(rr.bilinear(y2[0], T["s"]), o)
    ps = orc.psnr(gt2, x)
    counts = (rep.irls_rounds, rep.cg_iterations, rep.evaluations)
    pinned = cpu.TABLE["fitted"]["second"]
    print("second scene with the fitted kernel: GPU %.3f dB %s, pinned %.3f dB %s" % (ps, counts, pinned[0], pinned[1]))
    assert counts == pinned[1] and abs(ps - pinned[0]) <= 0.01


def test_cli_blur_kernel_flags(tmp_path):
    """generate_data --blur_kernel_path makes the frames the library makes with that kernel; super_resolution --fit_blur_from
    on those frames, started from the guessed Gaussian, saves a kernel that matches the generating one (up to the float32
    files) and ends above the same run without the fit; the saved file drives a run as --blur_kernel_path."""
    import srmap
    from test_gpu_apps import _read_envi, _write_envi
    gen, srbin = os.path.join(LIBDIR, "generate_data"), os.path.join(LIBDIR, "super_resolution")
    assert os.path.exists(gen) and os.path.exists(srbin), "build() makes the tools"
    C_, H, W, s, K = 1, 48, 64, 2, 4
    rng = np.random.default_rng(21)
    gt = np.clip(rr.prototype_ground_truth(C_, H, W) + 0.1 * rng.random((C_, H, W)), 0, 1).astype(np.float32).astype(np.float64)
    gt_cfg = _write_envi(str(tmp_path / "gt"), gt)
    psf = bk.anisotropic_psf()
    kfile = tmp_path / "psf.txt"
    kfile.write_text("5\n" + "".join(" ".join(repr(float(v)) for v in row) + "\n" for row in psf))
    shifts = [[0, 0], [1.25, .75], [.5, 1], [1, .25]]
    motion = tmp_path / "motion.txt"
    motion.write_text("".join("%r %r\n" % (float(a), float(b)) for a, b in shifts))
    lr_dir = tmp_path / "lr"
    lr_dir.mkdir()
    out = subprocess.run([gen, "--input_image=" + gt_cfg, "--output_image_dir=" + str(lr_dir), "--motion_sequence_path=" + str(motion),
                          "--blur_kernel_path=" + str(kfile), "--downsampling_scale=%d" % s, "--number_of_frames=%d" % K],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    frames = np.stack([_read_envi(str(lr_dir / ("low_res_%d" % i)), (C_, H // s, W // s)) for i in range(K)])
    p = srmap.Problem(srmap.Context(0), W, H, C_, K, s, shifts, 0, 0.0, srmap.F64)
    p.set_blur_kernel(psf)
    for k in range(K):
        assert np.allclose(frames[k], p.apply(gt, k), atol=2e-7)
    base = [srbin, "--data_path=" + str(lr_dir), "--ground_truth_image=" + gt_cfg, "--upsampling_scale=%d" % s,
            "--motion_sequence_path=" + str(motion), "--regularizer=btv", "--btv_scale_range=2", "--regularization_parameter=0.001",
            "--optimization_iterations=5", "--solver_iterations=30", "--evaluators=psnr"]

    def run(*flags):
        o = subprocess.run(base + list(flags), capture_output=True, text=True, timeout=600)
        print(o.stdout, o.stderr)
        assert o.returncode == 0
        return [float(l.split(":")[1]) for l in o.stdout.splitlines() if l.startswith("PSNR score on result")][0], o.stdout

    saved = tmp_path / "fitted.txt"
    ps_guess, _ = run("--blur_radius=3", "--blur_sigma=1.0")
    ps_fit, text = run("--blur_radius=3", "--blur_sigma=1.0", "--fit_blur_from=" + gt_cfg, "--fit_blur_ksize=5",
                       "--save_blur_kernel_path=" + str(saved))
    assert "Fitted a 5 x 5 blur kernel" in text
    vals = [float(v) for v in saved.read_text().split()]
    assert vals[0] == 5 and len(vals) == 26
    err = float(np.max(np.abs(np.array(vals[1:]).reshape(5, 5) - psf)))
    ps_file, _ = run("--blur_kernel_path=" + str(saved))
    print("CLI: %.3f dB with the guessed Gaussian, %.3f dB with --fit_blur_from (largest tap error %.2e), %.3f dB from the saved kernel"
          % (ps_guess, ps_fit, err, ps_file))
    assert err <= 1e-3 and ps_fit > ps_guess + 0.5 and abs(ps_file - ps_fit) <= 1e-6


def test_host_facade_returns_what_the_c_calls_return(tmp_path):
    exe = os.path.join(LIBDIR, "blur_kernel_test")
    assert os.path.exists(exe), "build() makes the facade test binary"
    o = subprocess.run([exe, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(o.stdout, o.stderr)
    assert o.returncode == 0 and "BLUR KERNEL FACADE TESTS PASSED" in o.stdout
