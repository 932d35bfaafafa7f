"""Hold-out validation on the GPU (include/srmap.h: srmap_problem_set_holdout / _get_holdout, srmap_holdout_score*,
srmap_problem_set_regularizer_lambda, srmap_solve_lambda_path; k_holdout_prior and k_holdout_sums in csrc/holdout.hip, the
hold-out's rows of csrc/data_weights.hpp, csrc/lambda_path.hip) against the library itself and against the numpy
restatement (tests/holdout_restatement.py).

Bars.  The mask and its counts: exact.  A problem with a hold-out against its twin whose caller set the prior
m .* (1 - h): bits.  The score against the restatement: 100 x the restatement's own summation-order sensitivity (a permuted
second evaluation) with a floor of 1e-13 relative in f64, 2e-5 in f32; the counts n exact.  The path against the three calls
it is made of: bits.  Every test here fails on the parent commit: none of these entry points exists there."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import holdout_restatement as hr  # noqa: E402
import robust_restatement as rr  # noqa: E402
import test_gpu_data_prior as gdp  # noqa: E402
from test_gpu_data_prior import in_dtype, make_problem, path_flow, product_in_dtype, report_tuple, short_options  # noqa: E402

pytestmark = pytest.mark.gpu

SMALLEST = 2.0 ** -24
FRACTIONS = [SMALLEST, 0.1, 0.5]
# LR sizes whose frame run C h w is one workgroup's worth of 16-byte groups (256 x 2 doubles, 256 x 4 floats) and that +- 1
GROUP_EDGE = [(7, 73), (16, 32), (19, 27), (31, 33), (32, 32), (25, 41)]


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


def tt(dtype):
    import torch
    return torch.float32 if dtype else torch.float64


def device(x, dtype):
    import torch
    t = torch.tensor(np.ascontiguousarray(x), dtype=tt(dtype), device="cuda")
    torch.cuda.synchronize()
    return t


# ------------------------------------------------------------------------------------------------ mask and counts
@pytest.mark.parametrize("KC", [(1, 1), (2, 3), (5, 1)])
@pytest.mark.parametrize("size", [(5, 7), (17, 23), (70, 129)])
def test_mask_and_counts_equal_the_restatement(sr, ctx, size, KC):
    h, w = size
    K, Cn = KC
    rng = np.random.default_rng(h + K)
    y = rng.random((K, Cn, h, w))
    m = rng.random(y.shape)
    for dtype in (0, 1):
        p = make_problem(sr, ctx, "subpixel" if K <= 4 else "direct", h, w, Cn, dtype, y)
        assert p.holdout()[0] == 0.0 and not p.holdout()[2].any() and not p.holdout()[3].any()
        for fraction, seed in zip(FRACTIONS, (1, 2, 2 ** 63 + 5)):
            tag = "%s K%d C%d f%d fraction %g" % (size, K, Cn, 32 if dtype else 64, fraction)
            p.set_holdout(fraction, seed)
            fr_, seed_, mask, counts = p.holdout()
            ref = hr.mask(y.shape, fraction, seed)
            assert fr_ == fraction and seed_ == seed, tag
            assert np.array_equal(mask, ref), tag
            assert counts[0] == ref.sum() and np.array_equal(counts[1:], ref.reshape(K, -1).sum(1)), tag
            assert p.holdout(want_mask=False)[2] is None and np.array_equal(p.holdout(want_mask=False)[3], counts), tag
            # the factor of the prior: ones .* (1 - h), and the caller's prior is still the caller's
            assert p.data_prior() is None and np.array_equal(p.data_weights(), 1.0 - ref), tag
            p.set_data_prior(m)
            assert np.array_equal(p.data_prior(), in_dtype(m, dtype)), tag
            assert np.array_equal(p.data_weights(), in_dtype(m, dtype) * (1.0 - ref)), tag
            p.set_data_prior(None)
            assert p.data_prior() is None and np.array_equal(p.data_weights(), 1.0 - ref), tag
        if size == (70, 129) and K == 5:  # the share at 10 %: within 3 binomial standard deviations
            p.set_holdout(0.1, 1)
            n = y.size
            q = hr.threshold(0.1) / 2.0 ** 24
            assert abs(p.holdout()[3][0] - n * q) <= 3 * np.sqrt(n * q * (1 - q))
        p.set_holdout(0)
        assert p.holdout()[0] == 0.0 and not p.holdout()[2].any()


# ------------------------------------------------------------------------------------------------ the prior twin
def variant(sr, p, name, K, Cn, H, W):
    """A model state beyond the path: applied alike to the problem and its twin."""
    import blur_kernel_restatement as bk
    if name == "blur":
        p.set_blur_kernel(0.6 * bk.anisotropic_psf() + 0.4 * bk.streak_psf(5))
    elif name == "bank":
        p.set_blur_bank(np.stack([bk.gaussian_taps(3, 0.7 + 0.2 * k) for k in range(K)]), sr.BLUR_PER_FRAME)
    elif name == "photometric":
        p.set_photometric(np.stack([np.linspace(0.9, 1.2, K), np.linspace(-0.05, 0.05, K)], axis=1))
    elif name == "lattice":
        import flow_lattice_restatement as fl
        lw, lh = fl.covering_size(W, H, 4)
        p.set_flow_lattice(fl.random_nodes(np.random.default_rng(5), K, lw, lh, 4, [(0.5 * k, -0.75 * k) for k in range(K)]), 4)


def twin_pair(sr, ctx, path, var, h, w, Cn, dtype, y, fraction, seed, m, wts):
    """a: hold-out (and the caller's m, w); b: the caller set the prior m .* (1 - h) itself."""
    K, s = y.shape[0], 2
    a = make_problem(sr, ctx, path, h, w, Cn, dtype, y)
    b = make_problem(sr, ctx, path, h, w, Cn, dtype, y)
    for p in (a, b):
        variant(sr, p, var, K, Cn, h * s, w * s)
        p.set_data_weights(wts)
    keep = 1.0 - hr.mask(y.shape, fraction, seed)
    a.set_data_prior(m)
    a.set_holdout(fraction, seed)
    b.set_data_prior(keep if m is None else np.asarray(m) * keep)
    return a, b


def assert_same_state(tag, sr, ctx, a, b, x, x0, dtype, solves):
    assert a.active_impl() == b.active_impl(), tag
    assert np.array_equal(a.data_weights(), b.data_weights()), tag
    for terms in (sr.TERM_ALL, sr.TERM_DATA):
        fa, ga = a.eval(x, terms)
        fb, gb = b.eval(x, terms)
        assert fa == fb and np.array_equal(ga, gb), tag
    lr = np.asarray(x)[:, ::2, ::2]
    for k in (0, a.K - 1):  # the operators read no weight
        assert np.array_equal(a.apply(x, k), b.apply(x, k)) and np.array_equal(a.apply_transpose(lr, k), b.apply_transpose(lr, k)), (tag, k)
    sa, sb = a.residual_scale(x), b.residual_scale(x)
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]), tag
    for kind in solves:
        o = short_options(sr)
        for p in (a, b):
            p.set_solver(sr.SOLVER_LBFGS if kind == "lbfgs" else sr.SOLVER_CG)
        o.split_channels = 1 if kind == "split" else 0
        xa, ra = a.solve(x0, o)
        xb, rb = b.solve(x0, o)
        assert report_tuple(ra) == report_tuple(rb) and np.array_equal(xa, xb), (tag, kind)
    for p in (a, b):
        p.set_solver(sr.SOLVER_CG)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", [("tile", None), ("subpixel", None), ("direct", None), ("affine", None), ("flow", None),
                                  ("subpixel", "lattice"), ("subpixel", "blur"), ("subpixel", "bank"), ("subpixel", "photometric")],
                         ids=lambda c: "%s-%s" % c)
def test_a_holdout_is_the_prior_its_caller_could_have_set(sr, ctx, case, dtype):
    path, var = case
    h, w, Cn, K, s = 17, 23, 3, 4, 2
    rng = np.random.default_rng(41 + dtype)
    y = rng.random((K, Cn, h, w))
    x, x0 = rng.random((Cn, h * s, w * s)), rng.random((Cn, h * s, w * s))
    m, wts = rng.random(y.shape), 2.0 * rng.random(y.shape)
    m[2] = 0.0
    for name, mm, ww in (("bare", None, None), ("prior", m, None), ("weights", None, wts), ("both", m, wts)):
        tag = "%s %s f%d %s" % (path, var, 32 if dtype else 64, name)
        a, b = twin_pair(sr, ctx, path, var, h, w, Cn, dtype, y, 0.1, 3, mm, ww)
        solves = ("cg", "lbfgs", "split") if name in ("bare", "both") else ()
        assert_same_state(tag, sr, ctx, a, b, x, x0, dtype, solves)
        if name in ("bare", "both"):  # a Huber step, FIXED and MAD, and a Huber solve
            xd = device(x, dtype)
            for mode in (sr.HUBER_DELTA_FIXED, sr.HUBER_DELTA_MAD):
                for p in (a, b):
                    p.set_data_loss(sr.DATA_LOSS_HUBER, 0.2)
                    p.set_huber_scale(mode, 1.345, 1e-4)
                    p.update_data_weights_device(xd.data_ptr())
                ctx.synchronize()
                assert np.array_equal(a.data_weights(), b.data_weights()), (tag, mode)
                assert a.huber_delta()[1] == b.huber_delta()[1] and np.array_equal(a.huber_delta()[3], b.huber_delta()[3]), (tag, mode)
                assert_same_state(tag + " huber", sr, ctx, a, b, x, x0, dtype, ("cg",))


@pytest.mark.parametrize("size", [(5, 7), (70, 129)])
@pytest.mark.parametrize("fraction", [SMALLEST, 0.5])
def test_the_twin_at_the_extreme_fractions_and_sizes(sr, ctx, size, fraction):
    h, w = size
    Cn, K, s = 1, 2, 2
    rng = np.random.default_rng(h)
    y = rng.random((K, Cn, h, w))
    x, x0 = rng.random((Cn, h * s, w * s)), rng.random((Cn, h * s, w * s))
    for dtype in (0, 1):
        a, b = twin_pair(sr, ctx, "subpixel", None, h, w, Cn, dtype, y, fraction, 9, None, None)
        assert_same_state("%s %g f%d" % (size, fraction, 32 if dtype else 64), sr, ctx, a, b, x, x0, dtype, ("cg",))


# ------------------------------------------------------------------------------------------------ persistence, removal
@pytest.mark.parametrize("dtype", [0, 1])
def test_removal_gives_the_bits_from_before_and_frees_everything(sr, ctx, dtype):
    h, w, Cn, K, s = 17, 23, 2, 4, 2
    rng = np.random.default_rng(3)
    y = rng.random((K, Cn, h, w))
    x = rng.random((Cn, h * s, w * s))
    m, wts = rng.random(y.shape), 2.0 * rng.random(y.shape)
    lib = sr.load()
    for name, mm, ww, huber in (("bare", None, None, False), ("prior", m, None, False), ("weights", None, wts, False),
                                ("both", m, wts, False), ("huber", None, None, True), ("huber prior", m, None, True)):
        p = make_problem(sr, ctx, "tile", h, w, Cn, dtype, y)
        p.set_data_prior(mm)
        p.set_data_weights(ww)
        if huber:
            p.set_data_loss(sr.DATA_LOSS_HUBER, 0.1)
        impl0, before, w0 = p.active_impl(), p.eval(x), p.data_weights()
        p.residual_scale(x)  # its buffers are the problem's from here on
        live = lib.srmap_live_allocations()
        p.set_holdout(0.1, 1)
        assert not np.array_equal(p.data_weights(), w0), name
        p.holdout_score(x, 0.0)
        p.set_holdout(0.25, 2)  # a second hold-out replaces the first
        assert np.array_equal(p.holdout()[2], hr.mask(y.shape, 0.25, 2)), name
        p.set_holdout(0)
        assert lib.srmap_live_allocations() == live, name
        after = p.eval(x)
        assert p.active_impl() == impl0 and before[0] == after[0] and np.array_equal(before[1], after[1]), name
        assert np.array_equal(p.data_weights(), w0), name
        assert (p.data_prior() is None) if mm is None else np.array_equal(p.data_prior(), in_dtype(mm, dtype)), name
        p.set_holdout(0)  # lifting nothing is no error


@pytest.mark.parametrize("dtype", [0, 1])
def test_the_holdout_persists_across_the_setters(sr, ctx, dtype):
    h, w, Cn, K, s = 17, 23, 2, 4, 2
    rng = np.random.default_rng(8)
    y, y2 = rng.random((K, Cn, h, w)), rng.random((K, Cn, h, w))
    x = rng.random((Cn, h * s, w * s))
    m, wts = rng.random(y.shape), 2.0 * rng.random(y.shape)
    taps = rng.random((3, 3))
    taps /= taps.sum()
    a, b = twin_pair(sr, ctx, "subpixel", None, h, w, Cn, dtype, y, 0.1, 4, None, None)
    ref = hr.mask(y.shape, 0.1, 4)
    keep = 1.0 - ref
    for step in ("observations", "weights", "prior", "loss", "flow", "blur", "photometric", "affine", "lambda"):
        for p in (a, b):
            if step == "observations":
                p.set_observations(y2)
            elif step == "weights":
                p.set_data_weights(wts)
            elif step == "prior":
                p.set_data_prior(m if p is a else m * keep)
            elif step == "loss":
                p.set_data_loss(sr.DATA_LOSS_HUBER, 0.05)
                p.set_data_loss(sr.DATA_LOSS_L2)
                p.set_data_weights(wts)  # Huber owned the buffer
            elif step == "flow":
                p.set_flow(path_flow(K, h * s, w * s))
            elif step == "blur":
                p.set_blur_kernel(taps)
            elif step == "photometric":
                p.set_photometric(np.stack([np.linspace(0.9, 1.2, K), np.linspace(-0.05, 0.05, K)], axis=1))
            elif step == "affine":
                p.set_affine_motion(np.stack([ar.translation(0.5 * k, -0.25 * k) for k in range(K)]))
            else:
                p.set_regularizer_lambda(0, 0.03)
        fr_, seed_, mask, counts = a.holdout()
        assert (fr_, seed_) == (0.1, 4) and np.array_equal(mask, ref) and counts[0] == ref.sum(), step
        assert np.array_equal(a.data_weights(), b.data_weights()) and np.all(a.data_weights()[ref > 0] == 0), step
        fa, ga = a.eval(x)
        fb, gb = b.eval(x)
        assert fa == fb and np.array_equal(ga, gb), step


# ------------------------------------------------------------------------------------------------ the score
def gpu_residuals(p, x, y_read, dtype):
    """r = A x - y~ from the library's own forward operator, rounded as the residual pass rounds it."""
    K = y_read.shape[0]
    if dtype:
        return np.stack([(p.apply(x, k).astype(np.float32) - y_read[k].astype(np.float32)).astype(np.float64) for k in range(K)])
    return np.stack([p.apply(x, k) - y_read[k] for k in range(K)])


def check_score(tag, got, ref_score, ref_sums, sens, dtype):
    score, sums = got
    bar = np.maximum(100.0 * sens, 1e-13) if dtype == 0 else np.full(sens.shape, 2e-5)
    err = np.abs(score - ref_score) / np.maximum(np.abs(ref_score), 1e-300)
    err[ref_score == 0] = np.abs(score[ref_score == 0])
    print("%s: score %.6e, |GPU - restatement| / score max %.2e (bar %.1e, own sensitivity %.1e)"
          % (tag, score[0], err.max(), bar.min(), sens.max()))
    assert np.all(err <= bar), (tag, err, bar)
    assert np.array_equal(sums[:, 3], ref_sums[:, 3]), tag  # the counts: exact
    rel = np.abs(sums[:, :3] - ref_sums[:, :3]) / np.maximum(np.abs(ref_sums[:, :3]), 1e-300)
    rel[ref_sums[:, :3] == 0] = 0.0
    assert np.all(sums[:, :3][ref_sums[:, :3] == 0] == 0) and rel.max() <= (1e-11 if dtype == 0 else 2e-5), (tag, rel.max())


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", [((5, 7), 1, 1), ((17, 23), 2, 3), ((70, 129), 5, 1)] + [(sz, 2, 1) for sz in GROUP_EDGE],
                         ids=lambda c: "%dx%d-K%d-C%d" % (c[0][0], c[0][1], c[1], c[2]))
def test_score_against_the_restatement(sr, ctx, case, dtype):
    (h, w), K, Cn = case
    s = 2
    rng = np.random.default_rng(h * 7 + K + dtype)
    shifts = gdp.SUB_SHIFTS[:K] if K <= 4 else [[0.25 * k, -0.5 * k] for k in range(K)]
    model = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=3, blur_sigma=1.0)
    gt = rng.random((Cn, h * s, w * s))
    y = np.stack([model.apply(gt, k) for k in range(K)]) + 0.05 * rng.standard_normal((K, Cn, h, w))
    y[rng.random(y.shape) < 0.05] = 1.0  # outliers: the two branches of rho both run
    x = gt + 0.02 * rng.standard_normal(gt.shape)
    m, wts = rng.random(y.shape), 2.0 * rng.random(y.shape)
    m[rng.random(y.shape) < 0.2] = 0.0
    if K > 1:
        m[1] = 0.0  # a frame whose prior is zero everywhere
    p = sr.Problem(ctx, w * s, h * s, Cn, K, s, shifts, 3, 1.0, dtype)
    p.set_observations(y)
    p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
    fraction, seed = (0.5, 6) if h * w < 100 else (0.1, 6)
    p.set_holdout(fraction, seed)
    hmask = hr.mask(y.shape, fraction, seed)
    r = gpu_residuals(p, x, in_dtype(y, dtype), dtype)
    if dtype == 0:  # the library's forward operator against the oracle's: the residuals are the model's
        assert np.max(np.abs(r - rr.residuals(model, y, x))) <= 1e-12
    tag0 = "%dx%d K%d C%d f%d" % (h, w, K, Cn, 32 if dtype else 64)
    np_dtype = np.float32 if dtype else np.float64
    for name, mm, ww in (("none", None, None), ("prior", m, None), ("weights", None, wts), ("both", m, wts)):
        p.set_data_loss(sr.DATA_LOSS_L2)
        p.set_data_weights(ww)
        p.set_data_prior(mm)
        u = hr.base_weight(y.shape, mm, ww, huber=False, dtype=np_dtype)
        for delta in (0.0, 0.04):
            ref = hr.score(r, hmask, u, delta)
            got = p.holdout_score(x, delta)
            check_score("%s L2 %s delta %g" % (tag0, name, delta), got, ref[0], ref[1], hr.score_sensitivity(r, hmask, u, delta), dtype)
            again = p.holdout_score(x, delta)  # the same bits every time, and from a device tensor
            dev = p.holdout_score(device(x, dtype), delta)
            for other in (again, dev):
                assert np.array_equal(got[0], other[0]) and np.array_equal(got[1], other[1]), (tag0, name, delta)
            if mm is not None and K > 1:
                assert got[0][2] == 0.0 and not got[1][2].any()  # the frame without a prior: score 0, n 0
        # "the problem's" delta under L2 is 0
        g0, gn = p.holdout_score(x, 0.0), p.holdout_score(x)
        assert np.array_equal(g0[0], gn[0]) and np.array_equal(g0[1], gn[1])
    # Huber: the base weight is the caller's prior alone, whatever the Huber weights are; the problem's delta is the fixed one
    p.set_data_weights(None)
    p.set_data_prior(m)
    p.set_data_loss(sr.DATA_LOSS_HUBER, 0.04)
    xd = device(x, dtype)
    p.update_data_weights_device(xd.data_ptr())
    ctx.synchronize()
    u = hr.base_weight(y.shape, m, None, huber=True, dtype=np_dtype)
    ref = hr.score(r, hmask, u, 0.04)
    got = p.holdout_score(x)
    check_score(tag0 + " Huber FIXED", got, ref[0], ref[1], hr.score_sensitivity(r, hmask, u, 0.04), dtype)
    same = p.holdout_score(x, 0.04)
    assert np.array_equal(got[0], same[0]) and np.array_equal(got[1], same[1])
    # MAD: the last Huber step's delta, read on the device; without a step the call is refused
    p.set_huber_scale(sr.HUBER_DELTA_MAD, 1.345, 1e-4)
    p.update_data_weights_device(xd.data_ptr())
    ctx.synchronize()
    d = p.huber_delta()[1]
    assert d > 0
    got, same = p.holdout_score(x), p.holdout_score(x, d)
    assert np.array_equal(got[0], same[0]) and np.array_equal(got[1], same[1])
    ref = hr.score(r, hmask, u, d)
    check_score(tag0 + " Huber MAD", got, ref[0], ref[1], hr.score_sensitivity(r, hmask, u, d), dtype)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", [("tile", None), ("direct", None), ("affine", None), ("flow", None), ("subpixel", "lattice"),
                                  ("subpixel", "bank"), ("subpixel", "photometric")], ids=lambda c: "%s-%s" % c)
def test_score_under_every_motion_kind_and_the_photometric_units(sr, ctx, case, dtype):
    path, var = case
    h, w, Cn, K, s = 17, 23, 2, 4, 2
    rng = np.random.default_rng(77)
    y = rng.random((K, Cn, h, w))
    x = rng.random((Cn, h * s, w * s))
    m = rng.random(y.shape)
    p = make_problem(sr, ctx, path, h, w, Cn, dtype, y)
    variant(sr, p, var, K, Cn, h * s, w * s)
    p.set_data_prior(m)
    p.set_holdout(0.1, 11)
    p.set_cost_rows(8, 16)  # the score covers the whole frames whatever the cost rows are
    y_read = in_dtype(y, dtype)
    if var == "photometric":  # the normalised units
        gb = np.stack([np.linspace(0.9, 1.2, K), np.linspace(-0.05, 0.05, K)], axis=1)
        yy = in_dtype(y, dtype).astype(np.float32 if dtype else np.float64)
        y_read = np.stack([((yy[k] - yy.dtype.type(gb[k, 1])) / yy.dtype.type(gb[k, 0])) for k in range(K)]).astype(np.float64)
    r = gpu_residuals(p, x, y_read, dtype)
    hmask = hr.mask(y.shape, 0.1, 11)
    u = hr.base_weight(y.shape, m, None, dtype=np.float32 if dtype else np.float64)
    for delta in (0.0, 0.3):
        ref = hr.score(r, hmask, u, delta)
        check_score("%s %s f%d delta %g" % (path, var, 32 if dtype else 64, delta), p.holdout_score(x, delta), ref[0], ref[1],
                    hr.score_sensitivity(r, hmask, u, delta), dtype)
    # a permuted stack is another input: the mask belongs to the index, not to the frame's content
    perm = [2, 0, 3, 1]
    if path in ("tile", "direct") and var is None:
        q = make_problem(sr, ctx, path, h, w, Cn, dtype, y[perm])
        q.set_data_prior(m)
        q.set_holdout(0.1, 11)
        rq = gpu_residuals(q, x, in_dtype(y[perm], dtype), dtype)
        ref = hr.score(rq, hmask, u, 0.0)
        check_score("%s permuted stack" % path, q.holdout_score(x, 0.0), ref[0], ref[1], hr.score_sensitivity(rq, hmask, u, 0.0), dtype)


# ------------------------------------------------------------------------------------------------ the path
def path_problem(sr, ctx, dtype, loss="l2", Cn=1, seed=5):
    h, w, K, s = 24, 32, 4, 2
    rng = np.random.default_rng(seed)
    model = orc.ImageModel(scale=s, shifts=gdp.SUB_SHIFTS, blur_ksize=3, blur_sigma=1.0)
    gt = rr.prototype_ground_truth(Cn, h * s, w * s)
    y = np.stack([model.apply(gt, k) for k in range(K)]) + 0.03 * rng.standard_normal((K, Cn, h, w))
    if loss != "l2":
        y[rng.random(y.shape) < 0.03] = 1.0
    p = sr.Problem(ctx, w * s, h * s, Cn, K, s, gdp.SUB_SHIFTS, 3, 1.0, dtype)
    p.set_observations(y)
    p.add_regularizer(sr.REG_BTV, 0.08, 2, 0.5)
    if loss != "l2":
        p.set_data_loss(sr.DATA_LOSS_HUBER, 0.05)
    if loss == "mad":
        p.set_huber_scale(sr.HUBER_DELTA_MAD, 1.345, 1e-4)
    x0 = rr.bilinear(y[0], s)
    return p, y, x0, gt


def path_options(sr):
    o = sr.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = 3, 10
    return o


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("loss", ["l2", "fixed", "mad"])
def test_a_path_row_is_its_three_calls_and_the_final_solve_is_a_solve(sr, ctx, loss, dtype):
    p, y, x0, gt = path_problem(sr, ctx, dtype, loss)
    q, _, _, _ = path_problem(sr, ctx, dtype, loss)
    scales = [1.0, 0.25, 0.0625, 0.015625]
    for a in (p, q):
        a.set_holdout(0.1, 2)
    o = path_options(sr)
    x, table, chosen, rep = p.solve_lambda_path(x0, scales, o)
    assert table.shape == (len(scales), sr.LAMBDA_PATH_ROW) and np.array_equal(table[:, 0], scales)
    assert chosen == hr.choose(list(table[:, 1]))
    delta = None
    xs = []
    for j, sc in enumerate(scales):  # by hand
        q.set_regularizer_lambda(0, 0.08 * sc)
        xj, rj = q.solve(x0, o)
        if loss == "mad" and j == 0:
            delta = q.huber_delta()[1]
        d = {"l2": 0.0, "fixed": 0.05, "mad": delta}[loss]
        score, sums = q.holdout_score(xj, d)
        row = [sc, score[0], sums[0, 0], sums[0, 1], sums[0, 2], sums[0, 3], rj.irls_rounds, rj.cg_iterations, rj.evaluations, rj.final_cost, d]
        assert np.array_equal(table[j], np.array(row, dtype=np.float64)), (loss, dtype, j, table[j], row)
        xs.append(xj)
    if loss == "mad":
        assert delta > 0 and np.all(table[:, 10] == delta)
    # on return: the chosen lambdas, the hold-out as it was
    assert p.regularizer_lambda(0) == 0.08 * scales[chosen]
    assert p.holdout()[:2] == (0.1, 2) and np.array_equal(p.holdout()[2], hr.mask(y.shape, 0.1, 2))
    # the final solve: the hold-out lifted, the chosen lambda
    q.set_holdout(0)
    q.set_regularizer_lambda(0, 0.08 * scales[chosen])
    xf, rf = q.solve(x0, o)
    assert np.array_equal(x, xf) and report_tuple(rep) == report_tuple(rf)
    # without it: the chosen row's solution, and the lambdas of the start scaled again from where they stand
    p.set_regularizer_lambda(0, 0.08)
    x2, table2, chosen2, rep2 = p.solve_lambda_path(x0, scales, o, final_solve=False)
    assert chosen2 == chosen and np.array_equal(table2, table) and np.array_equal(x2, xs[chosen])
    assert rep2.evaluations == table[chosen, 8] and rep2.final_cost == table[chosen, 9]


def test_patience_the_choice_and_the_lambdas_after_an_error(sr, ctx):
    p, y, x0, gt = path_problem(sr, ctx, 0)
    p.set_holdout(0.1, 2)
    o = path_options(sr)
    scales = [4.0 * 0.5 ** j for j in range(8)]
    x, full, chosen, _ = p.solve_lambda_path(x0, scales, o, final_solve=False)
    assert len(full) == 8 and chosen == int(np.argmin(full[:, 1]))
    print("scores %s, chosen %d" % (" ".join("%.5e" % v for v in full[:, 1]), chosen))
    for patience in (1, 2):
        p.set_regularizer_lambda(0, 0.08)
        want = next((n for n in range(1, 9) if hr.patience_stop(list(full[:n, 1]), patience)), 8)
        x, table, ch, _ = p.solve_lambda_path(x0, scales, o, patience=patience, final_solve=False)
        assert len(table) == want and np.array_equal(table, full[:want]) and ch == hr.choose(list(table[:, 1])), patience
    # an error: the lambdas of the call's start
    p.set_regularizer_lambda(0, 0.08)
    for bad in ([1.0, 1.0], [0.5, 1.0], [1.0, 0.0], [1.0, -1.0], [np.nan], [], [1.0 / (j + 1) for j in range(33)]):
        with pytest.raises(sr.SrmapError) as e:
            p.solve_lambda_path(x0, bad, o)
        assert e.value.status == sr.EINVAL and "lambda path" in str(e.value), bad
        assert p.regularizer_lambda(0) == 0.08
    with pytest.raises(sr.SrmapError) as e:
        p.solve_lambda_path(x0, [1.0, 0.5], o, patience=-1)
    assert e.value.status == sr.EINVAL and "patience" in str(e.value)
    with pytest.raises(sr.SrmapError) as e:
        p.solve_lambda_path(x0, [1.0, 0.5], o, struct_size=4)
    assert e.value.status == sr.EINVAL and "struct_size" in str(e.value)
    # a held-out set without weight: the score's refusal comes back from row 0, and the lambdas are the start's again
    p.set_data_prior(1.0 - hr.mask(y.shape, 0.1, 2))
    with pytest.raises(sr.SrmapError) as e:
        p.solve_lambda_path(x0, [1.0, 0.5], o)
    assert e.value.status == sr.EINVAL and "nothing is held out" in str(e.value)
    assert p.regularizer_lambda(0) == 0.08 and p.holdout()[:2] == (0.1, 2)


# ------------------------------------------------------------------------------------------------ the pinned table inputs
def _golden_table():
    import json
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "holdout_table.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["sigma 0.01", "sigma 0.03", "sigma 0.003", "salt and pepper"])
def test_the_path_on_the_table_inputs_is_the_restatements(sr, ctx, name):
    """The GPU path (solve, score, choice) against the independent restatement (tests/holdout_restatement.py's lambda_path,
    recorded by tests/golden/make_holdout_table.py and re-measured on the CPU by tests/test_holdout_cpu.py) on the README
    table's inputs, f64: the restatement's chosen row; its counts of held-out pixels; its solve counts (IRLS rounds,
    iterations, evaluations) on the rows whose counts are stable when the observations move by 1e-13; its scores to ten
    times the sensitivity the restatement measured under that move."""
    import test_holdout_cpu as cpu
    g = _golden_table()["inputs"][name]
    P, inputs = cpu._inputs()
    y, delta = inputs[name]
    assert g["scales"] == cpu.SCALES[name] and g["mask_seed"] == cpu.SEEDS[name] and g["huber_delta"] == delta
    kind, _, rng_, decay = P["reg"]
    p = sr.Problem(ctx, P["W"], P["H"], P["C"], P["K"], P["s"], P["shifts"], P["blur"][0], P["blur"][1], sr.F64)
    p.set_observations(y)
    p.add_regularizer(sr.REG_BTV, cpu.LAMBDA, rng_, decay)
    if delta is not None:
        p.set_data_loss(sr.DATA_LOSS_HUBER, delta)
    p.set_holdout(0.1, g["mask_seed"])
    x, table, chosen, _ = p.solve_lambda_path(rr.bilinear(y[0], P["s"]), g["scales"], final_solve=False)
    assert len(table) == len(g["scales"])
    ref, sens = np.array(g["scores"]), np.array(g["sensitivity"])
    err = np.abs(table[:, 1] - ref) / ref
    for j in range(len(table)):
        print("%s lambda %-8g score %.9e (restatement %.9e): |GPU - restatement| / score %.2e, bar %.2e (10 x %.1e); counts %s, "
              "restatement %s%s" % (name, cpu.LAMBDA * g["scales"][j], table[j, 1], ref[j], err[j], 10 * sens[j], sens[j],
                                    [int(v) for v in table[j, 6:9]], g["counts"][j], "" if g["stable"][j] else " (not stable)"))
    print("%s: chosen row %d, restatement %d" % (name, chosen, g["chosen"]))
    assert g["chosen"] == g["chosen_moved"]  # the argmin has room (tests/test_holdout_cpu.py): it holds under the move
    assert chosen == g["chosen"]
    assert np.array_equal(table[:, 5], [row[3] for row in g["sums"]])  # the held-out pixels that count
    for j in range(len(table)):
        if g["stable"][j]:
            assert [int(v) for v in table[j, 6:9]] == g["counts"][j], (name, j)
    assert np.all(err <= 10 * sens), (name, err, 10 * sens)


# ------------------------------------------------------------------------------------------------ statuses
def test_statuses_and_messages(sr, ctx):
    h, w, Cn, K, s = 5, 7, 1, 2, 2
    rng = np.random.default_rng(1)
    y = rng.random((K, Cn, h, w))
    x = rng.random((Cn, h * s, w * s))
    lib = sr.load()
    p = sr.Problem(ctx, w * s, h * s, Cn, K, s, gdp.SUB_SHIFTS[:K], 3, 1.0, 0)

    def refused(call, status, *words):
        with pytest.raises(sr.SrmapError) as e:
            call()
        assert e.value.status == status, str(e.value)
        for word in words:
            assert word in str(e.value), (word, str(e.value))

    for bad in (-0.1, 0.5000001, 1.0, 2.0 ** -25, np.nan, np.inf):
        refused(lambda: p.set_holdout(bad), sr.EINVAL, "hold-out fraction")
        assert p.holdout()[0] == 0.0
    # the lambda setter
    refused(lambda: p.set_regularizer_lambda(0, 0.1), sr.EINVAL, "no regularizer 0")
    refused(lambda: p.regularizer_lambda(0), sr.EINVAL, "no regularizer 0")
    p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
    for bad in (-1e-9, np.nan, np.inf):
        refused(lambda: p.set_regularizer_lambda(0, bad), sr.EINVAL, "finite and >= 0")
        assert p.regularizer_lambda(0) == 0.01
    refused(lambda: p.set_regularizer_lambda(1, 0.1), sr.EINVAL, "no regularizer 1")
    refused(lambda: p.set_regularizer_lambda(-1, 0.1), sr.EINVAL, "no regularizer -1")
    # the score and the path name what is missing
    refused(lambda: p.holdout_score(x, 0.0), sr.EINVAL, "no observations")
    p.set_holdout(0.5, 1)
    refused(lambda: p.holdout_score(x, 0.0), sr.EINVAL, "no observations")
    refused(lambda: p.solve_lambda_path(x, [1.0, 0.5]), sr.EINVAL, "srmap_set_observations")
    p.set_observations(y)
    p.set_holdout(0)
    refused(lambda: p.holdout_score(x, 0.0), sr.EINVAL, "srmap_problem_set_holdout")
    refused(lambda: p.solve_lambda_path(x, [1.0, 0.5]), sr.EINVAL, "srmap_problem_set_holdout")
    p.set_holdout(0.5, 1)
    p.set_regularizer_lambda(0, 0.0)
    refused(lambda: p.solve_lambda_path(x, [1.0, 0.5]), sr.EINVAL, "srmap_add_regularizer")
    p.set_regularizer_lambda(0, 0.01)
    refused(lambda: p.holdout_score(x, np.nan), sr.EINVAL, "delta must be finite")
    refused(lambda: p.holdout_score(x, np.inf), sr.EINVAL, "delta must be finite")
    p.set_data_loss(sr.DATA_LOSS_HUBER, 0.1)
    p.set_huber_scale(sr.HUBER_DELTA_MAD, 1.345, 1e-4)
    refused(lambda: p.holdout_score(x), sr.EINVAL, "no step has run")
    p.holdout_score(x, 0.1)  # an explicit delta needs no step
    xd0 = device(x, 0)
    p.update_data_weights_device(xd0.data_ptr())
    ctx.synchronize()
    p.holdout_score(x)  # a step has run
    p.set_huber_scale(sr.HUBER_DELTA_MAD, 1.345, 1e-4)  # the rule in force set again keeps the record
    p.holdout_score(x)
    p.set_huber_scale(sr.HUBER_DELTA_FIXED)
    p.set_huber_scale(sr.HUBER_DELTA_MAD, 1.345, 1e-4)  # a change of the rule forgets it: no stale delta
    refused(lambda: p.holdout_score(x), sr.EINVAL, "no step has run")
    p.update_data_weights_device(xd0.data_ptr())
    ctx.synchronize()
    p.holdout_score(x)
    p.set_data_loss(sr.DATA_LOSS_L2)
    p.set_data_loss(sr.DATA_LOSS_HUBER, 0.1)  # so does a change of the loss
    refused(lambda: p.holdout_score(x), sr.EINVAL, "no step has run")
    p.set_data_loss(sr.DATA_LOSS_L2)
    # nothing held out: the smallest fraction on 70 observations holds none out
    p.set_holdout(SMALLEST, 1)
    assert p.holdout()[3][0] == 0
    refused(lambda: p.holdout_score(x, 0.0), sr.EINVAL, "nothing is held out")
    # null handles
    assert lib.srmap_problem_set_holdout(None, 0.1, 1) == sr.EINVAL
    assert lib.srmap_problem_get_holdout(None, None, None, None, None) == sr.EINVAL
    assert lib.srmap_holdout_score(None, None, 0.0, None, None) == sr.EINVAL
    assert lib.srmap_holdout_score_device(None, None, None, 0.0, None, None) == sr.EINVAL
    assert lib.srmap_problem_set_regularizer_lambda(None, 0, 0.1) == sr.EINVAL
    assert lib.srmap_problem_get_regularizer_lambda(None, 0, None) == sr.EINVAL
    assert lib.srmap_solve_lambda_path(None, None, None, None, None, None, None, None, None) == sr.EINVAL
    # a sharded evaluation or solve over more than one rank: refused with the hold-out's own message
    p.set_holdout(0.5, 1)

    class NoExchange:
        """A torch.distributed stand-in that records every collective the solve would make."""
        calls = []

        class ReduceOp:
            SUM, MAX = 0, 1

        def all_reduce(self, *a, **k):
            self.calls.append("all_reduce")

        def isend(self, *a, **k):
            self.calls.append("isend")

        def irecv(self, *a, **k):
            self.calls.append("irecv")

    fake = NoExchange()
    comm = sr.Comm(ctx, 0, 2, backend="host", dist=fake)
    xd, gd = device(x, 0), device(x, 0)
    for mode in (sr.SHARD_FRAMES, sr.SHARD_ROWS, sr.SHARD_CHANNELS):
        sd = sr.ShardDesc()
        sd.mode = mode
        sd.own_row0, sd.own_row1, sd.own_ch0, sd.own_ch1 = 0, h * s, 0, 1
        refused(lambda: p.solve(x, comm=comm, shard=sd), sr.EUNSUPPORTED, "a hold-out is not sharded", "run the solve unsharded")
        refused(lambda: p.eval_sharded_device(comm, sd, xd.data_ptr(), gd.data_ptr()), sr.EUNSUPPORTED, "a hold-out is not sharded",
                "evaluate unsharded")
    assert fake.calls == []
    xs, rep = p.solve(x)  # unsharded it solves
    assert np.all(np.isfinite(xs)) and rep.cg_iterations > 0


# ------------------------------------------------------------------------------------------------ the layers above
def test_host_facade_runs_the_path_as_the_calls_it_is_made_of():
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "super-resolution_amd", "lib", "holdout_facade_test")
    assert os.path.exists(exe), "build() makes the facade test binary"
    o = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(o.stdout, o.stderr)
    assert o.returncode == 0 and "HOLDOUT FACADE TESTS PASSED" in o.stdout


def test_the_tool_chooses_lambda_from_the_holdout(tmp_path):
    """generate_data makes a noisy 48 x 64 burst (the ground truth of tests/test_gpu_flow.py's tool run, K = 4, noise sigma
    0.03); super_resolution --holdout_fraction=0.1 --lambda_path=0.32:0.5:6 prints a table of 6 rows, chooses the row with the
    least score, and its result is the run that is given the chosen lambda as --regularization_parameter: the same PSNR
    line.  Without the flags the command line behaves as before (no hold-out line, no table)."""
    import re
    import subprocess
    from conftest import ROOT
    from test_gpu_apps import _write_envi
    libdir = os.path.join(ROOT, "super-resolution_amd", "lib")
    gen, srbin = os.path.join(libdir, "generate_data"), os.path.join(libdir, "super_resolution")
    assert os.path.exists(gen) and os.path.exists(srbin), "build() makes the tools"
    C_, H, W, s, K = 1, 48, 64, 2, 4
    rng = np.random.default_rng(21)
    gt = np.clip(0.8 * rr.prototype_ground_truth(C_, H, W) + 0.1 * rng.random((C_, H, W)), 0, 1).astype(np.float32).astype(np.float64)
    gt_cfg = _write_envi(str(tmp_path / "gt"), gt)
    motion = tmp_path / "motion.txt"
    motion.write_text("".join("%r %r\n" % (float(a), float(b)) for a, b in ar.TABLE_SHIFTS[:K]))
    lr_dir = tmp_path / "lr"
    lr_dir.mkdir()
    out = subprocess.run([gen, "--input_image=" + gt_cfg, "--output_image_dir=" + str(lr_dir), "--motion_sequence_path=" + str(motion),
                          "--blur_radius=3", "--blur_sigma=1.0", "--downsampling_scale=%d" % s, "--number_of_frames=%d" % K,
                          "--noise_sigma=%r" % (0.03 * 255)], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    base = [srbin, "--data_path=" + str(lr_dir), "--ground_truth_image=" + gt_cfg, "--upsampling_scale=%d" % s, "--blur_radius=3",
            "--blur_sigma=1.0", "--motion_sequence_path=" + str(motion), "--regularizer=btv", "--btv_scale_range=2",
            "--optimization_iterations=5", "--solver_iterations=30", "--evaluators=psnr"]

    def run(*flags):
        o = subprocess.run(base + list(flags), capture_output=True, text=True, timeout=600)
        print(o.stdout, o.stderr)
        assert o.returncode == 0
        return o.stdout, [l for l in o.stdout.splitlines() if l.startswith("PSNR score on result")][0]

    text, psnr_line = run("--holdout_fraction=0.1", "--holdout_seed=2", "--lambda_path=0.32:0.5:6", "--print_lambda_path")
    head = re.search(r"Lambda path: 6 of 6 rows, chosen lambda (\S+) \(row (\d), hold-out score (\S+)\)\.", text)
    rows = re.findall(r"^  lambda (\S+): score (\S+) over (\d+) held-out pixels", text, flags=re.M)
    assert head and len(rows) == 6
    lambdas, scores = [float(r[0]) for r in rows], [float(r[1]) for r in rows]
    assert np.allclose(lambdas, [0.32 * 0.5 ** j for j in range(6)], rtol=1e-8)
    chosen = int(head.group(2))
    assert chosen == hr.choose(scores) and float(head.group(1)) == lambdas[chosen] and float(head.group(3)) == scores[chosen]
    assert all(int(r[2]) == int(hr.mask((K, C_, H // s, W // s), 0.1, 2).sum()) for r in rows)
    assert "Hold-out score of the result:" in text
    # the result is the plain run at the chosen lambda, and that run says nothing of a hold-out
    plain, plain_line = run("--regularization_parameter=%r" % (0.32 * 0.5 ** chosen))
    assert plain_line == psnr_line and "Lambda path" not in plain and "Hold-out" not in plain
    # patience stops the table early
    text, _ = run("--holdout_fraction=0.1", "--holdout_seed=2", "--lambda_path=0.32:0.5:6", "--lambda_patience=1", "--print_lambda_path")
    want = next((n for n in range(1, 7) if hr.patience_stop(scores[:n], 1)), 6)
    assert "Lambda path: %d of 6 rows" % want in text
