"""The affine per-frame motion model on the GPU (include/srmap.h: srmap_problem_set_affine_motion; the affine
instances of k_forward_direct and k_gather_sampled, csrc/kernels_data_direct.hip) against its numpy restatement (tests/affine_restatement.py: explicit triplets,
the literal transpose), against the translational direct kernels where the two definitions coincide, and against itself.

Bars: cost and every gradient element relative to max(1, |ref|), 1e-12 in f64 and 2e-5 in f32 (the project's bars).  Test
images stay <= 320 px wide: one ulp in every source coordinate moves the restatement's gradient by 4e-14 (158 x 62) to
8e-14 (316 x 124) relative, half the f64 bar at 2048 x 512.  The kernels form the coordinates by the restatement's own
expression, every operation rounded on its own, so the two hold the same weights; what is left is summation order."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as orc
import parity_log

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import robust_restatement as rr  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = {0: 1e-12, 1: 2e-5}
# multiples of 1/32 px off the rounding ties: the exact-coordinate warp equals warpAffine's quantised one (test_affine_cpu.py)
ANCHOR_SHIFTS = [(1.25, .75), (-.40625, 2.15625), (3, -2), (0, 0), (1, 0), (-2, 3)]


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


def _upload(sr, ctx, p, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    ptr = C.c_void_p()
    ctx.check(sr.load().srmap_device_alloc(ctx._h, a.size * 8, C.byref(ptr)))
    ctx.check(sr.load().srmap_upload(p.handle, a.ctypes.data_as(sr.c_double_p), ptr, a.size))
    return ptr


def _free(sr, ctx, ptr):
    ctx.check(sr.load().srmap_device_free(ctx._h, ptr))


def _check(tag, f, g, f_ref, g_ref, bar):
    ef = parity_log.note(abs(f - f_ref) / max(1.0, abs(f_ref)), tag + " cost")
    eg = parity_log.relerr(g, g_ref)
    print("%s: cost %.3e gradient %.3e (bar %.0e)" % (tag, ef, eg, bar))
    assert ef <= bar and eg <= bar, (tag, ef, eg)


def _matrices(rng, W, H):
    """Identity, a sub-pixel and an integer translation, two random matrices AT the domain bound, one inside it, a
    5-degree rotation about the centre with 3 % of scale, and one whose translation leaves part of the frame empty."""
    far = ar.random_matrix(rng, 0.2)
    far[:, 2] = (0.4 * W, -0.3 * H)
    return np.stack([ar.translation(0, 0), ar.translation(1.3, -0.45), ar.translation(-2, 1),
                     ar.random_matrix(rng, ar.MAX_DEVIATION, at_bound=True), ar.random_matrix(rng, ar.MAX_DEVIATION, at_bound=True),
                     ar.random_matrix(rng, 0.1), ar.rotation_about_centre(5.0, (0.7, -1.6), W, H, 1.03), far])


def _geometry(scale, blur, Cn):
    """Ragged sizes (no multiple of 64 LR cells or of the 256-thread workgroups), <= 320 px wide."""
    rng = np.random.default_rng(1000 * scale + 100 * blur + Cn)
    w, h = 60 + scale + Cn, 23 + scale
    W, H = w * scale, h * scale
    mats = _matrices(rng, W, H)
    K = len(mats)
    y = rng.random((K, Cn, h, w))
    x = rng.random((Cn, H, W))
    regw = 0.5 + rng.random(x.shape)
    return rng, K, w, h, W, H, mats, y, x, regw


def _problem(sr, ctx, W, H, Cn, K, scale, blur, dtype, mats, shifts=None):
    p = sr.Problem(ctx, W, H, Cn, K, scale, shifts, blur, 1.0 if blur else 0.0, dtype)
    if mats is not None:
        p.set_affine_motion(mats)
    return p


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("blur", [0, 3, 5])
@pytest.mark.parametrize("scale", [2, 3, 4])
def test_evaluation_matches_the_restatement(sr, ctx, scale, blur, Cn):
    """dtype x terms (DATA / ALL) x weights (none; random in [0, 2]; a binary mask with one whole frame zero; Huber-derived
    on the device, delta 0.1) and a cost-row band, per geometry; problems created with and without shifts_xy."""
    rng, K, w, h, W, H, mats, y, x, regw = _geometry(scale, blur, Cn)
    model = ar.AffineImageModel(scale, mats, blur, 1.0 if blur else 0.0)
    ref = orc.Problem(model, y)
    ref.add_regularizer(orc.REG_BTV, 0.01, 2, 0.6)
    ref.set_irls_weights(0, regw)
    f_reg, g_reg = ref.reg_term(0, x)
    delta = 0.1
    mask = (rng.random(y.shape) < 0.8).astype(float)
    mask[2] = 0.0
    weights = {"none": None, "random": 2.0 * rng.random(y.shape), "mask": mask,
               "huber": rr.huber_weights(rr.residuals(model, y, x), delta)}
    refs = {name: rr.weighted_data_term(model, y, wt, x) for name, wt in weights.items()}
    band = (scale * 3, scale * (h - 5))
    f_band = {name: rr.weighted_data_term(model, y, weights[name], x, want_grad=False, cost_rows=band)[0] for name in ("none", "random")}
    for dtype in (sr.F64, sr.F32):
        # created with shifts_xy (f64) and without (f32): the affine motion replaces either
        shifts = [[0.5 * k, -0.25 * k] for k in range(K)] if dtype == sr.F64 else None
        p = _problem(sr, ctx, W, H, Cn, K, scale, blur, dtype, mats, shifts)
        p.set_observations(y)
        p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
        p.set_irls_weights(0, regw)
        assert p.active_impl() == sr.IMPL_DIRECT
        for name in ("none", "random", "mask", "huber"):
            if name == "huber":
                p.set_data_weights(None)
                p.set_data_loss(sr.DATA_LOSS_HUBER, delta)
                xd = _upload(sr, ctx, p, x)
                p.update_data_weights_device(xd.value)
                ctx.synchronize()
                _free(sr, ctx, xd)
                e = parity_log.note(np.max(np.abs(p.data_weights() - weights["huber"])), "w")
                assert e <= BAR[dtype], e
            elif name != "none":
                p.set_data_weights(weights[name])
            assert p.active_impl() == sr.IMPL_DIRECT
            tag = "f%d %s" % (64 if dtype == sr.F64 else 32, name)
            f, g = p.eval(x, sr.TERM_DATA)
            _check(tag + " DATA", f, g, refs[name][0], refs[name][1], BAR[dtype])
            f, g = p.eval(x, sr.TERM_ALL)
            _check(tag + " ALL", f, g, refs[name][0] + f_reg, refs[name][1] + g_reg.reshape(g.shape), BAR[dtype])
            if name in f_band:
                p.set_cost_rows(*band)
                f, g = p.eval(x, sr.TERM_DATA)
                _check(tag + " band", f, g, f_band[name], refs[name][1], BAR[dtype])
                p.set_cost_rows(0, H)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("scale,blur", [(2, 3), (3, 5), (4, 0)])
def test_operators_match_the_restatement_and_are_adjoint(sr, ctx, scale, blur, dtype):
    rng, K, w, h, W, H, mats, y, x, regw = _geometry(scale, blur, 2)
    model = ar.AffineImageModel(scale, mats, blur, 1.0 if blur else 0.0)
    p = _problem(sr, ctx, W, H, 2, K, scale, blur, dtype, mats)
    u = rng.standard_normal((2, H, W))
    v = rng.standard_normal((2, h, w))
    for k in range(K):
        Au, Atv = p.apply(u, k), p.apply_transpose(v, k)
        ea = parity_log.relerr(Au, model.apply(u, k))
        et = parity_log.relerr(Atv, model.apply_transpose(v, k))
        # the device results: inputs and outputs were rounded to the dtype on the way
        uu, vv = (u, v) if dtype == 0 else (u.astype(np.float32).astype(np.float64), v.astype(np.float32).astype(np.float64))
        lhs, rhs = np.sum(Au * vv), np.sum(uu * Atv)
        # an inner product's rounding error scales with |Au| |v| (Cauchy-Schwarz), not with its possibly cancelling value:
        # a few hundred ulps of the dtype leave 1e-13 / 1e-5
        rel = parity_log.note(abs(lhs - rhs) / np.sqrt(np.sum(Au * Au) * np.sum(vv * vv)), "adjoint")
        print("frame %d: apply %.2e transpose %.2e adjoint identity %.2e" % (k, ea, et, rel))
        assert ea <= BAR[dtype] and et <= BAR[dtype]
        assert rel <= (1e-13 if dtype == 0 else 1e-5)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("scale,blur", [(2, 3), (3, 0), (4, 5)])
def test_pure_translation_matches_the_translational_direct_kernels(sr, ctx, scale, blur, dtype):
    rng = np.random.default_rng(scale + blur)
    Cn, K = 2, len(ANCHOR_SHIFTS)
    w, h = 61 + scale, 24 + scale
    W, H = w * scale, h * scale
    y = rng.random((K, Cn, h, w))
    x = rng.random((Cn, H, W))
    a = _problem(sr, ctx, W, H, Cn, K, scale, blur, dtype, np.stack([ar.translation(dx, dy) for dx, dy in ANCHOR_SHIFTS]))
    t = _problem(sr, ctx, W, H, Cn, K, scale, blur, dtype, None, [list(s) for s in ANCHOR_SHIFTS])
    t.set_impl(sr.IMPL_DIRECT)
    for p in (a, t):
        p.set_observations(y)
        p.add_regularizer(sr.REG_TV, 0.02)
    assert a.active_impl() == sr.IMPL_DIRECT  # linear parts exactly I: still the affine kernels, no silent re-route
    for terms in (sr.TERM_DATA, sr.TERM_ALL):
        fa, ga = a.eval(x, terms)
        ft, gt = t.eval(x, terms)
        _check("terms %d" % terms, fa, ga, ft, gt, BAR[dtype])
    for k in range(K):
        assert parity_log.relerr(a.apply(x, k), t.apply(x, k)) <= BAR[dtype]
        assert parity_log.relerr(a.apply_transpose(y[k], k), t.apply_transpose(y[k], k)) <= BAR[dtype]


@pytest.mark.parametrize("dtype", [0, 1])
def test_evaluations_are_reproducible_and_leave_translational_problems_alone(sr, ctx, dtype):
    rng, K, w, h, W, H, mats, y, x, regw = _geometry(3, 3, 2)
    shifts = [[0.37 * k, -0.61 * k] for k in range(K)]
    t = _problem(sr, ctx, W, H, 2, K, 3, 3, dtype, None, shifts)
    t.set_observations(y)
    t.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
    before = {impl: None for impl in (sr.IMPL_AUTO, sr.IMPL_DIRECT)}
    for impl in before:
        t.set_impl(impl)
        before[impl] = t.eval(x)
    a = _problem(sr, ctx, W, H, 2, K, 3, 3, dtype, mats, shifts)
    a.set_observations(y)
    a.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
    a.set_data_weights(2.0 * rng.random(y.shape))
    f1, g1 = a.eval(x)
    f2, g2 = a.eval(x)
    assert f1 == f2 and np.array_equal(g1, g2)
    for impl in before:
        t.set_impl(impl)
        f, g = t.eval(x)
        assert f == before[impl][0] and np.array_equal(g, before[impl][1]), impl


@pytest.mark.parametrize("dtype", [0, 1])
def test_null_restores_the_motion_the_problem_was_created_with(sr, ctx, dtype):
    rng, K, w, h, W, H, mats, y, x, regw = _geometry(2, 3, 1)
    for shifts in ([[0.37 * k, -0.61 * k] for k in range(K)], [[k % 3, -(k % 2)] for k in range(K)], None):
        fresh = _problem(sr, ctx, W, H, 1, K, 2, 3, dtype, None, shifts)
        p = _problem(sr, ctx, W, H, 1, K, 2, 3, dtype, None, shifts)
        for q in (fresh, p):
            q.set_observations(y)
            q.add_regularizer(sr.REG_TV, 0.02)
        impl0 = fresh.active_impl()
        f0, g0 = fresh.eval(x)
        p.set_affine_motion(mats)
        assert p.active_impl() == sr.IMPL_DIRECT
        fa, ga = p.eval(x)
        assert not np.array_equal(ga, g0)
        p.set_observations(y)  # the motion persists across new observations and weights
        p.set_data_weights(np.ones_like(y))
        p.set_data_weights(None)
        fb, gb = p.eval(x)
        assert fb == fa and np.array_equal(gb, ga)
        p.set_affine_motion(None)
        assert p.active_impl() == impl0
        f1, g1 = p.eval(x)
        assert f1 == f0 and np.array_equal(g1, g0)
        assert np.array_equal(p.apply(x, 1), fresh.apply(x, 1))


def test_errors_and_refusals(sr, ctx):
    rng = np.random.default_rng(2)
    W, H, s, K = 48, 32, 2, 4
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    p = sr.Problem(ctx, W, H, 1, K, s, shifts, 3, 1.0, sr.F64)
    y = rng.random((K, 1, H // s, W // s))
    x0 = rng.random((1, H, W))
    p.set_observations(y)
    p.add_regularizer(sr.REG_TV, 0.01)
    f0, g0 = p.eval(x0)
    impl0 = p.active_impl()
    good = np.stack([ar.rotation_about_centre(d, sh, W, H) for d, sh in zip((0, 2, -1, 1.5), shifts)])
    for bad in (np.nan, np.inf, -np.inf):
        for idx in ((1, 0, 0), (2, 1, 2), (3, 0, 2)):
            m = good.copy()
            m[idx] = bad
            with pytest.raises(sr.SrmapError) as e:
                p.set_affine_motion(m)
            assert e.value.status == sr.EINVAL
    for m1 in ([[1.26, 0, 0], [0, 1, 0]], [[1.1, 0.2, 0], [0, 1, 0]], [[1, 0, 0], [-0.13, 0.87, 0]],
               ar.rotation_about_centre(15.0, (0, 0), W, H), [[-1, 0, 0], [0, -1, 0]], [[0, 0, 0], [0, 0, 0]]):
        m = good.copy()
        m[2] = m1
        with pytest.raises(sr.SrmapError) as e:
            p.set_affine_motion(m)
        assert e.value.status == sr.EUNSUPPORTED
    # a refused call leaves the problem as it was
    assert p.active_impl() == impl0
    f1, g1 = p.eval(x0)
    assert f1 == f0 and np.array_equal(g1, g0)
    # exactly at the bound is inside the domain
    edge = good.copy()
    edge[1] = [[1.25, 0, 0.5], [0.125, 0.875, -0.5]]
    p.set_affine_motion(edge)
    p.set_affine_motion(good)
    assert p.active_impl() == sr.IMPL_DIRECT
    p.set_impl(sr.IMPL_TILED)
    with pytest.raises(sr.SrmapError) as e:
        p.eval(x0)
    assert e.value.status == sr.EUNSUPPORTED
    p.set_impl(sr.IMPL_DIRECT)
    assert np.all(np.isfinite(p.eval(x0)[1]))
    p.set_impl(sr.IMPL_AUTO)
    assert p.active_impl() == sr.IMPL_DIRECT

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
    xd, gd = _upload(sr, ctx, p, x0), _upload(sr, ctx, p, x0)
    for mode in (sr.SHARD_FRAMES, sr.SHARD_ROWS, sr.SHARD_CHANNELS):
        sd = sr.ShardDesc()
        sd.mode = mode
        sd.own_row0, sd.own_row1, sd.own_ch0, sd.own_ch1 = 0, H, 0, 1
        with pytest.raises(sr.SrmapError) as e:
            p.solve(x0, comm=comm, shard=sd)
        assert e.value.status == sr.EUNSUPPORTED
        with pytest.raises(sr.SrmapError) as e:
            p.eval_sharded_device(comm, sd, xd.value, gd.value)
        assert e.value.status == sr.EUNSUPPORTED
    assert fake.calls == []
    _free(sr, ctx, xd)
    _free(sr, ctx, gd)
    x, rep = p.solve(x0)  # unsharded it solves
    assert np.all(np.isfinite(x)) and rep.cg_iterations > 0


# ------------------------------------------------------------------------------------------------ solves
@pytest.fixture(scope="module")
def table():
    return ar.table_inputs()


def _perturbed(x0):
    return x0 * (1 + 1e-14 * np.random.default_rng(1).standard_normal(x0.shape))


def _table_problem(sr, ctx, T, y, mats):
    p = sr.Problem(ctx, T["W"], T["H"], T["C"], T["K"], T["s"], T["shifts"], T["blur"][0], T["blur"][1], sr.F64)
    if mats is not None:
        p.set_affine_motion(mats)
    p.set_observations(y)
    p.add_regularizer(*T["reg"])
    return p


def _agree(tag, T, x, rep, x_ref, rep_ref, own):
    """Counts equal, or the PSNR within max(0.01 dB, 10 x the restatement's own movement under a 1e-14 perturbation)."""
    ps, ps_ref = orc.psnr(T["gt"], x), orc.psnr(T["gt"], x_ref)
    counts, counts_ref = (rep.irls_rounds, rep.cg_iterations, rep.evaluations), (rep_ref.irls_rounds, rep_ref.cg_iterations, rep_ref.nfev)
    print("%s: GPU %.3f dB %s | restatement %.3f dB %s, its own movement %.4f dB" % (tag, ps, counts, ps_ref, counts_ref, own))
    parity_log.note(abs(ps - ps_ref), tag + " psnr")
    assert counts == counts_ref or abs(ps - ps_ref) <= max(0.01, 10 * own)
    return ps


@pytest.mark.parametrize("name,margin", [("0.5deg", 1.5), ("2deg", 10.0)])
def test_solve_matches_the_restatement_and_beats_translation_only(sr, ctx, table, name, margin):
    T = table
    mats, model, y = T["inputs"][name]
    x0 = rr.bilinear(y[0], T["s"])
    kw = dict(reg=T["reg"], composed=True)
    x_ref, rep_ref, _ = rr.irls_solve(model, y, x0, **kw)
    x_p, _, _ = rr.irls_solve(model, y, _perturbed(x0), **kw)
    own = abs(orc.psnr(T["gt"], x_p) - orc.psnr(T["gt"], x_ref))
    x, rep = _table_problem(sr, ctx, T, y, mats).solve(x0)
    ps = _agree(name + " affine L2", T, x, rep, x_ref, rep_ref, own)
    x_t, rep_t = _table_problem(sr, ctx, T, y, None).solve(x0)
    ps_t = orc.psnr(T["gt"], x_t)
    print("%s: bilinear %.3f dB, GPU translation-only L2 %.3f dB (%d / %d / %d), GPU affine L2 %.3f dB" % (
        name, orc.psnr(T["gt"], x0), ps_t, rep_t.irls_rounds, rep_t.cg_iterations, rep_t.evaluations, ps))
    assert ps >= ps_t + margin


@pytest.mark.parametrize("variant", ["lbfgs", "huber", "huber_lbfgs", "split_channels"])
def test_solve_variants_match_the_restatement(sr, ctx, table, variant):
    T = table
    mats, model, y = T["inputs"]["2deg"]
    x0 = rr.bilinear(y[0], T["s"])
    kw = dict(reg=T["reg"], composed=True)
    if "huber" in variant:
        kw.update(loss="huber", delta=T["delta"])
    if "lbfgs" in variant:
        kw.update(solver="lbfgs", m=5)
    x_ref, rep_ref, w_ref = rr.irls_solve(model, y, x0, **kw)
    x_p, _, _ = rr.irls_solve(model, y, _perturbed(x0), **kw)
    own = abs(orc.psnr(T["gt"], x_p) - orc.psnr(T["gt"], x_ref))
    p = _table_problem(sr, ctx, T, y, mats)
    if "huber" in variant:
        p.set_data_loss(sr.DATA_LOSS_HUBER, T["delta"])
    if "lbfgs" in variant:
        p.set_solver(sr.SOLVER_LBFGS, 5)
    o = sr.default_irls_options()
    o.split_channels = 1 if variant == "split_channels" else 0
    x, rep = p.solve(x0, o)
    _agree("2deg " + variant, T, x, rep, x_ref, rep_ref, own)
    if "huber" in variant:
        assert np.min(p.data_weights()) < 1.0


def test_split_channels_equals_per_channel_solves(sr, ctx):
    rng = np.random.default_rng(77)
    s, K, W, H, Cn = 2, 4, 96, 64, 3
    mats = np.stack([ar.rotation_about_centre(d, sh, W, H) for d, sh in zip((0, 1.5, -1, 0.5), ((0, 0), (1.25, .5), (.5, 1), (-1, .25)))])
    lr = rng.random((K, Cn, H // s, W // s))
    x0 = rng.random((Cn, H, W))

    def solve(y, x_start, split):
        p = sr.Problem(ctx, W, H, y.shape[1], K, s, None, 3, 1.0, sr.F64)
        p.set_affine_motion(mats)
        p.set_observations(y)
        p.add_regularizer(sr.REG_TV, 0.01)
        p.set_data_loss(sr.DATA_LOSS_HUBER, 0.1)
        o = sr.default_irls_options()
        o.split_channels, o.max_num_irls_iterations = split, 3
        x, rep = p.solve(x_start, o)
        return x, rep, p.data_weights()

    x, rep, wts = solve(lr, x0, 1)
    its = evs = 0
    for c in range(Cn):
        xc, rc, wc = solve(lr[:, c:c + 1], x0[c:c + 1], 0)
        assert np.array_equal(x[c:c + 1], xc), c
        assert np.array_equal(wts[:, c:c + 1], wc), c
        its += rc.cg_iterations
        evs += rc.evaluations
    assert (rep.cg_iterations, rep.evaluations) == (its, evs)
    assert np.min(wts) < 1.0


def test_cg_trace_follows_the_restatements_mincg(sr, ctx, table):
    T = table
    mats, model, y = T["inputs"]["2deg"]
    x0 = rr.bilinear(y[0], T["s"])
    shape = x0.shape
    ref = orc.Problem(model, y)
    ref.add_regularizer(*T["reg"])
    ref.set_irls_weights(0, np.ones(shape))
    fs = []

    def fg(v):
        xx = v.reshape(shape)
        f, g = rr.weighted_data_term(model, y, None, xx)
        fr, gr = ref.reg_term(0, xx)
        fs.append(f + fr)
        return f + fr, (g + gr.reshape(shape)).ravel()

    maxits = 12
    x_ref, rep_ref = orc.mincg(fg, x0, 0.0, 0.0, 0.0, maxits, use_alglib=orc.have_ref())
    p = _table_problem(sr, ctx, T, y, mats)
    x, its, nfev, term, ftrace = p.cg_trace(x0, 0.0, 0.0, 0.0, maxits)
    print("iterations %d/%d nfev %d/%d termination %d/%d" % (its, rep_ref.iterations, nfev, rep_ref.nfev, term, rep_ref.termination_type))
    assert (its, nfev, term) == (rep_ref.iterations, rep_ref.nfev, rep_ref.termination_type)
    assert len(ftrace) == nfev == len(fs)
    e = parity_log.note(np.max(np.abs(ftrace - np.array(fs)) / np.maximum(1.0, np.abs(fs))), "trace")
    print("max relative deviation of f over %d evaluations: %.3e" % (nfev, e))
    assert e <= 1e-11
    xl, itl, nfl, terml, ftl = p.lbfgs_trace(x0, 5, 0.0, 0.0, 0.0, 4)
    assert itl > 0 and np.all(np.isfinite(xl)) and ftl[-1] < ftl[0]


def test_cli_affine_motion_flag(sr, ctx, table, tmp_path):
    """generate_data --affine_motion_path, then super_resolution --affine_motion_path against the same run given only the
    translations: the 2-degree input's margin (>= 10 dB), and the tool's result equals a Python solve from its own x0."""
    import __graft_entry__ as ge
    from test_gpu_apps import _read_envi, _write_envi
    ge.build_lib()
    gen, srbin = ge.build_apps()
    T = table
    Cn, H, W, s, K = T["C"], T["H"], T["W"], T["s"], T["K"]
    mats = T["inputs"]["2deg"][0]
    gt = T["gt"].astype(np.float32).astype(np.float64)
    gt_cfg = _write_envi(str(tmp_path / "gt"), gt)
    affine = tmp_path / "affine.txt"
    affine.write_text("".join(" ".join(repr(float(v)) for v in m.ravel()) + "\n" for m in mats))
    motion = tmp_path / "motion.txt"
    motion.write_text("".join("%r %r\n" % (float(dx), float(dy)) for dx, dy in T["shifts"]))
    lr_dir = tmp_path / "lr"
    lr_dir.mkdir()
    out = subprocess.run([gen, "--input_image=" + gt_cfg, "--output_image_dir=" + str(lr_dir),
                          "--affine_motion_path=" + str(affine), "--blur_radius=3", "--blur_sigma=1.0", "--noise_sigma=2.55",
                          "--downsampling_scale=%d" % s, "--number_of_frames=%d" % K],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    frames = np.stack([_read_envi(str(lr_dir / ("low_res_%d" % i)), (Cn, H // s, W // s)) for i in range(K)])
    model = ar.AffineImageModel(s, mats, 3, 1.0)
    clean = np.stack([model.apply(gt, k) for k in range(K)])
    sd = float(np.std(frames - clean))
    print("generated frames: noise standard deviation %.4f around the restatement's clean frames" % sd)
    assert 0.008 <= sd <= 0.012

    def run(tag, flag):
        res = str(tmp_path / ("result_" + tag))
        o = subprocess.run([srbin, "--data_path=" + str(lr_dir), "--upsampling_scale=%d" % s, "--blur_radius=3",
                            "--blur_sigma=1.0", flag, "--regularizer=btv", "--btv_scale_range=2",
                            "--regularization_parameter=0.005", "--result_path=" + res,
                            "--save_initial_estimate=" + str(tmp_path / ("x0_" + tag))],
                           capture_output=True, text=True, timeout=600)
        print(o.stdout, o.stderr)
        assert o.returncode == 0
        return np.fromfile(res, dtype="<f4").reshape(Cn, H, W)

    x_a = run("affine", "--affine_motion_path=" + str(affine))
    x_t = run("translation", "--motion_sequence_path=" + str(motion))
    ps_a, ps_t = orc.psnr(gt, x_a.astype(np.float64)), orc.psnr(gt, x_t.astype(np.float64))
    print("CLI: affine %.3f dB, translations only %.3f dB" % (ps_a, ps_t))
    assert ps_a >= ps_t + 10.0
    x0 = np.fromfile(str(tmp_path / "x0_affine"), dtype=np.float64).reshape(Cn, H, W)
    x, _ = _table_problem(sr, ctx, T, frames, mats).solve(x0)
    assert np.array_equal(x.astype(np.float32), x_a)
    both = subprocess.run([srbin, "--data_path=" + str(lr_dir), "--affine_motion_path=" + str(affine),
                           "--motion_sequence_path=" + str(motion)], capture_output=True, text=True, timeout=120)
    assert both.returncode == 1 and "exclude each other" in both.stderr
