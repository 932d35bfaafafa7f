"""The displacement-field motion model on the GPU (include/srmap.h: srmap_problem_set_flow; the flow instances of
k_forward_direct and k_gather_sampled, k_flow_seed and k_flow_check of csrc/kernels_flow.hip) against its numpy / scipy.sparse restatement
(tests/flow_restatement.py: explicit matrices, the literal transpose), against the translational and the affine direct
kernels where the definitions coincide, and against itself.

Bars: cost and every gradient / operator element relative to max(1, |ref|), 1e-12 in f64 and 2e-5 in f32 (the project's
bars).  s = q + u is exact in both the kernels and the restatement (the restatement rounds the field to the problem's dtype
first, as the library stores it), so the two hold the same weights; what is left is summation order."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle as orc
import parity_log

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import blur_kernel_restatement as bk  # noqa: E402
import flow_restatement as fr  # noqa: E402
import robust_restatement as rr  # noqa: E402
from test_flow_cpu import matrix_fields  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = {0: 1e-12, 1: 2e-5}
NP_DTYPE = {0: np.float64, 1: np.float32}
FREE = "free"  # the free-form asymmetric 5 x 5 kernel


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


def _free_taps():
    """Asymmetric under both flips and under transposition: a rotated anisotropic Gaussian plus a one-sided streak."""
    return 0.6 * bk.anisotropic_psf() + 0.4 * bk.streak_psf(5)


def _taps(blur):
    return _free_taps() if blur == FREE else bk.gaussian_taps(blur, 1.0)


def _problem(sr, ctx, W, H, Cn, K, scale, blur, dtype, fields=None, shifts=None):
    b = 0 if blur == FREE else blur
    p = sr.Problem(ctx, W, H, Cn, K, scale, shifts, b, 1.0 if b else 0.0, dtype)
    if blur == FREE:
        p.set_blur_kernel(_free_taps())
    if fields is not None:
        p.set_flow(fields)
    return p


# LR h x w (5 x 7, 9 x 13; 70 x 129 = more than one 256-thread workgroup in both kernels, ragged in both axes) x scale x
# blur x channels x frames; every size sees all seven fields (a K = 5 and a K = 2 case), every scale, blur, C and K twice
FIELD_NAMES = ["zero", "integer", "subpixel", "affine_bound", "sinusoid_bound", "smooth_random", "third_outside"]
CASES = [
    (5, 7, 1, 0, 1, FIELD_NAMES[:5]),
    (5, 7, 4, FREE, 3, FIELD_NAMES[5:]),
    (9, 13, 2, 3, 3, FIELD_NAMES[2:]),
    (9, 13, 3, 5, 1, FIELD_NAMES[:2]),
    (70, 129, 2, FREE, 1, FIELD_NAMES[:5]),
    (70, 129, 3, 3, 3, FIELD_NAMES[5:]),
    (70, 129, 4, 5, 1, [FIELD_NAMES[4], FIELD_NAMES[6]]),
    (70, 129, 1, 5, 1, [FIELD_NAMES[3], FIELD_NAMES[5]]),
]


def _case(h, w, scale, blur, Cn, names):
    rng = np.random.default_rng(1000 * h + 10 * scale + Cn)
    H, W = h * scale, w * scale
    all_fields = matrix_fields(rng, H, W)
    fields = np.stack([all_fields[n] for n in names])
    K = len(names)
    return rng, K, H, W, fields, rng.random((K, Cn, h, w)), rng.random((Cn, H, W)), 0.5 + rng.random((Cn, H, W))


@pytest.mark.parametrize("h,w,scale,blur,Cn,names", CASES)
def test_evaluation_and_operators_match_the_restatement(sr, ctx, h, w, scale, blur, Cn, names):
    """dtype x terms (DATA / ALL) x weights (none; random in [0, 2]; a binary mask with one whole frame zero; Huber-derived
    on the device, delta 0.1) and a cost-row band; apply / apply_transpose per frame and their adjoint identity."""
    rng, K, H, W, fields, y, x, regw = _case(h, w, scale, blur, Cn, names)
    delta = 0.1
    mask = (rng.random(y.shape) < 0.8).astype(float)
    mask[K - 1] = 0.0
    rand = 2.0 * rng.random(y.shape)
    u = rng.standard_normal((Cn, H, W))
    v = rng.standard_normal((Cn, h, w))
    band = (scale * 1, scale * (h - 2))
    for dtype in (sr.F64, sr.F32):
        model = fr.FlowModel(scale, fields, _taps(blur), NP_DTYPE[dtype])
        ref = orc.Problem(model, y)
        ref.add_regularizer(orc.REG_BTV, 0.01, 2, 0.6)
        ref.set_irls_weights(0, regw)
        f_reg, g_reg = ref.reg_term(0, x)
        weights = {"none": None, "random": rand, "mask": mask, "huber": rr.huber_weights(rr.residuals(model, y, x), delta)}
        refs = {name: rr.weighted_data_term(model, y, wt, x) for name, wt in weights.items()}
        f_band = {name: rr.weighted_data_term(model, y, weights[name], x, want_grad=False, cost_rows=band)[0] for name in ("none", "random")}
        # created with shifts_xy (f64) and without (f32): the flow replaces either
        shifts = [[0.5 * k, -0.25 * k] for k in range(K)] if dtype == sr.F64 else None
        p = _problem(sr, ctx, W, H, Cn, K, scale, blur, dtype, fields, shifts)
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
        for k in range(K):
            Au, Atv = p.apply(u, k), p.apply_transpose(v, k)
            ea = parity_log.relerr(Au, model.apply(u, k))
            et = parity_log.relerr(Atv, model.apply_transpose(v, k))
            uu, vv = (u, v) if dtype == 0 else (u.astype(np.float32).astype(np.float64), v.astype(np.float32).astype(np.float64))
            lhs, rhs = np.sum(Au * vv), np.sum(uu * Atv)
            # an inner product's rounding error scales with |Au| |v| (Cauchy-Schwarz), not with its possibly cancelling value
            rel = parity_log.note(abs(lhs - rhs) / max(np.sqrt(np.sum(Au * Au) * np.sum(vv * vv)), 1e-300), "adjoint")
            print("frame %d (%s): apply %.2e transpose %.2e adjoint identity %.2e" % (k, names[k], ea, et, rel))
            assert ea <= BAR[dtype] and et <= BAR[dtype]
            assert rel <= (1e-12 if dtype == 0 else 1e-5)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("scale,blur", [(2, 3), (3, 0), (4, 5)])
def test_integer_flow_matches_the_translational_direct_kernels(sr, ctx, scale, blur, dtype):
    rng = np.random.default_rng(scale + blur)
    shifts = [[0, 0], [1, 1], [-2, 3], [3, -2], [0, -1]]
    Cn, K = 2, len(shifts)
    w, h = 61 + scale, 24 + scale
    W, H = w * scale, h * scale
    y = rng.random((K, Cn, h, w))
    x = rng.random((Cn, H, W))
    a = _problem(sr, ctx, W, H, Cn, K, scale, blur, dtype, sr.flow_from_shifts(shifts, H, W))
    t = _problem(sr, ctx, W, H, Cn, K, scale, blur, dtype, None, shifts)
    t.set_impl(sr.IMPL_DIRECT)
    for p in (a, t):
        p.set_observations(y)
        p.add_regularizer(sr.REG_TV, 0.02)
    assert a.active_impl() == sr.IMPL_DIRECT
    for terms in (sr.TERM_DATA, sr.TERM_ALL):
        fa, ga = a.eval(x, terms)
        ft, gt = t.eval(x, terms)
        _check("terms %d" % terms, fa, ga, ft, gt, BAR[dtype])
    for k in range(K):
        assert parity_log.relerr(a.apply(x, k), t.apply(x, k)) <= BAR[dtype]
        assert parity_log.relerr(a.apply_transpose(y[k], k), t.apply_transpose(y[k], k)) <= BAR[dtype]


@pytest.mark.parametrize("dtype", [0, 1])
def test_affine_derived_flow_matches_the_affine_kernels(sr, ctx, dtype):
    """Within 100 x the difference the restatement itself shows between the two formulations (s = F^-1(q) against
    s = q + (F^-1(q) - q), the field rounded to the dtype)."""
    rng = np.random.default_rng(17)
    s, Cn, h, w = 2, 2, 31, 45
    H, W = h * s, w * s
    mats = np.stack([ar.random_matrix(rng, ar.MAX_DEVIATION, at_bound=True), ar.rotation_about_centre(5.0, (0.7, -1.6), W, H, 1.03),
                     ar.translation(1.3, -0.45)])
    K = len(mats)
    y, x = rng.random((K, Cn, h, w)), rng.random((Cn, H, W))
    fields = fr.from_affine(mats, H, W)
    m_flow = fr.gaussian_model(s, fields, 3, 1.0, NP_DTYPE[dtype])
    m_aff = ar.AffineImageModel(s, mats, 3, 1.0)
    f_f, g_f = rr.weighted_data_term(m_flow, y, None, x)
    f_a, g_a = rr.weighted_data_term(m_aff, y, None, x)
    own_f, own_g = abs(f_f - f_a) / max(1.0, abs(f_a)), parity_log.relerr(g_f, g_a)
    a = _problem(sr, ctx, W, H, Cn, K, s, 3, dtype)
    a.set_affine_motion(mats)
    p = _problem(sr, ctx, W, H, Cn, K, s, 3, dtype, fields)
    for q in (a, p):
        q.set_observations(y)
    fa, ga = a.eval(x, sr.TERM_DATA)
    fp, gp = p.eval(x, sr.TERM_DATA)
    ef, eg = abs(fp - fa) / max(1.0, abs(fa)), parity_log.relerr(gp, ga)
    print("restatement: cost %.3e gradient %.3e between the formulations; GPU: cost %.3e gradient %.3e" % (own_f, own_g, ef, eg))
    assert ef <= 100 * own_f and eg <= 100 * own_g


def test_adjoint_identity_at_the_domain_bound(sr, ctx):
    """<A u, v> = <u, A^T v> through apply / apply_transpose to 1e-12 (f64), the field AT the documented bound."""
    rng = np.random.default_rng(23)
    s, Cn, h, w = 3, 2, 23, 37
    H, W = h * s, w * s
    fields = np.stack([fr.at_bound(fr.sinusoid(H, W, 1.0, 11.0 + 6 * k, offset=(20.0 * (-1) ** k, -13.5), phase=0.7 * k)) for k in range(3)])
    for f in fields:
        assert abs(sum(fr.neighbour_differences(f)) - fr.NEIGHBOUR_BOUND) <= 1e-9
    p = _problem(sr, ctx, W, H, Cn, len(fields), s, 5, sr.F64, fields)
    for k in range(len(fields)):
        u, v = rng.standard_normal((Cn, H, W)), rng.standard_normal((Cn, h, w))
        Au, Atv = p.apply(u, k), p.apply_transpose(v, k)
        rel = abs(np.sum(Au * v) - np.sum(u * Atv)) / np.sqrt(np.sum(Au * Au) * np.sum(v * v))
        print("frame %d: adjoint identity %.2e" % (k, rel))
        assert rel <= 1e-12


# ------------------------------------------------------------------------------------------------ status and state
def _state_case(seed=31, Cn=2):
    rng = np.random.default_rng(seed)
    s, h, w, K = 2, 21, 33, 4
    H, W = h * s, w * s
    fields = np.stack([fr.smooth_random(rng, H, W, 1.5) + fr.from_shifts([[0.5 * k, -0.75 * k]], H, W)[0] for k in range(K)])
    return rng, s, h, w, K, H, W, fields, rng.random((K, Cn, h, w)), rng.random((Cn, H, W))


@pytest.mark.parametrize("dtype", [0, 1])
def test_repeats_permutation_and_device_tensor_are_bit_identical(sr, ctx, dtype):
    import torch
    rng, s, h, w, K, H, W, fields, y, x = _state_case()
    p = _problem(sr, ctx, W, H, 2, K, s, 3, dtype, fields)
    p.set_observations(y)
    p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
    p.set_data_weights(2.0 * rng.random(y.shape))
    wts = p.data_weights()
    f1, g1 = p.eval(x)
    f2, g2 = p.eval(x)
    assert f1 == f2 and np.array_equal(g1, g2)
    assert np.array_equal(p.flow(), fr.stored(fields, NP_DTYPE[dtype]))
    # a permuted frame stack permutes nothing else: frame k's operator is the same bits wherever the frame sits
    perm = [2, 0, 3, 1]
    q = _problem(sr, ctx, W, H, 2, K, s, 3, dtype, fields[perm])
    for k in range(K):
        assert np.array_equal(q.apply(x, k), p.apply(x, perm[k]))
        assert np.array_equal(q.apply_transpose(y[0], k), p.apply_transpose(y[0], perm[k]))
    # host array against device tensor
    t = torch.from_numpy(np.ascontiguousarray(fields.astype(NP_DTYPE[dtype]))).to("cuda")
    torch.cuda.synchronize()
    d = _problem(sr, ctx, W, H, 2, K, s, 3, dtype)
    d.set_flow(t)
    d.set_observations(y)
    d.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
    d.set_data_weights(wts)
    f3, g3 = d.eval(x)
    assert f3 == f1 and np.array_equal(g3, g1)
    assert np.array_equal(d.flow(), p.flow())


@pytest.mark.parametrize("dtype", [0, 1])
def test_null_restores_and_flow_and_affine_replace_each_other(sr, ctx, dtype):
    rng, s, h, w, K, H, W, fields, y, x = _state_case(Cn=1)
    mats = np.stack([ar.rotation_about_centre(1.0 + k, (0.5 * k, -0.25), W, H) for k in range(K)])
    for shifts in ([[0.37 * k, -0.61 * k] for k in range(K)], [[k % 3, -(k % 2)] for k in range(K)], None):
        fresh = _problem(sr, ctx, W, H, 1, K, s, 3, dtype, None, shifts)
        p = _problem(sr, ctx, W, H, 1, K, s, 3, dtype, None, shifts)
        only_affine = _problem(sr, ctx, W, H, 1, K, s, 3, dtype, None, shifts)
        only_affine.set_affine_motion(mats)
        for q in (fresh, p, only_affine):
            q.set_observations(y)
            q.add_regularizer(sr.REG_TV, 0.02)
        impl0 = fresh.active_impl()
        f0, g0 = fresh.eval(x)
        fA, gA = only_affine.eval(x)
        assert p.flow() is None
        p.set_flow(fields)
        assert p.active_impl() == sr.IMPL_DIRECT
        fa, ga = p.eval(x)
        assert not np.array_equal(ga, g0)
        # the flow persists across new observations, weights, the blur and the photometric parameters
        p.set_observations(y)
        p.set_data_weights(np.ones_like(y))
        p.set_data_weights(None)
        p.set_blur_kernel(_free_taps())
        p.set_blur_kernel(None)
        p.set_photometric(np.tile([1.25, 0.1], (K, 1)))
        assert p.flow() is not None
        p.set_photometric(None)
        fb, gb = p.eval(x)
        assert fb == fa and np.array_equal(gb, ga)
        # set-flow then set-affine: the affine model, as if the flow had never been set; and the reverse
        p.set_affine_motion(mats)
        assert p.flow() is None
        f1, g1 = p.eval(x)
        assert f1 == fA and np.array_equal(g1, gA)
        p.set_flow(fields)
        f2, g2 = p.eval(x)
        assert f2 == fa and np.array_equal(g2, ga)
        # NULL (to either call) restores the created motion bit for bit
        p.set_flow(None)
        assert p.active_impl() == impl0 and p.flow() is None
        f3, g3 = p.eval(x)
        assert f3 == f0 and np.array_equal(g3, g0)
        p.set_flow(fields)
        p.set_affine_motion(None)
        f4, g4 = p.eval(x)
        assert f4 == f0 and np.array_equal(g4, g0)
        assert np.array_equal(p.apply(x, 1), fresh.apply(x, 1))


def test_flow_with_photometric_parameters_and_free_form_blur(sr, ctx):
    """The photometric normalisation and a free-form blur act on a flow problem as the restatement composes them."""
    rng, s, h, w, K, H, W, fields, y, x = _state_case(seed=37)
    gb = np.stack([1.0 + 0.1 * np.arange(K), 0.02 * np.arange(K) - 0.03], axis=1)
    model = fr.FlowModel(s, fields, _free_taps())
    f_ref, g_ref = rr.weighted_data_term(model, (y - gb[:, 1, None, None, None]) / gb[:, 0, None, None, None], None, x)
    p = _problem(sr, ctx, W, H, 2, K, s, FREE, sr.F64, fields)
    p.set_observations(y)
    p.set_photometric(gb)
    f, g = p.eval(x, sr.TERM_DATA)
    _check("photometric + free-form", f, g, f_ref, g_ref, BAR[0])


def test_errors_and_refusals(sr, ctx):
    rng, s, h, w, K, H, W, fields, y, x0 = _state_case(seed=41, Cn=1)
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    p = sr.Problem(ctx, W, H, 1, K, s, shifts, 3, 1.0, sr.F64)
    p.set_observations(y)
    p.add_regularizer(sr.REG_TV, 0.01)
    impl0 = p.active_impl()

    def refused(bad, status):
        with pytest.raises(sr.SrmapError) as e:
            p.set_flow(bad)
        assert e.value.status == status, e.value

    for state in ("created", "flow"):
        if state == "flow":
            p.set_flow(fields)
        f0, g0 = p.eval(x0)
        impl = p.active_impl()
        for bad_value in (np.nan, np.inf, -np.inf):
            for idx in ((1, 0, 3, 4), (3, 1, H - 1, W - 1)):
                bad = fields.copy()
                bad[idx] = bad_value
                refused(bad, sr.EINVAL)
        bad = fields.copy()
        bad[2, 0, 5, 6] = 2.0 ** 20 + 1
        refused(bad, sr.EUNSUPPORTED)
        bad = fields.copy()
        bad[1] = fr.folded(H, W)
        assert fr.classify(bad[1], W, H) == "eunsupported"
        refused(bad, sr.EUNSUPPORTED)
        # a refused call leaves the problem as it was: the next evaluation is bit-identical to the previous one
        assert p.active_impl() == impl
        f1, g1 = p.eval(x0)
        assert f1 == f0 and np.array_equal(g1, g0)
    assert impl0 in (sr.IMPL_DIRECT, sr.IMPL_TILED) and p.active_impl() == sr.IMPL_DIRECT
    p.set_impl(sr.IMPL_TILED)
    with pytest.raises(sr.SrmapError) as e:
        p.eval(x0)
    assert e.value.status == sr.EUNSUPPORTED
    p.set_impl(sr.IMPL_AUTO)
    assert p.active_impl() == sr.IMPL_DIRECT
    for call in (lambda: p.refine_motion(x0), lambda: p.fit_blur(x0), lambda: p.fit_photometric(x0)):
        with pytest.raises(sr.SrmapError) as e:
            call()
        assert e.value.status == sr.EUNSUPPORTED and "displacement field" in str(e.value)

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
    return fr.table_inputs()


def _table_problem(sr, ctx, T, y, fields):
    p = sr.Problem(ctx, T["W"], T["H"], T["C"], T["K"], T["s"], T["shifts"], T["blur"][0], T["blur"][1], sr.F64)
    if fields is not None:
        p.set_flow(fields)
    p.set_observations(y)
    p.add_regularizer(*T["reg"])
    return p


@pytest.mark.parametrize("variant,pinned", [("cg", "flow_l2"), ("lbfgs", "flow_lbfgs"), ("huber", "flow_huber"),
                                            ("split_channels", "flow_l2")])
def test_solves_match_the_pinned_table(sr, ctx, table, variant, pinned):
    """Same rounds / iterations / evaluations as the restatement's pinned solve (fr.TABLE, re-derived on the CPU by
    tests/test_flow_cpu.py) and PSNR within 0.01 dB."""
    T = table
    x0 = rr.bilinear(T["y"][0], T["s"])
    p = _table_problem(sr, ctx, T, T["y"], T["fields"])
    if variant == "huber":
        p.set_data_loss(sr.DATA_LOSS_HUBER, T["delta"])
    if variant == "lbfgs":
        p.set_solver(sr.SOLVER_LBFGS, 5)
    o = sr.default_irls_options()
    o.split_channels = 1 if variant == "split_channels" else 0
    x, rep = p.solve(x0, o)
    ps, counts = orc.psnr(T["gt"], x), (rep.irls_rounds, rep.cg_iterations, rep.evaluations)
    ps_ref, counts_ref = fr.TABLE[pinned]
    print("%s: GPU %.3f dB %s | restatement %.3f dB %s" % (variant, ps, counts, ps_ref, counts_ref))
    parity_log.note(abs(ps - ps_ref), variant + " psnr")
    assert counts == counts_ref
    assert abs(ps - ps_ref) <= 0.01
    if variant == "huber":
        assert np.min(p.data_weights()) < 1.0
    if variant == "cg":
        assert ps >= fr.TABLE["translation_l2"][0] + 5.0 and abs(ps - fr.TABLE["undeformed_l2"][0]) <= 0.3


def test_cg_trace_follows_the_restatements_mincg(sr, ctx, table):
    T = table
    model, y = T["model"], T["y"]
    x0 = rr.bilinear(y[0], T["s"])
    shape = x0.shape
    ref = orc.Problem(model, y)
    ref.add_regularizer(*T["reg"])
    ref.set_irls_weights(0, np.ones(shape))
    fs = []

    def fg(v):
        xx = v.reshape(shape)
        f, g = rr.weighted_data_term(model, y, None, xx)
        fr_, gr = ref.reg_term(0, xx)
        fs.append(f + fr_)
        return f + fr_, (g + gr.reshape(shape)).ravel()

    maxits = 12
    x_ref, rep_ref = orc.mincg(fg, x0, 0.0, 0.0, 0.0, maxits, use_alglib=orc.have_ref())
    p = _table_problem(sr, ctx, T, y, T["fields"])
    x, its, nfev, term, ftrace = p.cg_trace(x0, 0.0, 0.0, 0.0, maxits)
    print("iterations %d/%d nfev %d/%d termination %d/%d" % (its, rep_ref.iterations, nfev, rep_ref.nfev, term, rep_ref.termination_type))
    assert (its, nfev, term) == (rep_ref.iterations, rep_ref.nfev, rep_ref.termination_type)
    assert len(ftrace) == nfev == len(fs)
    e = parity_log.note(np.max(np.abs(ftrace - np.array(fs)) / np.maximum(1.0, np.abs(fs))), "trace")
    print("max relative deviation of f over %d evaluations: %.3e" % (nfev, e))
    assert e <= 1e-11


# ------------------------------------------------------------------------------------------------ the tools and the facade
def test_cli_flow_motion_flag(tmp_path):
    """generate_data --flow_motion_path on a 48 x 64 ground truth and K = 4 frames makes the restatement's frames;
    super_resolution --flow_motion_path on them ends where the restatement's solve of the same frames ends (PSNR within
    0.01 dB, the margin of tests/test_gpu_photometric.py's tool runs), well above the run that is given the translations only."""
    import subprocess
    from conftest import ROOT
    from test_gpu_apps import _read_envi, _write_envi
    libdir = os.path.join(ROOT, "super-resolution_amd", "lib")
    gen, srbin = os.path.join(libdir, "generate_data"), os.path.join(libdir, "super_resolution")
    assert os.path.exists(gen) and os.path.exists(srbin), "build() makes the tools"
    C_, H, W, s, K = 1, 48, 64, 2, 4
    rng = np.random.default_rng(21)
    gt = np.clip(0.8 * rr.prototype_ground_truth(C_, H, W) + 0.1 * rng.random((C_, H, W)), 0, 1).astype(np.float32).astype(np.float64)
    gt_cfg = _write_envi(str(tmp_path / "gt"), gt)
    shifts = ar.TABLE_SHIFTS[:K]
    fields = fr.table_fields(H, W, shifts)
    flow = tmp_path / "flow.bin"
    np.ascontiguousarray(fields, dtype="<f8").tofile(str(flow))
    motion = tmp_path / "motion.txt"
    motion.write_text("".join("%r %r\n" % (float(a), float(b)) for a, b in shifts))
    lr_dir = tmp_path / "lr"
    lr_dir.mkdir()
    out = subprocess.run([gen, "--input_image=" + gt_cfg, "--output_image_dir=" + str(lr_dir), "--flow_motion_path=" + str(flow),
                          "--blur_radius=3", "--blur_sigma=1.0", "--downsampling_scale=%d" % s, "--number_of_frames=%d" % K],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    frames = np.stack([_read_envi(str(lr_dir / ("low_res_%d" % i)), (C_, H // s, W // s)) for i in range(K)]).astype(np.float64)
    model = fr.gaussian_model(s, fields, 3, 1.0)
    for k in range(K):
        assert np.allclose(frames[k], model.apply(gt, k), atol=3e-7)
    base = [srbin, "--data_path=" + str(lr_dir), "--ground_truth_image=" + gt_cfg, "--upsampling_scale=%d" % s, "--blur_radius=3",
            "--blur_sigma=1.0", "--regularizer=btv", "--btv_scale_range=2", "--regularization_parameter=0.005",
            "--optimization_iterations=5", "--solver_iterations=30", "--evaluators=psnr"]

    def run(*flags):
        o = subprocess.run(base + list(flags), capture_output=True, text=True, timeout=600)
        print(o.stdout, o.stderr)
        assert o.returncode == 0
        return [float(l.split(":")[1]) for l in o.stdout.splitlines() if l.startswith("PSNR score on result")][0]

    ps_flow = run("--flow_motion_path=" + str(flow))
    ps_trans = run("--motion_sequence_path=" + str(motion))
    x0 = rr.bilinear(frames[0], s)
    o = orc.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = 5, 30
    ref = orc.psnr(gt, rr.irls_solve(model, frames, x0, reg=(orc.REG_BTV, 0.005, 2, 0.5), options=o, composed=True)[0])
    print("CLI / restatement: %.4f / %.4f dB with the flow; CLI with the translations only %.4f dB" % (ps_flow, ref, ps_trans))
    assert abs(ps_flow - ref) <= 0.01
    assert ps_flow >= ps_trans + 5.0
    short = subprocess.run([gen, "--input_image=" + gt_cfg, "--output_image_dir=" + str(lr_dir), "--flow_motion_path=" + str(flow),
                            "--number_of_frames=%d" % (K + 1)], capture_output=True, text=True, timeout=120)
    assert short.returncode == 1 and "holds 4 frames" in short.stderr


def test_host_facade_returns_what_the_c_calls_return(tmp_path):
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "super-resolution_amd", "lib", "flow_motion_test")
    assert os.path.exists(exe), "build() makes the facade test binary"
    o = subprocess.run([exe, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(o.stdout, o.stderr)
    assert o.returncode == 0 and "FLOW MOTION FACADE TESTS PASSED" in o.stdout
