"""The robust data term on the GPU (include/srmap.h: srmap_set_data_weights*, srmap_get_data_weights,
srmap_problem_set_data_loss, srmap_update_data_weights_device; the WEIGHTED instances of k_forward_sp / k_forward_direct,
k_huber_weights, the Huber rounds of csrc/solver.hip) against its numpy restatement over the CPU oracle
(tests/robust_restatement.py), and against itself across the library's switches.

Bars: cost and every gradient element relative to max(1, |ref|), 1e-12 in f64 and 2e-5 in f32 (the project's bars)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as orc
import parity_log

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_restatement as rr  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = {0: 1e-12, 1: 2e-5}


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


def _upload(sr, ctx, p, a):
    """A device copy of `a` in the problem's dtype; returns the raw pointer (freed with the context's allocator)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    ptr = C.c_void_p()
    ctx.check(sr.load().srmap_device_alloc(ctx._h, a.size * 8, C.byref(ptr)))
    ctx.check(sr.load().srmap_upload(p.handle, a.ctypes.data_as(sr.c_double_p), ptr, a.size))
    return ptr


def _free(sr, ctx, ptr):
    ctx.check(sr.load().srmap_device_free(ctx._h, ptr))


def _geometry(scale, blur, subpixel, Cn):
    """Sizes that are multiples neither of the tile (64 LR cells x 8 HR rows) nor of 64 LR cells."""
    rng = np.random.default_rng(1000 * scale + 100 * blur + 10 * subpixel + Cn)
    K = 5
    w, h = 70 + 3 * scale + Cn, 27 + scale
    if subpixel:
        shifts = [[0.0, 0.0]] + [[float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2))] for _ in range(K - 1)]
    else:
        shifts = [[0, 0]] + [[int(rng.integers(-2, 3)), int(rng.integers(-2, 3))] for _ in range(K - 1)]
    y = rng.random((K, Cn, h, w))
    x = rng.random((Cn, h * scale, w * scale))
    regw = 0.5 + rng.random(x.shape)
    return rng, K, w, h, shifts, y, x, regw


def _check(tag, f, g, f_ref, g_ref, bar):
    ef = parity_log.note(abs(f - f_ref) / max(1.0, abs(f_ref)), tag + " cost")
    eg = parity_log.relerr(g, g_ref)
    print("%s: cost %.3e gradient %.3e (bar %.0e)" % (tag, ef, eg, bar))
    assert ef <= bar and eg <= bar, (tag, ef, eg)


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("subpixel", [False, True])
@pytest.mark.parametrize("blur", [0, 3])
@pytest.mark.parametrize("scale", [2, 3, 4])
def test_weighted_evaluation_matches_the_composition(sr, ctx, scale, blur, subpixel, Cn):
    """dtype x impl (AUTO / DIRECT / TILED) x terms (DATA / ALL) x weights (random in [0, 2]; a binary mask with one
    whole frame zero; Huber-derived on the device, delta 0.1) and a cost-row band, per geometry."""
    rng, K, w, h, shifts, y, x, regw = _geometry(scale, blur, subpixel, Cn)
    H, W = h * scale, w * scale
    model = orc.ImageModel(scale=scale, shifts=shifts, blur_ksize=blur, blur_sigma=1.0 if blur else 0.0)
    ref = orc.Problem(model, y)
    ref.add_regularizer(orc.REG_BTV, 0.01, 2, 0.6)
    ref.set_irls_weights(0, regw)
    f_reg, g_reg = ref.reg_term(0, x)
    delta = 0.1
    mask = (rng.random(y.shape) < 0.8).astype(float)
    mask[2] = 0.0
    weights = {"random": 2.0 * rng.random(y.shape), "mask": mask, "huber": rr.huber_weights(rr.residuals(model, y, x), delta)}
    refs = {name: rr.weighted_data_term(model, y, wt, x) for name, wt in weights.items()}
    band = (scale * 3, scale * (h - 5))
    f_band, _ = rr.weighted_data_term(model, y, weights["random"], x, want_grad=False, cost_rows=band)
    for dtype in (sr.F64, sr.F32):
        for impl in (sr.IMPL_AUTO, sr.IMPL_DIRECT, sr.IMPL_TILED):
            p = sr.Problem(ctx, W, H, Cn, K, scale, shifts, blur, 1.0 if blur else 0.0, dtype)
            p.set_impl(impl)
            p.set_observations(y)
            p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
            p.set_irls_weights(0, regw)
            for name in ("random", "mask", "huber"):
                if name == "huber":
                    p.set_data_loss(sr.DATA_LOSS_HUBER, delta)
                    xd = _upload(sr, ctx, p, x)
                    p.update_data_weights_device(xd.value)
                    ctx.synchronize()
                    _free(sr, ctx, xd)
                else:
                    p.set_data_weights(weights[name])
                # a problem with weights keeps the tile family wherever the forward-residual plan admits the geometry
                assert p.active_impl() == (sr.IMPL_DIRECT if impl == sr.IMPL_DIRECT else sr.IMPL_TILED)
                tag = "f%d impl %d %s" % (64 if dtype == sr.F64 else 32, impl, name)
                f, g = p.eval(x, sr.TERM_DATA)
                _check(tag + " DATA", f, g, refs[name][0], refs[name][1], BAR[dtype])
                f, g = p.eval(x, sr.TERM_ALL)
                _check(tag + " ALL", f, g, refs[name][0] + f_reg, refs[name][1] + g_reg.reshape(g.shape), BAR[dtype])
                if name == "random":
                    p.set_cost_rows(*band)
                    f, g = p.eval(x, sr.TERM_DATA)
                    _check(tag + " band", f, g, f_band, refs[name][1], BAR[dtype])
                    p.set_cost_rows(0, H)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("subpixel", [False, True])
def test_zero_frame_mask_equals_problem_without_the_frames(sr, ctx, subpixel, dtype):
    rng, K, w, h, shifts, y, x, regw = _geometry(4, 3, subpixel, 2)
    H, W = 4 * h, 4 * w
    keep = [0, 2, 3]
    wts = np.zeros_like(y)
    wts[keep] = 1.0
    full = sr.Problem(ctx, W, H, 2, K, 4, shifts, 3, 1.0, dtype)
    full.set_observations(y)
    full.set_data_weights(wts)
    part = sr.Problem(ctx, W, H, 2, len(keep), 4, [shifts[k] for k in keep], 3, 1.0, dtype)
    part.set_observations(y[keep])
    for terms in (sr.TERM_DATA, sr.TERM_ALL):
        fa, ga = full.eval(x, terms)
        fb, gb = part.eval(x, terms)
        _check("terms %d" % terms, fa, ga, fb, gb, BAR[dtype])


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("impl", [0, 1])
def test_unit_weights_are_bit_identical_on_subpixel_shifts(sr, ctx, impl, dtype):
    """Sub-pixel geometry: the weighted evaluation runs the same kernels behind the forward kernel, and w = 1.0
    multiplies exactly."""
    rng, K, w, h, shifts, y, x, regw = _geometry(3, 3, True, 2)
    p = sr.Problem(ctx, 3 * w, 3 * h, 2, K, 3, shifts, 3, 1.0, dtype)
    p.set_impl(impl)
    p.set_observations(y)
    p.add_regularizer(sr.REG_TV, 0.02)
    p.set_irls_weights(0, regw)
    f0, g0 = p.eval(x)
    p.set_data_weights(np.ones_like(y))
    f1, g1 = p.eval(x)
    assert f1 == f0 and np.array_equal(g1, g0)
    assert np.array_equal(p.data_weights(), np.ones_like(y))


@pytest.mark.parametrize("dtype", [0, 1])
def test_switching_weights_off_restores_the_integer_shift_plan(sr, ctx, dtype):
    """Integer shifts: weights re-plan the tile family into its forward-residual form (parity, not bit equality, with the
    in-tile form); taking them away re-plans back, bit for bit the evaluation before."""
    rng, K, w, h, shifts, y, x, regw = _geometry(4, 3, False, 1)
    p = sr.Problem(ctx, 4 * w, 4 * h, 1, K, 4, shifts, 3, 1.0, dtype)
    p.set_observations(y)
    p.add_regularizer(sr.REG_BTV, 0.01, 3, 0.5)
    f0, g0 = p.eval(x)
    assert np.array_equal(p.data_weights(), np.ones_like(y))
    p.set_data_weights(np.ones_like(y))
    assert p.active_impl() == sr.IMPL_TILED
    f1, g1 = p.eval(x)
    _check("ones vs none", f1, g1, f0, g0, BAR[dtype])
    p.set_data_weights(None)
    f2, g2 = p.eval(x)
    assert f2 == f0 and np.array_equal(g2, g0)
    # weights persist across new observations
    wts = 2.0 * rng.random(y.shape)
    p.set_data_weights(wts)
    p.set_observations(y)
    got = p.data_weights()
    assert np.max(np.abs(got - wts)) <= (0.0 if dtype == 0 else 2.0 ** -23)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("subpixel", [False, True])
@pytest.mark.parametrize("impl", [0, 1])
def test_update_data_weights_matches_huber_weights(sr, ctx, impl, subpixel, dtype):
    """k_huber_weights on the device's unweighted residuals against huber_weights on the composed residual: 1e-12 (f64) /
    2e-5 (f32) ABSOLUTE, weights in [0, 1].  The function is continuous at |r| = delta, so a rounding tie cannot show; its
    sensitivity to the residual's own rounding dr is dw <= dr / delta, largest at |r| = delta: delta = 0.1 on residuals
    spread over (-1, 1) puts both branches to work and keeps an f32 residual error of a few 1e-7 at a few 1e-6 in w."""
    delta = 0.1
    for Cn, scale, blur in ((1, 2, 3), (3, 4, 3), (2, 3, 0)):
        rng, K, w, h, shifts, y, x, regw = _geometry(scale, blur, subpixel, Cn)
        model = orc.ImageModel(scale=scale, shifts=shifts, blur_ksize=blur, blur_sigma=1.0 if blur else 0.0)
        want = rr.huber_weights(rr.residuals(model, y, x), delta)
        p = sr.Problem(ctx, scale * w, scale * h, Cn, K, scale, shifts, blur, 1.0 if blur else 0.0, dtype)
        p.set_impl(impl)
        p.set_observations(y)
        p.set_data_loss(sr.DATA_LOSS_HUBER, delta)
        xd = _upload(sr, ctx, p, x)
        p.update_data_weights_device(xd.value)
        got = p.data_weights()
        _free(sr, ctx, xd)
        e = parity_log.note(np.max(np.abs(got - want)), "w")
        print("C %d scale %d blur %d: max |w - ref| %.3e, share below 1: %.2f" % (Cn, scale, blur, e, np.mean(want < 1)))
        assert 0.1 < np.mean(want < 1) < 0.99
        assert np.min(got) >= 0.0 and np.max(got) <= 1.0
        assert e <= BAR[dtype]


# ------------------------------------------------------------------------------------------------ solves
@pytest.fixture(scope="module")
def proto():
    return rr.prototype_inputs()


def _gpu_problem(sr, ctx, proto, y, dtype=0, reg=True):
    p = sr.Problem(ctx, proto["W"], proto["H"], proto["C"], proto["K"], proto["s"], proto["shifts"], proto["blur"][0],
                   proto["blur"][1], dtype)
    p.set_observations(y)
    if reg:
        p.add_regularizer(*proto["reg"])
    return p


def _perturbed(x0):
    return x0 * (1 + 1e-14 * np.random.default_rng(1).standard_normal(x0.shape))


@pytest.mark.parametrize("solver", ["cg", "lbfgs"])
def test_huber_solve_matches_the_restatement_on_the_noise_input(sr, ctx, proto, solver):
    """Noise-only input, Huber 0.02: identical rounds / iterations / evaluations; cost within 1e-9 relative and x within
    1e-7 (the bars of test_gpu_solve_parity.py::_compare), or 10 x the restatement's own movement under a 1e-14 relative
    perturbation of the start, whichever is larger (measured in place)."""
    name, y, _ = proto["inputs"][0]
    x0 = rr.bilinear(y[0], proto["s"])
    kw = dict(reg=proto["reg"], loss="huber", delta=proto["delta"], solver=solver, m=5)
    x_ref, rep_ref, w_ref = rr.irls_solve(proto["model"], y, x0, **kw)
    x_p, rep_p, _ = rr.irls_solve(proto["model"], y, _perturbed(x0), **kw)
    own_cost, own_x = abs(rep_p.final_cost - rep_ref.final_cost), np.max(np.abs(x_p - x_ref))
    p = _gpu_problem(sr, ctx, proto, y)
    p.set_data_loss(sr.DATA_LOSS_HUBER, proto["delta"])
    if solver == "lbfgs":
        p.set_solver(sr.SOLVER_LBFGS, 5)
    x, rep = p.solve(x0)
    dc, dx = abs(rep.final_cost - rep_ref.final_cost), np.max(np.abs(x - x_ref))
    print("%s: rounds %d/%d iterations %d/%d evaluations %d/%d cost %.12g / %.12g; GPU vs restatement: cost %.3e x %.3e; "
          "restatement under a 1e-14 perturbation: cost %.3e x %.3e; PSNR %.3f / %.3f dB" % (
              solver, rep.irls_rounds, rep_ref.irls_rounds, rep.cg_iterations, rep_ref.cg_iterations, rep.evaluations,
              rep_ref.nfev, rep.final_cost, rep_ref.final_cost, dc, dx, own_cost, own_x, orc.psnr(proto["gt"], x),
              orc.psnr(proto["gt"], x_ref)))
    parity_log.note(dc / abs(rep_ref.final_cost), "cost")
    parity_log.note(dx, "x")
    assert (rep.irls_rounds, rep.cg_iterations, rep.evaluations) == (rep_ref.irls_rounds, rep_ref.cg_iterations, rep_ref.nfev)
    assert dc <= max(1e-9 * abs(rep_ref.final_cost), 10 * own_cost)
    assert dx <= max(1e-7, 10 * own_x)
    # the weights follow the residuals, |dw| <= |dr| / delta, and |dr| <= max |dx| (the rows of A sum to at most 1)
    assert parity_log.note(np.max(np.abs(p.data_weights() - w_ref)), "w") <= max(1e-7, 10 * own_x) / proto["delta"]


@pytest.mark.parametrize("which", [1, 2])
def test_huber_solve_on_the_outlier_inputs(sr, ctx, proto, which):
    """Salt-and-pepper / misregistered frame: the GPU Huber PSNR within max(0.01 dB, 10 x the restatement's own PSNR
    movement under a 1e-14 perturbation) of the restatement's; at least 10 dB above the GPU L2 solve; on the
    salt-and-pepper input the final weights separate the corruption (< 0.5 on >= 90 % of the corrupted LR pixels, >= 0.5
    on >= 90 % of the clean ones)."""
    name, y, corrupted = proto["inputs"][which]
    gt = proto["gt"]
    x0 = rr.bilinear(y[0], proto["s"])
    kw = dict(reg=proto["reg"], loss="huber", delta=proto["delta"])
    x_ref, rep_ref, _ = rr.irls_solve(proto["model"], y, x0, **kw)
    x_p, _, _ = rr.irls_solve(proto["model"], y, _perturbed(x0), **kw)
    psnr_ref, own = orc.psnr(gt, x_ref), abs(orc.psnr(gt, x_p) - orc.psnr(gt, x_ref))
    p = _gpu_problem(sr, ctx, proto, y)
    x_l2, rep_l2 = p.solve(x0)
    p.set_data_loss(sr.DATA_LOSS_HUBER, proto["delta"])
    x, rep = p.solve(x0)
    psnr_l2, psnr_h = orc.psnr(gt, x_l2), orc.psnr(gt, x)
    print("%s: bilinear %.3f | GPU L2 %.3f (%d / %d / %d) | GPU Huber %.3f (%d / %d / %d) | restatement Huber %.3f "
          "(%d / %d / %d), its own movement %.4f dB" % (
              name, orc.psnr(gt, x0), psnr_l2, rep_l2.irls_rounds, rep_l2.cg_iterations, rep_l2.evaluations, psnr_h,
              rep.irls_rounds, rep.cg_iterations, rep.evaluations, psnr_ref, rep_ref.irls_rounds, rep_ref.cg_iterations,
              rep_ref.nfev, own))
    parity_log.note(abs(psnr_h - psnr_ref), "psnr")
    assert abs(psnr_h - psnr_ref) <= max(0.01, 10 * own)
    assert psnr_h >= psnr_l2 + 10.0
    if corrupted is not None:
        wts = p.data_weights()
        hit, kept = np.mean(wts[corrupted] < 0.5), np.mean(wts[~corrupted] >= 0.5)
        print("outlier map: %.2f %% of the %d corrupted pixels below 0.5, %.2f %% of the clean ones at or above" % (
            100 * hit, int(corrupted.sum()), 100 * kept))
        assert hit >= 0.9 and kept >= 0.9


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("solver", ["cg", "lbfgs"])
def test_huber_chained_equals_host_paced(sr, ctx, proto, solver, dtype):
    name, y, _ = proto["inputs"][1]
    x0 = rr.bilinear(y[0], proto["s"])
    out = {}
    for paced in (0, 1):
        p = _gpu_problem(sr, ctx, proto, y, dtype)
        p.set_data_loss(sr.DATA_LOSS_HUBER, proto["delta"])
        if solver == "lbfgs":
            p.set_solver(sr.SOLVER_LBFGS, 5)
        o = sr.default_irls_options()
        o.max_num_irls_iterations, o.max_num_solver_iterations, o.host_paced_passes = 4, 20, paced
        x, rep = p.solve(x0, o)
        out[paced] = (x, p.data_weights(), rep.irls_rounds, rep.cg_iterations, rep.evaluations, rep.final_cost)
    assert out[0][2:] == out[1][2:]
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_huber_split_channels_equals_per_channel_solves(sr, ctx):
    rng = np.random.default_rng(77)
    s, K, W, H, Cn = 2, 4, 96, 64, 3
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    lr = rng.random((K, Cn, H // s, W // s))
    x0 = rng.random((Cn, H, W))

    def solve(y, x_start, split):
        p = sr.Problem(ctx, W, H, y.shape[1], K, s, shifts, 3, 1.0, sr.F64)
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


def test_huber_without_regulariser_runs_more_than_one_round(sr, ctx, proto):
    name, y, _ = proto["inputs"][1]
    x0 = rr.bilinear(y[0], proto["s"])
    p = _gpu_problem(sr, ctx, proto, y, reg=False)
    _, rep_l2 = p.solve(x0)
    assert rep_l2.irls_rounds == 1
    p.set_data_loss(sr.DATA_LOSS_HUBER, proto["delta"])
    x, rep = p.solve(x0)
    print("no regulariser: L2 %d round, Huber %d rounds" % (rep_l2.irls_rounds, rep.irls_rounds))
    assert rep.irls_rounds > 1 and np.all(np.isfinite(x))


def test_l2_solve_leaves_the_callers_weights_untouched(sr, ctx, proto):
    name, y, corrupted = proto["inputs"][1]
    x0 = rr.bilinear(y[0], proto["s"])
    wts = (~corrupted).astype(float)  # "ignore these pixels"
    p = _gpu_problem(sr, ctx, proto, y)
    x_plain, _ = p.solve(x0)
    p.set_data_weights(wts)
    x, rep = p.solve(x0)
    assert np.array_equal(p.data_weights(), wts)
    print("salt-and-pepper with the corrupted pixels masked: %.3f dB (unmasked %.3f dB)" % (
        orc.psnr(proto["gt"], x), orc.psnr(proto["gt"], x_plain)))
    assert orc.psnr(proto["gt"], x) >= orc.psnr(proto["gt"], x_plain) + 10.0


def test_argument_and_sharding_errors(sr, ctx):
    rng = np.random.default_rng(2)
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    p = sr.Problem(ctx, 48, 32, 1, 4, 2, shifts, 3, 1.0, sr.F64)
    y = rng.random((4, 1, 16, 24))
    p.set_observations(y)
    p.add_regularizer(sr.REG_TV, 0.01)
    for bad in (-1e-3, np.nan, np.inf):
        wts = np.ones_like(y)
        wts[1, 0, 3, 4] = bad
        with pytest.raises(sr.SrmapError) as e:
            p.set_data_weights(wts)
        assert e.value.status == sr.EINVAL
    for loss, delta in ((sr.DATA_LOSS_HUBER, 0.0), (sr.DATA_LOSS_HUBER, -1.0), (sr.DATA_LOSS_HUBER, np.nan),
                        (sr.DATA_LOSS_HUBER, np.inf), (2, 0.02), (-1, 0.02)):
        with pytest.raises(sr.SrmapError) as e:
            p.set_data_loss(loss, delta)
        assert e.value.status == sr.EINVAL
    x0 = rng.random((1, 32, 48))
    xd = _upload(sr, ctx, p, x0)
    with pytest.raises(sr.SrmapError) as e:  # the weights are re-derived for a Huber loss only
        p.update_data_weights_device(xd.value)
    assert e.value.status == sr.EINVAL
    _free(sr, ctx, xd)

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

    def refused():
        for mode in (sr.SHARD_FRAMES, sr.SHARD_ROWS, sr.SHARD_CHANNELS):
            sd = sr.ShardDesc()
            sd.mode = mode
            sd.own_row0, sd.own_row1, sd.own_ch0, sd.own_ch1 = 0, 32, 0, 1
            with pytest.raises(sr.SrmapError) as e:
                p.solve(x0, comm=comm, shard=sd)
            assert e.value.status == sr.EUNSUPPORTED
        assert fake.calls == []

    p.set_data_weights(np.ones_like(y))
    refused()
    p.set_data_weights(None)
    p.set_data_loss(sr.DATA_LOSS_HUBER, 0.02)
    refused()
    x, rep = p.solve(x0)  # unsharded it solves
    assert np.all(np.isfinite(x)) and rep.cg_iterations > 0


def test_cli_data_loss_flag(sr, ctx, tmp_path):
    """super_resolution --data_loss=huber --huber_delta=0.02: its result equals a Python Huber solve from the tool's own
    x0 (bit for bit in the float32 result file); --data_loss=bogus warns and equals --data_loss=l2."""
    import __graft_entry__ as ge
    from test_gpu_apps import _ground_truth, _read_envi, _write_envi
    ge.build_lib()
    gen, srbin = ge.build_apps()
    Cn, H, W, s, K = 1, 48, 64, 2, 4
    gt = _ground_truth(Cn, H, W)
    gt_cfg = _write_envi(str(tmp_path / "gt"), gt)
    motion = tmp_path / "motion.txt"
    motion.write_text("0 0\n1 1\n0 1\n1 0\n")
    lr_dir = tmp_path / "lr"
    lr_dir.mkdir()
    out = subprocess.run([gen, "--input_image=" + gt_cfg, "--output_image_dir=" + str(lr_dir),
                          "--motion_sequence_path=" + str(motion), "--blur_radius=3", "--blur_sigma=1.0",
                          "--downsampling_scale=%d" % s, "--number_of_frames=%d" % K],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    frames = np.stack([_read_envi(str(lr_dir / ("low_res_%d" % i)), (Cn, H // s, W // s)) for i in range(K)])
    # dead / hot pixels in the stored frames: something for the Huber loss to reject
    rng = np.random.default_rng(4)
    hot = rng.random(frames.shape) < 0.03
    frames = np.where(hot, rng.integers(0, 2, frames.shape).astype(float), frames)
    for i in range(K):
        frames[i].astype("<f4").tofile(str(lr_dir / ("low_res_%d" % i)))  # the raw cube; its .config stays
    frames = np.stack([_read_envi(str(lr_dir / ("low_res_%d" % i)), (Cn, H // s, W // s)) for i in range(K)])

    def run(loss):
        res = str(tmp_path / ("result_" + loss))
        o = subprocess.run([srbin, "--data_path=" + str(lr_dir), "--upsampling_scale=%d" % s, "--blur_radius=3",
                            "--blur_sigma=1.0", "--motion_sequence_path=" + str(motion), "--regularizer=btv",
                            "--btv_scale_range=2", "--regularization_parameter=0.005", "--optimization_iterations=5",
                            "--solver_iterations=30", "--data_loss=" + loss, "--huber_delta=0.02", "--result_path=" + res,
                            "--save_initial_estimate=" + str(tmp_path / ("x0_" + loss))],
                           capture_output=True, text=True, timeout=600)
        print(o.stdout, o.stderr)
        assert o.returncode == 0
        return res, o.stderr

    res_h, err_h = run("huber")
    assert "WARNING" not in err_h
    x0 = np.fromfile(str(tmp_path / "x0_huber"), dtype=np.float64).reshape(Cn, H, W)
    p = sr.Problem(ctx, W, H, Cn, K, s, [[0, 0], [1, 1], [0, 1], [1, 0]], 3, 1.0, sr.F64)
    p.set_observations(frames)
    p.add_regularizer(sr.REG_BTV, 0.005, 2, 0.5)
    p.set_data_loss(sr.DATA_LOSS_HUBER, 0.02)
    o = sr.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = 5, 30
    x, _ = p.solve(x0, o)
    cli = np.fromfile(res_h, dtype="<f4").reshape(Cn, H, W)
    assert np.array_equal(x.astype(np.float32), cli)
    res_l2, err_l2 = run("l2")
    res_bogus, err_bogus = run("bogus")
    assert "WARNING" not in err_l2 and "WARNING" in err_bogus
    assert open(res_l2, "rb").read() == open(res_bogus, "rb").read()
    assert open(res_l2, "rb").read() != open(res_h, "rb").read()
