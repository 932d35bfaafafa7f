"""The residual scale on the GPU (include/srmap.h: srmap_residual_scale*, srmap_problem_set_huber_scale,
srmap_problem_get_huber_delta; k_select_hist / k_select_pick / k_select_finish of csrc/residual_scale.hip, the DELTA_DEV
instances of k_huber_weights) against its numpy restatement (tests/residual_scale_restatement.py: np.partition).

Exactness: with x = 0 the model gives A x = 0 exactly, so r = -y and the test owns |r| through y rounded to the dtype; the
scale must then EQUAL 1.4826 x the numpy lower median and the counts must be equal.  On a general x the order statistic
is 1-Lipschitz in the residuals (tests/test_residual_scale_cpu.py), so the scale inherits the residuals' parity bar:
1.4826 x 1e-12 (f64) / 2e-5 (f32), residuals in (-1, 1)."""
import os
import sys

import numpy as np
import pytest

import oracle as orc
import parity_log

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import residual_scale_restatement as rs  # noqa: E402
import robust_restatement as rr  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = {0: 1e-12, 1: 2e-5}
NP = {0: np.float64, 1: np.float32}
TUNING, FLOOR = 1.345, 1e-4


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


def _shifts(K, subpixel=False, seed=0):
    rng = np.random.default_rng(seed)
    if subpixel:
        return [[0.0, 0.0]] + [[float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2))] for _ in range(K - 1)]
    return [[0, 0]] + [[int(rng.integers(-2, 3)), int(rng.integers(-2, 3))] for _ in range(K - 1)]


def _problem(sr, ctx, K, Cn, h, w, dtype, scale=2, blur=3, subpixel=False):
    return sr.Problem(ctx, w * scale, h * scale, Cn, K, scale, _shifts(K, subpixel), blur, 1.0 if blur else 0.0, dtype)


def _destroy(sr, p):
    sr.load().srmap_problem_destroy(p._h)
    p._h = None


def _tensor(x, dtype):
    import torch
    t = torch.tensor(np.asarray(x), dtype=torch.float32 if dtype else torch.float64, device="cuda")
    torch.cuda.synchronize()
    return t


def _expect(y, dtype, mask=None):
    """scales and counts of r = -y, y rounded to the dtype."""
    return rs.residual_scales(np.asarray(y).astype(NP[dtype]), mask)


def _assert_exact(tag, got, want):
    (s, c), (ws, wc) = got, want
    assert np.array_equal(c, wc), (tag, c, wc)
    assert np.array_equal(s, ws), (tag, s, ws)


# ------------------------------------------------------------------------------------------------ exactness
# LR sizes; the last three hold, per frame, exactly one workgroup's worth of 16-byte groups (256 groups: 512 doubles / 1024
# floats), one element fewer and one more
SIZES = [(5, 7), (17, 23), (70, 129)]
GROUP_SIZES = {0: [(16, 32), (7, 73), (19, 27)], 1: [(32, 32), (31, 33), (25, 41)]}


def _exactness(sr, ctx, K, Cn, h, w, dtype):
    p = _problem(sr, ctx, K, Cn, h, w, dtype)
    x0 = np.zeros((Cn, 2 * h, 2 * w))
    shape = (K, Cn, h, w)
    n = int(np.prod(shape))
    rng = np.random.default_rng(1000 * K + 100 * Cn + h + dtype)
    for name, v in rs.patterns(NP[dtype], n, rng, denormals=False).items():
        y = v.astype(np.float64).reshape(shape)
        p.set_observations(y)
        _assert_exact("%s" % name, p.residual_scale(x0), _expect(y, dtype))
    y = rng.standard_normal(shape)
    p.set_observations(y)
    wts = rng.random(shape) * (rng.random(shape) < 0.7)
    binary = (rng.random(shape) < 0.5).astype(float)
    frame_off = np.ones(shape)
    frame_off[K // 2] = 0.0
    p.set_data_weights(wts)
    _assert_exact("user weights with zeros, L2", p.residual_scale(x0), _expect(y, dtype, wts))
    p.set_data_weights(None)
    for tag, m in (("binary prior", binary), ("a prior that zeroes a frame", frame_off), ("both", binary * frame_off)):
        p.set_data_prior(m)
        for loss in (sr.DATA_LOSS_L2, sr.DATA_LOSS_HUBER):
            p.set_data_loss(loss, 0.1)
            got = p.residual_scale(x0)
            _assert_exact("%s, loss %d" % (tag, loss), got, _expect(y, dtype, m))
        p.set_data_loss(sr.DATA_LOSS_L2)
        if m is not binary:
            s, c = got
            assert s[1 + K // 2] == 0.0 and c[1 + K // 2] == 0.0
            assert K == 1 or (s[0] > 0.0 and c[0] > 0.0)
    p.set_data_prior(wts)  # under L2 the effective weights m .* w count
    p.set_data_weights(binary)
    _assert_exact("prior and weights, L2", p.residual_scale(x0), _expect(y, dtype, wts * binary))
    p.set_data_prior(None)
    p.set_data_weights(None)
    p.set_data_loss(sr.DATA_LOSS_HUBER, 0.1)  # Huber without a prior: every observation counts, whatever the weights hold
    _assert_exact("Huber, no prior", p.residual_scale(x0), _expect(y, dtype))
    _destroy(sr, p)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("size", SIZES)
def test_scale_equals_the_numpy_lower_median(sr, ctx, size, K, Cn, dtype):
    _exactness(sr, ctx, K, Cn, size[0], size[1], dtype)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_scale_at_one_workgroup_of_16_byte_groups(sr, ctx, which, dtype):
    h, w = GROUP_SIZES[dtype][which]
    assert h * w == 256 * (4 if dtype else 2) + (0, -1, 1)[which]
    _exactness(sr, ctx, 3, 1, h, w, dtype)


# ------------------------------------------------------------------------------------------------ a general x
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("blur", [0, 3])
@pytest.mark.parametrize("subpixel", [False, True])
def test_scale_on_a_general_x_matches_the_restatement(sr, ctx, subpixel, blur, dtype):
    K, Cn, h, w, s = 5, 2, 29, 75, 3
    rng = np.random.default_rng(10 * blur + subpixel)
    shifts = _shifts(K, subpixel)
    model = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=blur, blur_sigma=1.0 if blur else 0.0)
    y, x = rng.random((K, Cn, h, w)), rng.random((Cn, h * s, w * s))
    mask = (rng.random(y.shape) < 0.8).astype(float)
    r = rr.residuals(model, y, x)
    p = sr.Problem(ctx, w * s, h * s, Cn, K, s, shifts, blur, 1.0 if blur else 0.0, dtype)
    p.set_observations(y)
    for m in (None, mask):
        p.set_data_prior(m)
        (sc, cn), (ws, wc) = p.residual_scale(x), rs.residual_scales(r, m)
        e = parity_log.note(np.max(np.abs(sc - ws)), "scale")
        print("subpixel %d blur %d f%d mask %d: max |scale - ref| %.3e (bar %.3e)" % (subpixel, blur, 32 if dtype else 64,
                                                                                     m is not None, e, 1.4826 * BAR[dtype]))
        assert np.array_equal(cn, wc)
        assert e <= 1.4826 * BAR[dtype]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("what", ["affine", "flow", "blur kernel", "photometric"])
def test_scale_under_every_model_state(sr, ctx, what, dtype):
    """Affine motion, a displacement field, a free-form 5 x 5 blur, photometric parameters: the scale of the residuals of
    each model's own numpy restatement (tests/affine_restatement.py, flow_restatement.py, blur_kernel_restatement.py,
    photometric_restatement.py), within the same bar."""
    import affine_restatement as ar
    import blur_kernel_restatement as bk
    import flow_restatement as fr
    import photometric_restatement as pr
    K, Cn, h, w, s = 4, 1, 31, 45, 2
    H, W = h * s, w * s
    rng = np.random.default_rng(7)
    shifts = _shifts(K, what == "photometric")
    p = sr.Problem(ctx, W, H, Cn, K, s, shifts, 3, 1.0, dtype)
    y, x = rng.random((K, Cn, h, w)), rng.random((Cn, H, W))
    yn = y
    if what == "affine":
        mats = np.tile(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (K, 1, 1))
        mats[1:] += np.concatenate([0.02 * rng.standard_normal((K - 1, 2, 2)), rng.uniform(-1.5, 1.5, (K - 1, 2, 1))], axis=2)
        p.set_affine_motion(mats)
        model = ar.AffineImageModel(s, mats, 3, 1.0)
    elif what == "flow":
        v, u = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
        fields = np.stack([np.stack([0.3 * k * np.sin(2 * u + k), 0.2 * k * np.cos(3 * v)]) for k in range(K)])
        p.set_flow(fields)
        model = fr.gaussian_model(s, fields, 3, 1.0, dtype=NP[dtype])
    elif what == "blur kernel":
        taps = rng.random((5, 5))
        taps /= taps.sum()
        p.set_blur_kernel(taps)
        model = bk.BlurKernelModel(s, K, H, W, taps, motion=("shifts", shifts))
    else:
        gb = np.stack([rng.uniform(0.7, 1.4, K), rng.uniform(-0.1, 0.1, K)], axis=1)
        p.set_photometric(gb)
        model = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=3, blur_sigma=1.0)
        yn = pr.normalise(y, gb, NP[dtype]).astype(np.float64)
    p.set_observations(y)
    r = rr.residuals(model, yn, x)
    (sc, cn), (ws, wc) = p.residual_scale(x), rs.residual_scales(r)
    e = parity_log.note(np.max(np.abs(sc - ws)), "scale")
    print("%s f%d: max |scale - ref| %.3e" % (what, 32 if dtype else 64, e))
    assert np.array_equal(cn, wc) and e <= 1.4826 * BAR[dtype]


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("dtype", [0, 1])
def test_repeats_permutations_and_the_device_form(sr, ctx, dtype):
    K, Cn, h, w, s = 5, 2, 23, 37, 2
    rng = np.random.default_rng(3)
    shifts = _shifts(K, True)
    y, x = rng.random((K, Cn, h, w)), rng.random((Cn, h * s, w * s))
    mask = (rng.random(y.shape) < 0.7).astype(float)

    def scales(order, device=False):
        p = sr.Problem(ctx, w * s, h * s, Cn, K, s, [shifts[k] for k in order], 3, 1.0, dtype)
        p.set_observations(y[order])
        p.set_data_prior(mask[order])
        return p.residual_scale(_tensor(x, dtype) if device else x), p

    (s0, c0), p = scales(list(range(K)))
    for _ in range(3):  # repeats are bit-identical
        s1, c1 = p.residual_scale(x)
        assert np.array_equal(s1, s0) and np.array_equal(c1, c0)
    (sd, cd), _ = scales(list(range(K)), device=True)  # a host array and a device tensor
    assert np.array_equal(sd, s0) and np.array_equal(cd, c0)
    order = [3, 0, 4, 2, 1]
    (sp, cp), _ = scales(order)  # a permuted stack: the permuted frame scales, the IDENTICAL global one
    assert sp[0] == s0[0] and cp[0] == c0[0]
    assert np.array_equal(sp[1:], s0[1:][order]) and np.array_equal(cp[1:], c0[1:][order])


# ------------------------------------------------------------------------------------------------ the step
def _step(sr, ctx, p, x, dtype):
    xd = _tensor(x, dtype)
    p.update_data_weights_device(xd.data_ptr())
    out = p.data_weights()  # waits for the step
    del xd
    return out


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("prior", [False, True])
def test_mad_step_equals_a_fixed_step_given_its_delta(sr, ctx, prior, Cn, dtype):
    K, h, w, s = 4, 27, 41, 2
    rng = np.random.default_rng(Cn + 10 * prior)
    y, x = rng.random((K, Cn, h, w)), 0.5 + 0.1 * rng.random((Cn, h * s, w * s))
    m = (rng.random(y.shape) < 0.75).astype(float) * (0.5 + rng.random(y.shape))
    twins = []
    for _ in range(2):
        p = _problem(sr, ctx, K, Cn, h, w, dtype, subpixel=True)
        p.set_observations(y)
        p.set_data_loss(sr.DATA_LOSS_HUBER, 0.02)
        if prior:
            p.set_data_prior(m)
        twins.append(p)
    auto, fixed = twins
    auto.set_huber_scale(sr.HUBER_DELTA_MAD, TUNING, FLOOR)
    w_auto = _step(sr, ctx, auto, x, dtype)
    mode, delta, scales, counts = auto.huber_delta()
    s_diag, c_diag = auto.residual_scale(x)
    assert mode == sr.HUBER_DELTA_MAD
    assert delta == max(TUNING * s_diag[0], FLOOR) and delta > FLOOR
    assert np.array_equal(scales, s_diag) and np.array_equal(counts, c_diag)
    assert counts[0] == (np.sum(m > 0) if prior else y.size)
    assert fixed.huber_delta()[:2] == (sr.HUBER_DELTA_FIXED, 0.02) and not np.any(fixed.huber_delta()[2])
    fixed.set_data_loss(sr.DATA_LOSS_HUBER, delta)
    w_fixed = _step(sr, ctx, fixed, x, dtype)
    assert np.array_equal(w_auto, w_fixed)
    down = np.mean(w_auto[m > 0] < m[m > 0]) if prior else np.mean(w_auto < 1.0)  # both branches of the weight at work
    assert 0.05 < down < 0.95, down
    # the mode persists across the loss, weight and prior calls
    auto.set_data_loss(sr.DATA_LOSS_L2)
    auto.set_data_weights(None)
    auto.set_data_prior(None)
    auto.set_data_loss(sr.DATA_LOSS_HUBER, 0.5)
    assert auto.huber_delta()[0] == sr.HUBER_DELTA_MAD


@pytest.mark.parametrize("dtype", [0, 1])
def test_the_floor_takes_over_on_a_perfect_fit(sr, ctx, dtype):
    K, Cn, h, w, s = 3, 1, 16, 24, 2
    rng = np.random.default_rng(4)
    gt = rng.random((Cn, h * s, w * s))
    p = _problem(sr, ctx, K, Cn, h, w, dtype)
    y = np.stack([p.apply(gt, k) for k in range(K)])
    p.set_observations(y)
    p.set_data_loss(sr.DATA_LOSS_HUBER, 0.02)
    p.set_huber_scale(sr.HUBER_DELTA_MAD, TUNING, FLOOR)
    wts = _step(sr, ctx, p, gt, dtype)
    mode, delta, scales, counts = p.huber_delta()
    print("perfect fit f%d: scale %.3e, delta %.3e" % (32 if dtype else 64, scales[0], delta))
    assert TUNING * scales[0] < FLOOR and delta == FLOOR and counts[0] == y.size
    assert np.array_equal(wts, np.ones_like(y))


def test_split_channels_estimates_delta_per_channel(sr, ctx):
    """A split_channels solve re-weights through a channel view: bit for bit three one-channel problems, so every channel
    took the delta of its own residuals."""
    rng = np.random.default_rng(77)
    s, K, W, H, Cn = 2, 4, 90, 62, 3  # 45 x 31 LR: a channel's run starts off a 16-byte boundary
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    lr = rng.random((K, Cn, H // s, W // s)) * np.array([0.2, 1.0, 3.0])[None, :, None, None]
    x0 = rng.random((Cn, H, W))
    m = (rng.random(lr.shape) < 0.8).astype(float)

    def solve(y, x_start, prior, split):
        p = sr.Problem(ctx, W, H, y.shape[1], K, s, shifts, 3, 1.0, sr.F64)
        p.set_observations(y)
        p.add_regularizer(sr.REG_TV, 0.01)
        p.set_data_loss(sr.DATA_LOSS_HUBER, 0.1)
        p.set_data_prior(prior)
        p.set_huber_scale(sr.HUBER_DELTA_MAD, TUNING, FLOOR)
        o = sr.default_irls_options()
        o.split_channels, o.max_num_irls_iterations = split, 3
        x, rep = p.solve(x_start, o)
        return x, rep, p.data_weights(), p.huber_delta()[1]

    x, rep, wts, delta = solve(lr, x0, m, 1)
    deltas = []
    for c in range(Cn):
        xc, rc, wc, dc = solve(lr[:, c:c + 1], x0[c:c + 1], m[:, c:c + 1], 0)
        assert np.array_equal(x[c:c + 1], xc), c
        assert np.array_equal(wts[:, c:c + 1], wc), c
        deltas.append(dc)
    assert delta == deltas[-1] and deltas[0] < deltas[1] < deltas[2]


# ------------------------------------------------------------------------------------------------ unchanged paths
@pytest.mark.parametrize("dtype", [0, 1])
def test_mad_and_back_to_fixed_is_the_untouched_problem(sr, ctx, dtype):
    lib = sr.load()
    start = int(lib.srmap_live_allocations())
    K, Cn, h, w, s = 4, 2, 24, 40, 2
    rng = np.random.default_rng(8)
    y, x0 = rng.random((K, Cn, h, w)), rng.random((Cn, h * s, w * s))
    out = []
    for touched in (False, True):
        p = _problem(sr, ctx, K, Cn, h, w, dtype)
        p.set_observations(y)
        p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.5)
        p.set_data_loss(sr.DATA_LOSS_HUBER, 0.05)
        o = sr.default_irls_options()
        o.max_num_irls_iterations, o.max_num_solver_iterations = 3, 15
        if touched:
            p.set_huber_scale(sr.HUBER_DELTA_MAD, TUNING, FLOOR)
            xm, _ = p.solve(x0, o)
            p.residual_scale(xm)
            p.set_huber_scale(sr.HUBER_DELTA_FIXED, 0.0, 0.0)
        x, rep = p.solve(x0, o)
        out.append((x, p.data_weights(), rep.irls_rounds, rep.cg_iterations, rep.evaluations, rep.final_cost))
        _destroy(sr, p)
    assert out[0][2:] == out[1][2:]
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert int(lib.srmap_live_allocations()) == start


# ------------------------------------------------------------------------------------------------ solves
@pytest.fixture(scope="module")
def proto():
    return rr.prototype_inputs()


def _perturbed(x0):
    return x0 * (1 + 1e-14 * np.random.default_rng(1).standard_normal(x0.shape))


def _gpu_mad_solve(sr, ctx, proto, y, x0, solver):
    p = sr.Problem(ctx, proto["W"], proto["H"], proto["C"], proto["K"], proto["s"], proto["shifts"], proto["blur"][0],
                   proto["blur"][1], sr.F64)
    p.set_observations(y)
    p.add_regularizer(*proto["reg"])
    p.set_data_loss(sr.DATA_LOSS_HUBER, proto["delta"])
    p.set_huber_scale(sr.HUBER_DELTA_MAD, TUNING, FLOOR)
    if solver == "lbfgs":
        p.set_solver(sr.SOLVER_LBFGS, 5)
    x, rep = p.solve(x0)
    return x, rep, p.huber_delta()


@pytest.mark.parametrize("solver", ["cg", "lbfgs"])
def test_mad_solve_matches_the_restatement_on_the_noise_input(sr, ctx, proto, solver):
    """Noise-only input, the rules of tests/test_gpu_robust.py: identical rounds / iterations / evaluations; the final delta
    within ten times the restatement's own movement under a 1e-14 relative perturbation of the start (or 1e-9)."""
    name, y, _ = proto["inputs"][0]
    x0 = rr.bilinear(y[0], proto["s"])
    kw = dict(solver=solver, m=5, tuning=TUNING, min_delta=FLOOR)
    x_ref, rep_ref, _, d_ref, _ = rs.irls_solve_mad(proto["model"], y, x0, proto["reg"], **kw)
    x_p, rep_p, _, d_p, _ = rs.irls_solve_mad(proto["model"], y, _perturbed(x0), proto["reg"], **kw)
    own_x, own_d = np.max(np.abs(x_p - x_ref)), abs(d_p[-1] - d_ref[-1])
    x, rep, (mode, delta, scales, counts) = _gpu_mad_solve(sr, ctx, proto, y, x0, solver)
    dx, dd = np.max(np.abs(x - x_ref)), abs(delta - d_ref[-1])
    print("%s: rounds %d/%d iterations %d/%d evaluations %d/%d; x %.3e (own %.3e); delta %.9g / %.9g: %.3e (own %.3e); "
          "PSNR %.3f / %.3f dB" % (solver, rep.irls_rounds, rep_ref.irls_rounds, rep.cg_iterations, rep_ref.cg_iterations,
                                   rep.evaluations, rep_ref.nfev, dx, own_x, delta, d_ref[-1], dd, own_d,
                                   orc.psnr(proto["gt"], x), orc.psnr(proto["gt"], x_ref)))
    assert (rep.irls_rounds, rep.cg_iterations, rep.evaluations) == (rep_ref.irls_rounds, rep_ref.cg_iterations, rep_ref.nfev)
    assert dx <= max(1e-7, 10 * own_x)
    assert dd <= max(1e-9, 10 * own_d)
    assert counts[0] == y.size and np.all(counts[1:] == y[0].size)


@pytest.mark.parametrize("solver", ["cg", "lbfgs"])
@pytest.mark.parametrize("which", [1, 2, 3, 4])
def test_mad_solve_on_the_outlier_inputs(sr, ctx, proto, which, solver):
    """Salt-and-pepper / misregistered frame / salt-and-pepper at noise 0.003 (delta falls to 0.0036) and 0.03 (the longest
    chain of select -> delta -> weights steps): PSNR within max(0.01 dB, 10 x the restatement's own movement under a 1e-14
    relative perturbation of the start) of the restatement's, the final delta within ten times its own movement (or 1e-9);
    the misregistered frame's scale stands out; at noise 0.03 the round count is the restatement's."""
    inputs = [(n, y) for n, y, _ in proto["inputs"]] + [("salt_pepper sigma 0.003", rs.seed11_input(0.003)),
                                                        ("salt_pepper sigma 0.03", rs.seed11_input(0.03))]
    name, y = inputs[which]
    gt = proto["gt"]
    x0 = rr.bilinear(y[0], proto["s"])
    kw = dict(solver=solver, m=5, tuning=TUNING, min_delta=FLOOR)
    x_ref, rep_ref, _, d_ref, f_ref = rs.irls_solve_mad(proto["model"], y, x0, proto["reg"], **kw)
    x_p, rep_p, _, d_p, _ = rs.irls_solve_mad(proto["model"], y, _perturbed(x0), proto["reg"], **kw)
    own, own_d = abs(orc.psnr(gt, x_p) - orc.psnr(gt, x_ref)), abs(d_p[-1] - d_ref[-1])
    x, rep, (mode, delta, scales, counts) = _gpu_mad_solve(sr, ctx, proto, y, x0, solver)
    print("%s %s: GPU %.3f dB (%d / %d / %d), restatement %.3f dB (%d / %d / %d; perturbed %d / %d / %d), own movement %.4f dB; "
          "delta %.6f / %.6f (own %.2e); frame scales %s" % (
              name, solver, orc.psnr(gt, x), rep.irls_rounds, rep.cg_iterations, rep.evaluations, orc.psnr(gt, x_ref),
              rep_ref.irls_rounds, rep_ref.cg_iterations, rep_ref.nfev, rep_p.irls_rounds, rep_p.cg_iterations, rep_p.nfev, own,
              delta, d_ref[-1], own_d, " ".join("%.4f" % v for v in scales[1:])))
    parity_log.note(abs(orc.psnr(gt, x) - orc.psnr(gt, x_ref)), "psnr")
    assert abs(orc.psnr(gt, x) - orc.psnr(gt, x_ref)) <= max(0.01, 10 * own)
    assert abs(delta - d_ref[-1]) <= max(1e-9, 10 * own_d)
    assert counts[0] == y.size
    if which == 2:
        assert scales[5] >= 2.0 * np.median(np.delete(scales[1:], 4))
    if which == 4:
        assert rep.irls_rounds == rep_ref.irls_rounds


# ------------------------------------------------------------------------------------------------ errors
def test_argument_and_sharding_errors(sr, ctx):
    rng = np.random.default_rng(2)
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    lib = sr.load()
    p = sr.Problem(ctx, 48, 32, 1, 4, 2, shifts, 3, 1.0, sr.F64)
    x0 = rng.random((1, 32, 48))
    with pytest.raises(sr.SrmapError) as e:  # no observations
        p.residual_scale(x0)
    assert e.value.status == sr.EINVAL
    with pytest.raises(sr.SrmapError) as e:
        p.residual_scale(_tensor(x0, 0))
    assert e.value.status == sr.EINVAL
    y = rng.random((4, 1, 16, 24))
    p.set_observations(y)
    p.add_regularizer(sr.REG_TV, 0.01)
    for mode, tuning, floor in ((2, 1.345, 1e-4), (-1, 1.345, 1e-4), (1, 0.0, 1e-4), (1, -1.0, 1e-4), (1, np.nan, 1e-4),
                                (1, np.inf, 1e-4), (1, 1.345, 0.0), (1, 1.345, -1e-4), (1, 1.345, np.nan), (1, 1.345, np.inf)):
        with pytest.raises(sr.SrmapError) as e:
            p.set_huber_scale(mode, tuning, floor)
        assert e.value.status == sr.EINVAL
    assert p.huber_delta()[0] == sr.HUBER_DELTA_FIXED  # a refused call changes nothing
    sc = np.zeros(5)
    px, ps = x0.ctypes.data_as(sr.c_double_p), sc.ctypes.data_as(sr.c_double_p)
    assert lib.srmap_problem_set_huber_scale(None, 1, 1.345, 1e-4) == sr.EINVAL
    assert lib.srmap_problem_get_huber_delta(None, None, None, None, None) == sr.EINVAL
    assert lib.srmap_problem_get_huber_delta(p.handle, None, None, None, None) == sr.OK  # every output is optional
    assert lib.srmap_residual_scale(None, px, ps, None) == sr.EINVAL
    assert lib.srmap_residual_scale(p.handle, None, ps, None) == sr.EINVAL
    assert lib.srmap_residual_scale(p.handle, px, None, None) == sr.EINVAL
    assert lib.srmap_residual_scale(p.handle, px, ps, None) == sr.OK  # the counts are optional
    assert lib.srmap_residual_scale_device(None, None, None, ps, None) == sr.EINVAL
    assert lib.srmap_residual_scale_device(p.handle, None, None, ps, None) == sr.EINVAL
    assert sc[0] > 0.0

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
    p.set_data_loss(sr.DATA_LOSS_HUBER, 0.02)
    p.set_huber_scale(sr.HUBER_DELTA_MAD, TUNING, FLOOR)
    for mode in (sr.SHARD_FRAMES, sr.SHARD_ROWS, sr.SHARD_CHANNELS):
        sd = sr.ShardDesc()
        sd.mode = mode
        sd.own_row0, sd.own_row1, sd.own_ch0, sd.own_ch1 = 0, 32, 0, 1
        with pytest.raises(sr.SrmapError) as e:
            p.solve(x0, comm=comm, shard=sd)
        assert e.value.status == sr.EUNSUPPORTED
    assert fake.calls == []
    x, rep = p.solve(x0)  # unsharded it solves
    assert np.all(np.isfinite(x)) and rep.cg_iterations > 0 and p.huber_delta()[1] >= FLOOR


# ------------------------------------------------------------------------------------------------ the tool and the facade
def test_cli_huber_scale_flags(sr, ctx, tmp_path):
    """super_resolution --data_loss=huber --huber_scale=mad (through IRLSMapSolverOptions::huber_scale and
    IRLSMapSolver::ResidualScale / HuberDelta): its result equals a Python MAD solve from the tool's own x0, bit for bit in
    the float32 result file, and the scales it prints are the Python route's; --huber_scale=bogus warns and equals fixed."""
    import re
    import subprocess
    import __graft_entry__ as ge
    from test_gpu_apps import _ground_truth, _read_envi, _write_envi
    ge.build_lib()
    gen, srbin = ge.build_apps()
    Cn, H, W, s, K = 1, 48, 64, 2, 4
    gt_cfg = _write_envi(str(tmp_path / "gt"), _ground_truth(Cn, H, W))
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
    rng = np.random.default_rng(4)
    hot = rng.random(frames.shape) < 0.03
    frames = np.where(hot, rng.integers(0, 2, frames.shape).astype(float), frames + 0.01 * rng.standard_normal(frames.shape))
    for i in range(K):
        frames[i].astype("<f4").tofile(str(lr_dir / ("low_res_%d" % i)))  # the raw cube; its .config stays
    frames = np.stack([_read_envi(str(lr_dir / ("low_res_%d" % i)), (Cn, H // s, W // s)) for i in range(K)])

    def run(scale):
        res = str(tmp_path / ("result_" + scale))
        o = subprocess.run([srbin, "--data_path=" + str(lr_dir), "--upsampling_scale=%d" % s, "--blur_radius=3",
                            "--blur_sigma=1.0", "--motion_sequence_path=" + str(motion), "--regularizer=btv",
                            "--btv_scale_range=2", "--regularization_parameter=0.005", "--optimization_iterations=5",
                            "--solver_iterations=30", "--data_loss=huber", "--huber_delta=0.02", "--huber_scale=" + scale,
                            "--huber_tuning=1.5", "--huber_min_delta=0.001", "--print_residual_scale", "--result_path=" + res,
                            "--save_initial_estimate=" + str(tmp_path / ("x0_" + scale))],
                           capture_output=True, text=True, timeout=600)
        print(o.stdout, o.stderr)
        assert o.returncode == 0
        return res, o.stdout, o.stderr

    res_m, out_m, err_m = run("mad")
    assert "WARNING" not in err_m
    x0 = np.fromfile(str(tmp_path / "x0_mad"), dtype=np.float64).reshape(Cn, H, W)
    p = sr.Problem(ctx, W, H, Cn, K, s, [[0, 0], [1, 1], [0, 1], [1, 0]], 3, 1.0, sr.F64)
    p.set_observations(frames)
    p.add_regularizer(sr.REG_BTV, 0.005, 2, 0.5)
    p.set_data_loss(sr.DATA_LOSS_HUBER, 0.02)
    p.set_huber_scale(sr.HUBER_DELTA_MAD, 1.5, 0.001)
    o = sr.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = 5, 30
    x, _ = p.solve(x0, o)
    assert np.array_equal(x.astype(np.float32), np.fromfile(res_m, dtype="<f4").reshape(Cn, H, W))
    delta = float(re.search(r"Huber delta of the last re-weighting: (\S+)", out_m).group(1))
    assert delta == pytest.approx(p.huber_delta()[1], rel=1e-8) and delta > 0.001
    printed = [float(v) for v in re.findall(r"(?:over all frames|frame \d+): (\S+)", out_m)]
    scales, _ = p.residual_scale(x)
    assert len(printed) == 1 + K and printed == pytest.approx(list(scales), rel=1e-7)
    res_f, out_f, err_f = run("fixed")
    res_b, out_b, err_b = run("bogus")
    assert "WARNING" not in err_f and "WARNING" in err_b
    assert open(res_f, "rb").read() == open(res_b, "rb").read()
    assert open(res_f, "rb").read() != open(res_m, "rb").read()
    assert "Huber delta of the last re-weighting" not in out_f
