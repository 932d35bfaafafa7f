"""The blur-kernel bank and its per-entry calibration fit on the GPU (include/srmap.h: srmap_problem_set_blur_bank,
srmap_problem_get_blur_bank, srmap_fit_blur_bank; the bank legs of k_forward_direct, k_gather_direct, k_gather_sampled,
k_refine_sums, k_photometric_sums and the per-channel grid of k_blur_fit_sums, k_fit_reduce) against the numpy
restatement (tests/blur_bank_restatement.py), against the single free-form kernel and against itself.

Bars.  Evaluations: the project's per-element bars, 1e-12 (f64) and 2e-5 (f32), every comparison through parity_log.  Fit
sums, f64: each block of an entry's Gram (G, b, y.y) is held to 100 x the restatement's own sensitivity to the ORDER of its
sums, floor 1e-13 of the block's largest magnitude (section 3.8's bar); f32: 2e-5 of the block's largest magnitude against
the restatement given the f32-rounded inputs.  Taps: 100 x the restatement's order sensitivity of the taps, floor 1e-10.
The dependent fits keep the bars of their own GPU tests (tests/test_gpu_motion_refinement.py, tests/test_gpu_photometric.py).
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import blur_bank_restatement as bb  # noqa: E402
import blur_kernel_restatement as bk  # noqa: E402
import flow_restatement as fr  # noqa: E402
import motion_refinement_restatement as mr  # noqa: E402
import parity_log as pl  # noqa: E402
import photometric_restatement as pr  # noqa: E402
import robust_restatement as rr  # noqa: E402
import test_blur_bank_cpu as cpu  # noqa: E402
import test_gpu_photometric as tp  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ["frame", "channel", "frame_channel"]
MOTIONS = ["none", "shifts", "affine", "flow"]
WEIGHTS = [None, "random", "mask", "huber"]
# LR shape, scale, ksize, K, C: walked through by the case number, so that every mode x motion x weights meets several
SHAPES = [((5, 7), 2, 7, 2, 3), ((9, 13), 3, 3, 5, 1), ((17, 23), 2, 5, 2, 1), ((9, 13), 2, 1, 5, 3), ((5, 7), 3, 5, 5, 3),
          ((17, 23), 3, 7, 2, 3), ((9, 13), 2, 5, 2, 3)]
HUBER_DELTA = 0.1


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


def f32r(a):
    return None if a is None else np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def upload(sr, ctx, p, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    ptr = C.c_void_p()
    ctx.check(sr.load().srmap_device_alloc(ctx._h, a.size * 8, C.byref(ptr)))
    ctx.check(sr.load().srmap_upload(p.handle, a.ctypes.data_as(sr.c_double_p), ptr, a.size))
    return ptr


def free(sr, ctx, ptr):
    ctx.check(sr.load().srmap_device_free(ctx._h, ptr))


def make_motion(kind, rng, K, W, H, f32=False):
    """(restatement motion, shifts or None, affine matrices or None, displacement fields or None)."""
    if kind == "none":
        return None, None, None, None
    sh = [[0, 0], [1.25, -.75], [-.5, 2.03125], [2, -1], [-1.59375, .5]][:K]
    if kind == "shifts":
        return ("shifts", sh), sh, None, None
    if kind == "affine":
        mats = np.stack([ar.random_matrix(rng, ar.MAX_DEVIATION, shift=2.0, at_bound=True) if k % 2 else ar.random_matrix(rng, 0.2, shift=2.0)
                         for k in range(K)])
        return ("affine", mats), None, mats, None
    # a flow: smooth fields about uniform offsets, the second frame's 2.6 px to the right and down, which pushes the
    # samples of its last columns and rows outside the image
    off = [[0.3, -0.2], [-2.6, -2.6], [0.5, 1.25], [-1.0, 0.4], [1.6, -0.5]][:K]
    fields = fr.from_shifts(off, H, W) + np.stack([fr.smooth_random(rng, H, W, 0.3, spacing=8) for _ in range(K)])
    return ("flow", fr.stored(fields, np.float32 if f32 else np.float64)), None, None, fields


def make_bank(rng, mode, K, Cn, ksize):
    """Asymmetric entries, all different, with negative taps; no normalisation.  The taps scale with 1 / ksize so that a
    blurred value stays of the order of a pixel value at every size: the bars are relative to max(1, |reference|), and with
    49 taps of order 1 at scale 3 the f32 rounding of the gradient's sums of order 100 sits at the 2e-5 bar (2.2e-5 was
    measured there)."""
    lead = (K, Cn) if mode == "frame_channel" else ((K,) if mode == "frame" else (Cn,))
    return rng.uniform(-0.5, 1.0, lead + (ksize, ksize)) / ksize


def make_weights(kind, rng, shape):
    if kind == "random":
        return 0.1 + rng.random(shape)
    if kind == "mask":
        w = (rng.random(shape) < 0.7).astype(np.float64)
        w[1] = 0.0  # a whole frame masked out
        return w
    return None


def make_problem(sr, ctx, lr_shape, s, Cn, K, dtype, shifts, mats, fields, blur=(3, 1.0)):
    h, w = lr_shape
    p = sr.Problem(ctx, w * s, h * s, Cn, K, s, shifts, blur[0], blur[1], sr.F32 if dtype == "f32" else sr.F64)
    if mats is not None:
        p.set_affine_motion(mats)
    if fields is not None:
        p.set_flow(fields)
    return p


def mode_id(sr, mode):
    return {"frame": sr.BLUR_PER_FRAME, "channel": sr.BLUR_PER_CHANNEL, "frame_channel": sr.BLUR_PER_FRAME_CHANNEL}[mode]


def check_parity(p, model, x, y, wts, r, K, tol, tag, rows=None, sr=None):
    f_ref, g_ref = model.data_term(y, wts, x, cost_rows=rows)
    f, g = p.eval(x, terms=sr.TERM_DATA)
    ef = pl.note(abs(f - f_ref) / max(1.0, abs(f_ref)), "cost")
    eg = pl.relerr(g, g_ref)
    ea = max(pl.relerr(p.apply(x, k), model.apply(x, k)) for k in range(K))
    et = max(pl.relerr(p.apply_transpose(r, k), model.apply_transpose(r, k)) for k in range(K))
    print("%s: cost %.2e gradient %.2e apply %.2e apply_transpose %.2e (bar %.0e)" % (tag, ef, eg, ea, et, tol))
    assert max(ef, eg, ea, et) <= tol, (tag, ef, eg, ea, et)


# ------------------------------------------------------------------------------------------- parity with the restatement
PARITY = [(i,) + c for i, c in enumerate(itertools.product(MODES, MOTIONS, WEIGHTS))]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("case", PARITY, ids=lambda c: "%s_%s_%s" % c[1:])
def test_evaluation_matches_the_restatement(sr, ctx, case, dtype):
    i, mode, mkind, wkind = case
    (h, w), s, ksize, K, Cn = SHAPES[i % len(SHAPES)]
    H, W = h * s, w * s
    f32 = dtype == "f32"
    rng = np.random.default_rng(1000 + i)
    motion, shifts, mats, fields = make_motion(mkind, rng, K, W, H, f32)
    bank = make_bank(rng, mode, K, Cn, ksize)
    x, y, r = rng.random((Cn, H, W)), rng.random((K, Cn, h, w)), rng.random((Cn, h, w))
    tol = 2e-5 if f32 else 1e-12
    p = make_problem(sr, ctx, (h, w), s, Cn, K, dtype, shifts, mats, fields)  # created with another blur size
    p.set_blur_bank(bank, mode_id(sr, mode))
    got_mode, got = p.blur_bank()
    assert p.active_impl() == sr.IMPL_DIRECT and got_mode == mode_id(sr, mode) and np.array_equal(got, bank)
    p.set_observations(y)  # the bank persists across the observation, weight and loss calls
    model = bb.BlurBankModel(s, K, Cn, H, W, bank, bb.MODES[mode], motion)
    wts = make_weights(wkind, rng, y.shape)
    if wkind == "huber":
        wts = rr.huber_weights(rr.residuals(model, y, x), HUBER_DELTA)
        p.set_data_loss(sr.DATA_LOSS_HUBER, HUBER_DELTA)
        xd = upload(sr, ctx, p, x)
        p.update_data_weights_device(xd.value)
        ctx.synchronize()
        free(sr, ctx, xd)
    elif wts is not None:
        p.set_data_weights(wts)
    assert np.array_equal(p.blur_bank()[1], bank)
    check_parity(p, model, x, y, wts, r, K, tol, "%s %s" % (case, dtype), sr=sr)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", MODES)
def test_cost_rows_regulariser_and_photometric_parameters(sr, ctx, mode, dtype):
    (h, w), s, ksize, K, Cn = (17, 23), 2, 5, 5, 3
    H, W = h * s, w * s
    rng = np.random.default_rng(31)
    motion, shifts, _, _ = make_motion("shifts", rng, K, W, H)
    bank = make_bank(rng, mode, K, Cn, ksize)
    x, y, r = rng.random((Cn, H, W)), rng.random((K, Cn, h, w)), rng.random((Cn, h, w))
    regw = 0.5 + rng.random(x.shape)
    tol = 2e-5 if dtype == "f32" else 1e-12
    p = make_problem(sr, ctx, (h, w), s, Cn, K, dtype, shifts, None, None)
    p.set_blur_bank(bank, mode_id(sr, mode))
    p.set_observations(y)
    model = bb.BlurBankModel(s, K, Cn, H, W, bank, bb.MODES[mode], motion)
    rows = (2 * s, (h - 3) * s)
    p.set_cost_rows(*rows)
    check_parity(p, model, x, y, None, r, K, tol, "%s %s band" % (mode, dtype), rows=rows, sr=sr)
    p.set_cost_rows(0, H)
    # with a regulariser: the data term of the bank plus the checker's regulariser term
    p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
    p.set_irls_weights(0, regw)
    ref = orc.Problem(orc.ImageModel(scale=s, shifts=shifts, num_frames=K), y)
    ref.add_regularizer(orc.REG_BTV, 0.01, 2, 0.6)
    ref.set_irls_weights(0, regw)
    f_reg, g_reg = ref.reg_term(0, x)
    f_ref, g_ref = model.data_term(y, None, x)
    f, g = p.eval(x)
    assert pl.note(abs(f - f_ref - f_reg) / max(1.0, abs(f_ref + f_reg)), "cost ALL") <= tol
    assert pl.relerr(g, g_ref + g_reg.reshape(g_ref.shape)) <= tol
    # photometric parameters: the problem solves against the normalised frames; the bank persists across the call
    gb = np.stack([0.7 + 0.6 * rng.random(K), 0.1 * rng.standard_normal(K)], axis=1)
    p.clear_regularizers()
    p.set_photometric(gb)
    assert np.array_equal(p.blur_bank()[1], bank)
    yn = pr.normalise(y, gb, np.float32 if dtype == "f32" else np.float64)
    check_parity(p, model, x, yn, None, r, K, tol, "%s %s photometric" % (mode, dtype), sr=sr)


def test_split_channels_takes_a_per_channel_entry_by_the_problems_channel(sr, ctx):
    """A split_channels solve of a C = 3 problem with a per-channel bank solves channel c under entry c: each channel of
    its solution is, bit for bit, the solve of the one-channel problem of that channel under that kernel (the same
    kernels on the same values: the thresholds of a split solve are those of one channel's unknowns)."""
    (h, w), s, ksize, K, Cn = (17, 23), 2, 5, 2, 3
    H, W = h * s, w * s
    rng = np.random.default_rng(17)
    _, shifts, _, _ = make_motion("shifts", rng, K, W, H)
    bank = np.stack([bk.streak_psf(5), bk.anisotropic_psf(), bk.resize_kernel(bk.gaussian_taps(3, 1.0), 5)])
    gt = rng.random((Cn, H, W))
    model = bb.BlurBankModel(s, K, Cn, H, W, bank, bb.PER_CHANNEL, ("shifts", shifts))
    y = np.stack([model.apply(gt, k) for k in range(K)])
    x0 = np.stack([rr.bilinear(y[0, c:c + 1], s)[0] for c in range(Cn)])
    o = sr.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations, o.split_channels = 2, 10, 1
    p = make_problem(sr, ctx, (h, w), s, Cn, K, "f64", shifts, None, None)
    p.set_blur_bank(bank, sr.BLUR_PER_CHANNEL)
    p.set_observations(y)
    p.add_regularizer(sr.REG_BTV, 0.001, 2, 0.5)
    f0, _ = p.eval(x0)
    x, rep = p.solve(x0, o)
    p.clear_regularizers()
    p.add_regularizer(sr.REG_BTV, 0.001, 2, 0.5)
    f1, _ = p.eval(x)
    d1, _ = p.eval(x, terms=sr.TERM_DATA, want_grad=False)
    ref1, _ = model.data_term(y, None, x, want_grad=False)
    assert f1 < f0 and pl.note(abs(d1 - ref1) / max(1.0, abs(ref1)), "data cost after the solve") <= 1e-12
    o.split_channels = 0
    for c in range(Cn):
        q = make_problem(sr, ctx, (h, w), s, 1, K, "f64", shifts, None, None)
        q.set_blur_kernel(bank[c])
        q.set_observations(y[:, c:c + 1])
        q.add_regularizer(sr.REG_BTV, 0.001, 2, 0.5)
        xc, _ = q.solve(x0[c:c + 1], o)
        assert np.array_equal(xc[0], x[c]), (c, np.max(np.abs(xc[0] - x[c])))


# ------------------------------------------------------------------------------------------- bit identity
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mkind", MOTIONS)
@pytest.mark.parametrize("mode", MODES)
def test_equal_entries_are_the_single_kernel_bit_for_bit(sr, ctx, mode, mkind, dtype):
    (h, w), s, ksize, K, Cn = (17, 23), 2, 5, 5, 3
    H, W = h * s, w * s
    rng = np.random.default_rng(23)
    _, shifts, mats, fields = make_motion(mkind, rng, K, W, H, dtype == "f32")
    taps = rng.uniform(-0.5, 1.0, (ksize, ksize))
    lead = (K, Cn) if mode == "frame_channel" else ((K,) if mode == "frame" else (Cn,))
    bank = np.broadcast_to(taps, lead + taps.shape).copy()
    x, y = rng.random((Cn, H, W)), rng.random((K, Cn, h, w))
    x0 = rng.random((Cn, H, W))
    wts = 0.1 + rng.random(y.shape)
    o = sr.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = 2, 8
    out = {}
    for which in ("kernel", "bank"):
        p = make_problem(sr, ctx, (h, w), s, Cn, K, dtype, shifts, mats, fields)
        p.set_observations(y)
        p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
        if which == "kernel":
            p.set_blur_kernel(taps)
        else:
            p.set_blur_bank(bank, mode_id(sr, mode))
        plain = p.eval(x)
        p.set_data_weights(wts)
        weighted = p.eval(x)
        p.set_data_weights(None)
        xs, rep = p.solve(x0, o)
        out[which] = (plain, weighted, xs, (rep.irls_rounds, rep.cg_iterations, rep.evaluations, rep.final_cost))
    for a, b in zip(out["kernel"][:2], out["bank"][:2]):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert np.array_equal(out["kernel"][2], out["bank"][2]) and out["kernel"][3] == out["bank"][3]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_set_null_pairs_and_replacement_are_bit_identical(sr, ctx, dtype):
    s, h, w, K, Cn = 2, 40, 72, 3, 1
    rng = np.random.default_rng(4)
    shifts = [[0, 0], [1.25, -.75], [-.5, 1.5]]
    x, y = rng.random((Cn, h * s, w * s)), rng.random((K, Cn, h, w))
    p = make_problem(sr, ctx, (h, w), s, Cn, K, dtype, shifts, None, None)
    p.set_observations(y)
    p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
    assert p.active_impl() == sr.IMPL_TILED and p.blur_bank() == (0, None)
    auto = p.eval(x)
    gauss = p.blur_kernel()
    bank, taps = rng.random((K, 5, 5)), rng.random((7, 7))
    p.set_blur_bank(bank)  # K != C: the mode is inferred
    assert p.blur_bank()[0] == sr.BLUR_PER_FRAME and p.active_impl() == sr.IMPL_DIRECT
    with_bank = p.eval(x)
    p.set_blur_bank(None)  # restores the created blur, its size and the tile family
    assert p.active_impl() == sr.IMPL_TILED and p.blur_bank() == (0, None) and np.array_equal(p.blur_kernel(), gauss)
    again = p.eval(x)
    assert again[0] == auto[0] and np.array_equal(again[1], auto[1])
    # a bank replaced by a single kernel and back; NULL on the other call restores as well
    p.set_blur_kernel(taps)
    with_kernel = p.eval(x)
    p.set_blur_bank(bank, sr.BLUR_PER_FRAME)
    assert p.blur_bank()[0] == sr.BLUR_PER_FRAME
    again = p.eval(x)
    assert again[0] == with_bank[0] and np.array_equal(again[1], with_bank[1])
    p.set_blur_kernel(taps)
    assert p.blur_bank() == (0, None) and np.array_equal(p.blur_kernel(), taps)
    again = p.eval(x)
    assert again[0] == with_kernel[0] and np.array_equal(again[1], with_kernel[1])
    p.set_blur_bank(bank, sr.BLUR_PER_FRAME)
    p.set_blur_kernel(None)
    assert p.active_impl() == sr.IMPL_TILED and p.blur_bank() == (0, None)
    again = p.eval(x)
    assert again[0] == auto[0] and np.array_equal(again[1], auto[1])


# ------------------------------------------------------------------------------------------- status answers
def test_status_answers(sr, ctx):
    s, h, w, K, Cn = 2, 17, 23, 2, 2
    H, W = h * s, w * s
    rng = np.random.default_rng(8)
    x, y = rng.random((Cn, H, W)), rng.random((K, Cn, h, w))
    p = make_problem(sr, ctx, (h, w), s, Cn, K, "f64", [[0, 0], [1, 1]], None, None)
    p.set_observations(y)
    good = rng.random((K, 5, 5))
    lib = sr.load()
    with pytest.raises(ValueError):
        p.set_blur_bank(good)  # K == C: the mode is required
    p.set_blur_bank(good, sr.BLUR_PER_FRAME)
    before = p.eval(x)

    def unchanged():
        after = p.eval(x)
        m, b = p.blur_bank()
        return m == sr.BLUR_PER_FRAME and np.array_equal(b, good) and after[0] == before[0] and np.array_equal(after[1], before[1])

    nan, inf = good.copy(), good.copy()
    nan[1, 2, 3], inf[0, 0, 0] = np.nan, np.inf

    def raw(mode, ksize, a):
        return lib.srmap_problem_set_blur_bank(p.handle, mode, ksize, np.ascontiguousarray(a).ctypes.data_as(sr.c_double_p))

    for mode, ksize, a, status in ((1, 9, rng.random((K, 9, 9)), sr.EUNSUPPORTED), (1, 4, rng.random((K, 4, 4)), sr.EINVAL),
                                   (1, 0, good, sr.EINVAL), (1, -1, good, sr.EINVAL), (1, 5, nan, sr.EINVAL), (1, 5, inf, sr.EINVAL),
                                   (0, 5, good, sr.EINVAL), (4, 5, good, sr.EINVAL)):
        assert raw(mode, ksize, a) == status, (mode, ksize)
        assert unchanged()
    # the single-kernel calls while a bank is set
    k = C.c_int(0)
    assert lib.srmap_problem_get_blur_kernel(p.handle, C.byref(k), None) == sr.OK and k.value == 5
    out = np.zeros(25)
    assert lib.srmap_problem_get_blur_kernel(p.handle, C.byref(k), out.ctypes.data_as(sr.c_double_p)) == sr.EUNSUPPORTED
    assert "srmap_problem_get_blur_bank" in ctx_error(sr, ctx)
    with pytest.raises(sr.SrmapError) as e:
        p.fit_blur(x, ksize=5)
    assert e.value.status == sr.EUNSUPPORTED and "srmap_fit_blur_bank" in str(e.value)
    assert unchanged()
    # the bank fit's errors are srmap_fit_blur's, plus the mode
    for kw, status in ((dict(ksize=9), sr.EUNSUPPORTED), (dict(ksize=4), sr.EINVAL), (dict(ridge=-1.0), sr.EINVAL),
                       (dict(ridge=np.nan), sr.EINVAL), (dict(struct_size=8), sr.EINVAL)):
        with pytest.raises(sr.SrmapError) as e:
            p.fit_blur_bank(x, sr.BLUR_PER_FRAME, **kw)
        assert e.value.status == status, kw
        assert unchanged()
    o = sr.BlurFitOptions()
    lib.srmap_blur_fit_options_default(C.byref(o))
    xa = np.ascontiguousarray(x)
    assert lib.srmap_fit_blur_bank(p.handle, xa.ctypes.data_as(sr.c_double_p), 7, C.byref(o), None, None, None) == sr.EINVAL
    assert unchanged()
    empty = make_problem(sr, ctx, (h, w), s, Cn, K, "f64", None, None, None)
    with pytest.raises(sr.SrmapError) as e:
        empty.fit_blur_bank(x, sr.BLUR_PER_FRAME)
    assert e.value.status == sr.EINVAL and "no observations" in str(e.value)
    # the tile family does not cover a bank
    p.set_impl(sr.IMPL_TILED)
    with pytest.raises(sr.SrmapError) as e:
        p.eval(x)
    assert e.value.status == sr.EUNSUPPORTED
    p.set_impl(sr.IMPL_AUTO)
    assert p.active_impl() == sr.IMPL_DIRECT and unchanged()

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
    xd, gd = upload(sr, ctx, p, x), upload(sr, ctx, p, x)
    for mode in (sr.SHARD_FRAMES, sr.SHARD_ROWS, sr.SHARD_CHANNELS):
        sd = sr.ShardDesc()
        sd.mode = mode
        sd.own_row0, sd.own_row1, sd.own_ch0, sd.own_ch1 = 0, H, 0, 1
        with pytest.raises(sr.SrmapError) as e:
            p.solve(x, comm=comm, shard=sd)
        assert e.value.status == sr.EUNSUPPORTED and "bank" in str(e.value)
        with pytest.raises(sr.SrmapError) as e:
            p.eval_sharded_device(comm, sd, xd.value, gd.value)
        assert e.value.status == sr.EUNSUPPORTED
    assert fake.calls == []
    for ptr in (xd, gd):
        free(sr, ctx, ptr)
    assert unchanged()
    # a displacement field: the bank fit has no sampling leg for it, as srmap_fit_blur
    p.set_flow(fr.from_shifts([[0, 0], [1, 1]], H, W))
    with pytest.raises(sr.SrmapError) as e:
        p.fit_blur_bank(x, sr.BLUR_PER_FRAME)
    assert e.value.status == sr.EUNSUPPORTED


def ctx_error(sr, ctx):
    return sr.load().srmap_last_error(ctx._h).decode()


# ------------------------------------------------------------------------------------------- the fit
# LR shape, scale, ksize, motion, weights, K, C
FIT_CASES = [
    ((5, 7), 2, 7, "none", None, 2, 1),        # fewer observations than one tile
    ((9, 13), 3, 3, "affine", "mask", 5, 3),   # a whole frame of zero weight
    ((17, 23), 2, 5, "shifts", "random", 2, 3),
    ((17, 23), 3, 1, "shifts", None, 5, 1),
    ((37, 29), 2, 3, "affine", "random", 2, 3),  # 9 tiles per channel: five chunks, the last of one tile
    ((17, 23), 2, 7, "shifts", "random", 2, 3),  # 1275 sums: five blocks of the reduce, each over two chunks per channel
]


def fit_bars(G, sens, f32):
    """Bar per element of the Grams [entries][n + 1][n + 1]."""
    n = G.shape[1] - 1
    bar = np.zeros_like(G)
    blocks = ((slice(0, n), slice(0, n)), (slice(0, n), slice(n, n + 1)), (slice(n, n + 1), slice(n, n + 1)))
    for e in range(G.shape[0]):
        for q, sl in enumerate(blocks):
            big = np.max(np.abs(G[e][sl]))
            bar[e][sl] = 2e-5 * big if f32 else max(100 * sens[e][q], 1e-13 * big)
    return bar + bar.transpose(0, 2, 1) - bar * np.eye(n + 1)[None]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", FIT_CASES, ids=lambda c: "%dx%d_s%d_k%d_%s_%s_K%d_C%d" % (c[0] + c[1:]))
def test_fit_sums_taps_and_statuses(sr, ctx, case, mode, dtype):
    (h, w), s, ksize, mkind, wkind, K, Cn = case
    H, W = h * s, w * s
    f32 = dtype == "f32"
    rng = np.random.default_rng(7 * h + w + ksize)
    motion, shifts, mats, _ = make_motion(mkind, rng, K, W, H)
    x, y = rng.random((Cn, H, W)), rng.random((K, Cn, h, w))
    wts = make_weights(wkind, rng, y.shape)
    p = make_problem(sr, ctx, (h, w), s, Cn, K, dtype, shifts, mats, None)
    p.set_observations(y)
    if wts is not None:
        p.set_data_weights(wts)
    taps, q, ne = p.fit_blur_bank(x, mode_id(sr, mode), ksize=ksize, apply=False)
    assert p.blur_bank() == (0, None)
    xr, yr, wr = (f32r(x), f32r(y), f32r(wts)) if f32 else (x, y, wts)
    G, sens = bb.gram_sensitivity(xr, yr, wr, motion, ksize, s, bb.MODES[mode])
    n = ksize * ksize
    got = np.stack([bk.unpack(ne[e], n) for e in range(len(ne))])
    bar = fit_bars(G, sens, f32)
    worst = float(np.max(np.abs(got - G) / np.where(bar > 0, bar, 1.0)))
    pl.note(worst, "fit sums / bar")
    print("%s %s %s: largest deviation of the sums / bar %.3f" % (case, mode, dtype, worst))
    assert np.all(np.abs(got - G) <= bar)
    # taps and statuses per entry: the restatement's solve of the restatement's Gram, natural and permuted order
    cur = bk.gaussian_taps(3, 1.0)
    rt, rq, _ = bb.fit_bank(xr, yr, wr, motion, ksize, s, bb.MODES[mode], cur)
    pt, _, _ = bb.fit_bank(xr, yr, wr, motion, ksize, s, bb.MODES[mode], cur, order="permuted")
    assert np.array_equal(q[:, 4], rq[:, 4])
    if wkind == "mask" and mode != "channel":
        dead = [e for e in range(len(q)) if all(k == 1 for k, _ in bb.members(bb.MODES[mode], K, Cn, e))]
        assert dead and all(q[e, 4] == 3 for e in dead)
        for e in dead:  # a degenerate entry keeps the kernel in force, at the fit's size
            assert np.array_equal(taps.reshape(-1, ksize, ksize)[e], bk.resize_kernel(cur, ksize))
    if not f32:
        tap_bar = max(100 * float(np.max(np.abs(rt - pt))), 1e-10)
        err = float(np.max(np.abs(taps.reshape(rt.shape) - rt)))
        print("  taps: deviation %.2e (bar %.2e)" % (err, tap_bar))
        assert err <= tap_bar
    # bit-identical repeats, host and device form alike in what they sum
    t2, q2, ne2 = p.fit_blur_bank(x, mode_id(sr, mode), ksize=ksize, apply=False)
    assert np.array_equal(taps, t2) and np.array_equal(q, q2) and np.array_equal(ne, ne2)


def test_fit_options_apply_ridge_sum_to_one_and_a_permuted_stack(sr, ctx):
    (h, w), s, ksize, K, Cn = (17, 23), 2, 5, 5, 1
    H, W = h * s, w * s
    rng = np.random.default_rng(12)
    motion, shifts, _, _ = make_motion("shifts", rng, K, W, H)
    truth = np.stack([bk.streak_psf(5), bk.anisotropic_psf(), bb.streak(45), bb.pad(bk.gaussian_taps(3, 1.0), 5), bb.streak(90)])
    gt = rng.random((Cn, H, W))
    model = bb.BlurBankModel(s, K, Cn, H, W, truth, bb.PER_FRAME, motion)
    y = np.stack([model.apply(gt, k) for k in range(K)])
    p = make_problem(sr, ctx, (h, w), s, Cn, K, "f64", shifts, None, None)
    p.set_observations(y)
    # noise-free recovery of every entry, the single kernel's bar (tests/test_blur_kernel_cpu.py)
    taps, q, _ = p.fit_blur_bank(gt, sr.BLUR_PER_FRAME, ksize=5, apply=False)
    err = float(np.max(np.abs(taps - truth)))
    print("noise-free: largest tap error %.2e" % err)
    assert np.all(q[:, 4] == 0) and err <= cpu.RECOVERY_BAR and abs(taps.sum(axis=(1, 2)) - 1).max() <= 1e-14
    assert p.blur_bank() == (0, None)
    # apply installs the bank, and the next fit's ridge pulls towards the entries in force
    p.fit_blur_bank(gt, sr.BLUR_PER_FRAME, ksize=5)
    m, b = p.blur_bank()
    assert m == sr.BLUR_PER_FRAME and np.array_equal(b, taps)
    yn = y + 0.01 * rng.standard_normal(y.shape)
    p.set_observations(yn)
    for ridge, s1 in ((0.0, False), (1e-2, True), (1e-2, False)):
        got, gq, _ = p.fit_blur_bank(gt, sr.BLUR_PER_FRAME, ksize=5, ridge=ridge, sum_to_one=s1, apply=False)
        ref, rq, _ = bb.fit_bank(gt, yn, None, motion, 5, s, bb.PER_FRAME, (bb.PER_FRAME, taps), s1, ridge)
        other, _, _ = bb.fit_bank(gt, yn, None, motion, 5, s, bb.PER_FRAME, (bb.PER_FRAME, taps), s1, ridge, order="permuted")
        bar = max(100 * float(np.max(np.abs(ref - other))), 1e-10)
        assert float(np.max(np.abs(got - ref))) <= bar, (ridge, s1)
        assert np.array_equal(gq[:, 4], rq[:, 4])
        if s1:
            assert abs(got.sum(axis=(1, 2)) - 1).max() <= 1e-14
    # the device form returns what the host form returns
    import torch
    xt = torch.from_numpy(gt).to("cuda")
    dev = p.fit_blur_bank(xt, sr.BLUR_PER_FRAME, ksize=5, apply=False)
    host = p.fit_blur_bank(gt, sr.BLUR_PER_FRAME, ksize=5, apply=False)
    assert all(np.array_equal(a, b_) for a, b_ in zip(dev, host))
    # a permuted stack gives the permuted bank, bit for bit (each entry sums its own frame's records)
    perm = [3, 0, 4, 1, 2]
    p2 = make_problem(sr, ctx, (h, w), s, Cn, K, "f64", [shifts[k] for k in perm], None, None)
    p2.set_observations(yn[perm])
    p.set_blur_bank(None)
    a, qa, _ = p.fit_blur_bank(gt, sr.BLUR_PER_FRAME, ksize=5, apply=False)
    b2, qb, _ = p2.fit_blur_bank(gt, sr.BLUR_PER_FRAME, ksize=5, apply=False)
    assert np.array_equal(b2, a[perm]) and np.array_equal(qb, qa[perm])


# ------------------------------------------------------------------------------------------- the dependent fits
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("mode", MODES)
def test_refine_motion_and_fit_photometric_read_the_bank(sr, ctx, mode, dtype):
    (h, w), s, ksize, K, Cn = (17, 23), 2, 5, 5, 3
    H, W = h * s, w * s
    f32 = dtype == "f32"
    rng = np.random.default_rng(41)
    motion, _, mats, _ = make_motion("affine", rng, K, W, H)
    bank = make_bank(rng, mode, K, Cn, ksize)
    x, y = rng.random((Cn, H, W)), rng.random((K, Cn, h, w))
    wts = 0.1 + rng.random(y.shape)
    p = make_problem(sr, ctx, (h, w), s, Cn, K, dtype, None, mats, None)
    p.set_blur_bank(bank, mode_id(sr, mode))
    p.set_observations(y)
    p.set_data_weights(wts)
    xr, yr, wr = (f32r(x), f32r(y), f32r(wts)) if f32 else (x, y, wts)
    flat = bb.flat_bank(f32r(bank) if f32 else bank, bb.MODES[mode], K, Cn)
    # one pass of the refinement: per frame the channels' sums under their own entries, the refinement test's bars
    _, q, ne = p.refine_motion(x, max_iterations=0, apply=False)
    for k in range(K):
        S = {o: sum(mr.refine_sums(xr[c:c + 1], yr[k, c:c + 1], wr[k, c:c + 1], ar.inverse_map(mats[k]),
                                   flat[bb.entry_of(bb.MODES[mode], Cn, k, c)], s, o) for c in range(Cn)) for o in ("rows", "cols", "reversed")}
        ref, bar = S["rows"], np.zeros(mr.SUMS)
        for lo, hi in ((0, 21), (21, 27), (27, 28)):
            sens = max(np.max(np.abs(S[o][lo:hi] - ref[lo:hi])) for o in ("cols", "reversed"))
            bar[lo:hi] = max(100 * sens, 1e-13 * np.max(np.abs(ref[lo:hi])))
        dev = np.abs(ne[k] - ref)
        pl.note(np.max(dev / np.where(bar > 0, bar, 1.0)), "refine sums / bar")
        assert np.all(dev <= bar), (k, dev, bar)
    # the photometric fit's six sums per frame: 100 x the restatement's order sensitivity, floor 1e-13 of the magnitude
    # (f32: 2e-5 of the magnitude), as tests/test_gpu_photometric.py holds them
    _, _, ps = p.fit_photometric(x, apply=False)
    model = bb.BlurBankModel(s, K, Cn, H, W, flat, bb.MODES[mode], motion)
    ref, bar = tp.sums_bars(model, xr, yr, wr, f32)
    dev = np.abs(ps - ref)
    pl.note(np.max(dev / np.where(bar > 0, bar, 1.0)), "photometric sums / bar")
    assert np.all(dev <= bar), (dev, bar)


# ------------------------------------------------------------------------------------------- the table
@pytest.fixture(scope="module")
def table():
    return bb.table_inputs()


@pytest.mark.parametrize("told", ["guess", "true", "fitted"])
def test_table_solves_reproduce_the_pinned_figures(sr, ctx, table, told):
    """The three solves of DESIGN.md 3.14 on the GPU against the restatement's pinned figures: the counts equal, the PSNR
    within 0.01 dB."""
    T = table
    o = sr.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = bb.SOLVE_CAPS
    got = {}
    for scene in ("calibration", "second"):
        gt, _, y = T["scenes"][scene]
        p = sr.Problem(ctx, T["W"], T["H"], T["C"], T["K"], T["s"], T["shifts"], 0, 0.0, sr.F64)
        p.set_observations(y)
        p.add_regularizer(sr.REG_BTV, *T["reg"][1:])
        if told == "guess":
            p.set_blur_kernel(bk.gaussian_taps(*T["guess"]))
        elif told == "true":
            p.set_blur_bank(T["bank"], sr.BLUR_PER_FRAME)
        else:  # fitted from the calibration pair, applied to this scene
            cal = sr.Problem(ctx, T["W"], T["H"], T["C"], T["K"], T["s"], T["shifts"], 3, 1.0, sr.F64)
            cal.set_observations(T["scenes"]["calibration"][2])
            fitted, q, _ = cal.fit_blur_bank(T["scenes"]["calibration"][0], sr.BLUR_PER_FRAME, ksize=5)
            assert np.all(q[:, 4] == 0) and np.array_equal(cal.blur_bank()[1], fitted)
            p.set_blur_bank(fitted, sr.BLUR_PER_FRAME)
        x, rep = p.solve(rr.bilinear(y[0], T["s"]), o)
        got[scene] = (orc.psnr(gt, x), (rep.irls_rounds, rep.cg_iterations, rep.evaluations))
        want = cpu.TABLE[told][scene]
        print("%-7s %-11s PSNR %.3f dB (pinned %.3f), rounds / iterations / evaluations %s (pinned %s)"
              % (told, scene, got[scene][0], want[0], got[scene][1], want[1]))
    for scene in got:
        want = cpu.TABLE[told][scene]
        # the counts equal the pinned ones, the evaluations within the restatement's own spread where it has one
        assert abs(pl.note(got[scene][0] - want[0], "PSNR - pinned")) <= 0.01 and cpu.counts_match(told, scene, got[scene][1]), (scene, got[scene])
