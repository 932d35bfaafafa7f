"""Parity matrix of the direct regulariser kernels (csrc/kernels_reg_direct.hip): every values, IRLS-weights and gradient
variant of tests/reg_matrix.py in both dtypes against the f64 oracle with the term-scaled bars of tests/error_bars.py,
and the bit identities the kernels' comments claim between the variants.

Inputs are dyadic (x = k/64, weights = k/16, lambda = 2^-6, decay 0.5 or 1): f32 casts are exact, every difference
|x_p - x_q| is exact, so kernel and oracle differ by the rounding of the sums alone.
"""
import numpy as np
import pytest

import oracle as orc
import error_bars as eb
import reg_matrix as rm
from parity_log import note

pytestmark = pytest.mark.gpu

DTYPES = (eb.F64, eb.F32)
LAM = eb.LAMBDA


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


def _x(rng, C, H, W):
    return rng.integers(0, 65, size=(C, H, W)) / 64.0


def _problem(sr, ctx, C, H, W, dtype, regs, S=1, shifts=None, lr=None):
    """GPU and oracle problems with the regularisers regs [(kind, R, decay, weights or None)] at lambda = 2^-6."""
    K = 1 if shifts is None else len(shifts)
    shifts = [[0, 0]] if shifts is None else shifts
    if lr is None:
        lr = np.zeros((K, C, H // S, W // S))
    p = sr.Problem(ctx, W, H, C, K, S, shifts, 0, 0.0, dtype)
    p.set_observations(lr)
    ref = orc.Problem(orc.ImageModel(scale=S, shifts=shifts), lr)
    for kind, R, dc, w in regs:
        i = p.add_regularizer(kind, LAM, R, dc)
        j = ref.add_regularizer(kind, LAM, R, dc)
        if w is not None:
            p.set_irls_weights(i, w)
            ref.set_irls_weights(j, w)
    return p, ref


def _reg_eval(sr, p, x):
    p.set_impl(sr.IMPL_DIRECT)
    return p.eval(x, sr.TERM_REG)


def _assert_grad_cost(f, g, f_ref, g_ref, Mf, M, dtype, extra=0.0):
    rg = eb.check_gradient(g, g_ref.reshape(g.shape), M, dtype, "reg grad")
    rf = eb.check_cost(f, f_ref, Mf, dtype, "reg cost")
    assert rg <= eb.C_REG_GRAD[dtype] + extra, rg
    assert rf <= eb.C_REG_COST[dtype] + extra, rf


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", rm.VALUE_CELLS, ids=[rm.cell_id(c) for c in rm.VALUE_CELLS])
def test_values(sr, ctx, cell, dtype):
    """srmap_reg_values on every values-kernel cell against the oracle's ApplyToImage."""
    kind, R, dc, C, H, W = cell
    x = _x(np.random.default_rng(C * 1000 + H * 7 + W), C, H, W)
    p, _ = _problem(sr, ctx, C, H, W, dtype, [(kind, R, dc, None)])
    v = p.reg_values(0, x)
    v_ref = orc.reg_values(kind, x, R, dc)
    rv = note(eb.bar_ratio(v, v_ref, eb.value_magnitude(kind, x, R, dc)) / eb.U[dtype],
              "values err/(u*M) %s" % ("f64" if dtype == eb.F64 else "f32"))
    assert rv <= eb.C_REG_VAL[dtype], rv


def _btv_values(sr, ctx, x, R, dc, dtype):
    C, H, W = x.shape
    p, _ = _problem(sr, ctx, C, H, W, dtype, [(rm.BTV, R, dc, None)])
    return p.reg_values(0, np.ascontiguousarray(x))


BIT_W4 = [c for c in rm.STRIP + rm.VALUES4 if c[5] - 1 - c[1] > 0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", rm.STRIP, ids=[rm.cell_id(c) for c in rm.STRIP])
def test_strip_bitwise_equals_values4(sr, ctx, cell, dtype):
    """A BTV value at row r reads rows r .. r + R only: on rows r + R < 15, strip(X) == values4(X[:, :15]) bitwise."""
    kind, R, dc, C, H, W = cell
    x = _x(np.random.default_rng(H * 31 + W), C, H, W)
    assert rm.values_kernel(kind, R, C, H, W) == "strip" and rm.values_kernel(kind, R, C, 15, W) == "values4_R3"
    a = _btv_values(sr, ctx, x, R, dc, dtype)
    b = _btv_values(sr, ctx, x[:, :15], R, dc, dtype)
    n = 15 - R
    assert np.array_equal(a[:, :n], b[:, :n])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", BIT_W4, ids=[rm.cell_id(c) for c in BIT_W4])
def test_values4_bitwise_equals_reg_values(sr, ctx, cell, dtype):
    """A BTV value at column c reads columns c .. c + R only: on columns c + R < W - 1, the four-column kernels of X
    (strip, values4) equal k_reg_values of X[..., :W-1] (W - 1 not a multiple of 4) bitwise."""
    kind, R, dc, C, H, W = cell
    x = _x(np.random.default_rng(H * 37 + W), C, H, W)
    assert rm.values_kernel(kind, R, C, H, W - 1) == "reg_values"
    a = _btv_values(sr, ctx, x, R, dc, dtype)
    b = _btv_values(sr, ctx, x[..., :W - 1], R, dc, dtype)
    n = W - 1 - R
    assert np.array_equal(a[..., :n], b[..., :n])


# ---------------------------------------------------------------- IRLS weights
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", rm.VALUE_CELLS, ids=[rm.cell_id(c) for c in rm.VALUE_CELLS])
def test_irls_weights_at_another_x(sr, ctx, cell, dtype):
    """srmap_update_irls_weights_device(x) on every values-kernel cell (the same launcher with as_weights = 1), then the
    TERM_REG cost and gradient at a DIFFERENT x' under IMPL_DIRECT, against the oracle with w = 1 / max(1e-5, r(x))."""
    import torch
    kind, R, dc, C, H, W = cell
    rng = np.random.default_rng(C * 977 + H * 13 + W)
    xw = rm.weights_input(rng, C, H, W)
    x2 = _x(rng, C, H, W)
    w_ref = 1.0 / np.maximum(1e-5, orc.reg_values(kind, xw, R, dc))
    p, ref = _problem(sr, ctx, C, H, W, dtype, [(kind, R, dc, None)])
    ref.set_irls_weights(0, w_ref)
    xt = torch.tensor(xw, dtype=torch.float64 if dtype == eb.F64 else torch.float32, device="cuda")
    torch.cuda.synchronize()
    p.update_irls_weights_device(0, xt.data_ptr())
    f, g = _reg_eval(sr, p, x2)
    f_ref, g_ref = ref.reg_term(0, x2)
    assert np.all(np.isfinite(g)) and np.isfinite(f)
    Mf, M = eb.reg_magnitude(kind, x2, w_ref, LAM, R, dc)
    _assert_grad_cost(f, g, f_ref, g_ref, Mf, M, dtype, extra=eb.weights_rel(kind, R))
    del xt


# ---------------------------------------------------------------- gradients and cost
def _grad_case(cell, seed):
    kind, R, dc, C, H, W = cell
    rng = np.random.default_rng(seed)
    return _x(rng, C, H, W), eb.dyadic_weights(rng, C, H, W)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", rm.GRAD_CELLS, ids=[rm.cell_id(c) for c in rm.GRAD_CELLS])
def test_reg_gradient_and_cost(sr, ctx, cell, dtype):
    """eval(x, TERM_REG) under IMPL_DIRECT on every gradient-kernel cell, dyadic IRLS weights."""
    kind, R, dc, C, H, W = cell
    x, w = _grad_case(cell, C * 101 + H * 3 + W)
    p, ref = _problem(sr, ctx, C, H, W, dtype, [(kind, R, dc, w)])
    f, g = _reg_eval(sr, p, x)
    f_ref, g_ref = ref.reg_term(0, x)
    Mf, M = eb.reg_magnitude(kind, x, w, LAM, R, dc)
    _assert_grad_cost(f, g, f_ref, g_ref, Mf, M, dtype)


TV_VALUES_GRAD = [c for c in rm.ONEPASS + rm.MARCH if c[4] < 1000]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", TV_VALUES_GRAD, ids=[rm.cell_id(c) for c in TV_VALUES_GRAD])
def test_tv_values_and_gradient_with_values(sr, ctx, cell, dtype):
    """srmap_reg_values_and_gradient: TV kinds WITH values go to k_reg_gradient_direct (eval never takes that path)."""
    kind, R, dc, C, H, W = cell
    x, gc = _grad_case(cell, C * 103 + H * 5 + W)
    assert rm.grad_kernel(kind, C, H, W, True) == "reg_gradient_direct"
    p, _ = _problem(sr, ctx, C, H, W, dtype, [(kind, R, dc, None)])
    v, g = p.reg_values_and_gradient(0, x, gc)
    v_ref, g_ref = orc.reg_values_and_gradient(kind, x, gc, R, dc)
    assert eb.bar_ratio(v, v_ref, eb.value_magnitude(kind, x)) / eb.U[dtype] <= eb.C_REG_VAL[dtype]
    _, M = eb.reg_magnitude(kind, x, gc, 1.0)  # the gradient constants gc stand for lambda * w
    rg = eb.check_gradient(g, g_ref, M, dtype, "reg grad")
    assert rg <= eb.C_REG_GRAD[dtype], rg


BIT_MARCH = [c for c in rm.MARCH if c[5] >= 4 and c[4] < 1000]
BIT_FAST = [c for c in rm.ONEPASS if "fast" in rm.onepass_paths(c[4], c[5])]


def _grad_only(sr, ctx, kind, x, w, dtype):
    C, H, W = x.shape
    p, _ = _problem(sr, ctx, C, H, W, dtype, [(kind, 0, 0.0, np.ascontiguousarray(w))])
    return _reg_eval(sr, p, np.ascontiguousarray(x))[1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", BIT_MARCH + BIT_FAST, ids=[rm.cell_id(c) for c in BIT_MARCH + BIT_FAST])
def test_tv_gradient_bitwise_across_kernels(sr, ctx, cell, dtype):
    """A TV gradient at column c reads columns up to c + 1: on columns c < W - 2 the march (TV3D, C >= 2) or the
    onepass fast path (W % 4 == 0) on X equals the onepass masked path on X[..., :W-1] bitwise."""
    kind, R, dc, C, H, W = cell
    x, w = _grad_case(cell, C * 107 + H * 11 + W)
    k1 = rm.grad_kernel(kind, C, H, W, False)
    assert k1 == "march" or "fast" in rm.onepass_paths(H, W)
    assert rm.grad_kernel(kind, C, H, W - 1, False).startswith("onepass") and rm.onepass_paths(H, W - 1) == {"masked"}
    a = _grad_only(sr, ctx, kind, x, w, dtype)
    b = _grad_only(sr, ctx, kind, x[..., :W - 1], w[..., :W - 1], dtype)
    assert np.array_equal(a[..., :W - 2], b[..., :W - 2])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,R,C,H,W", [(rm.TV3D, 0, 3, 12, 260), (rm.TV, 0, 2, 10, 258), (rm.BTV, 3, 1, 18, 20)],
                         ids=["march", "onepass-masked", "btv3-strip"])
def test_with_data_term_accumulates(sr, ctx, kind, R, C, H, W, dtype):
    """TERM_ALL under IMPL_DIRECT: the regulariser kernel adds onto the data gradient (accumulate reads the old g)."""
    S = 2
    shifts = [[0, 0], [1, -1], [-2, 1]]
    rng = np.random.default_rng(H * W + kind)
    x, lr = eb.dyadic_inputs(rng, len(shifts), C, H, W, S)
    w = eb.dyadic_weights(rng, C, H, W)
    p, ref = _problem(sr, ctx, C, H, W, dtype, [(kind, R, 0.5, w)], S=S, shifts=shifts, lr=lr)
    p.set_impl(sr.IMPL_DIRECT)
    f, g = p.eval(x, sr.TERM_ALL)
    f_ref, g_ref = ref.objective(x)
    Mf, M = eb.term_magnitude(orc.ImageModel(scale=S, shifts=shifts), lr, x, [(kind, LAM, R, 0.5, w)])
    _assert_grad_cost(f, g, f_ref, g_ref, Mf, M, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("first", [(0, 0), (2, 3)], ids=["tv", "btv3"])
def test_auto_tile_with_march_second_regulariser(sr, ctx, first, dtype):
    """IMPL_AUTO at a tile-eligible size: the tile kernel fuses the first regulariser, the march adds 3-D TV onto its
    gradient ("remaining regularisers" of the tile evaluation, eval.hip launch_regs_direct)."""
    S, W, H, C = 2, 128, 24, 3
    shifts = [[0, 0], [0, 0]]
    rng = np.random.default_rng(5 + first[0])
    x, lr = eb.dyadic_inputs(rng, len(shifts), C, H, W, S)
    w1, w2 = eb.dyadic_weights(rng, C, H, W), eb.dyadic_weights(rng, C, H, W)
    regs = [(first[0], first[1], 0.5, w1), (rm.TV3D, 0, 0.0, w2)]
    assert rm.grad_kernel(rm.TV3D, C, H, W, False) == "march"
    p, ref = _problem(sr, ctx, C, H, W, dtype, regs, S=S, shifts=shifts, lr=lr)
    p.set_impl(sr.IMPL_AUTO)
    f, g = p.eval(x, sr.TERM_ALL)
    assert p.active_impl() == sr.IMPL_TILED
    f_ref, g_ref = ref.objective(x)
    Mf, M = eb.term_magnitude(orc.ImageModel(scale=S, shifts=shifts), lr, x,
                              [(k, LAM, R, dc, w) for k, R, dc, w in regs])
    _assert_grad_cost(f, g, f_ref, g_ref, Mf, M, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", [(rm.TV3D, 0, 0.0, 3, 13, 260), (rm.TV, 0, 0.0, 2, 13, 255),
                                  (rm.TV, 0, 0.0, 1, 14, 256), (rm.BTV, 2, 0.5, 2, 13, 9)],
                         ids=["march", "onepass-masked", "onepass-fast", "btv2"])
def test_cost_rows_band_inside_row_blocks(sr, ctx, cell, dtype):
    """set_cost_rows(2, 10): both band ends fall inside a 4-row block of the onepass / march grid."""
    kind, R, dc, C, H, W = cell
    x, w = _grad_case(cell, 13 * H + W)
    p, ref = _problem(sr, ctx, C, H, W, dtype, [(kind, R, dc, w)])
    r0, r1 = 2, 10
    p.set_cost_rows(r0, r1)
    f, g = _reg_eval(sr, p, x)
    f_full, g_ref = ref.reg_term(0, x)
    v = orc.reg_values(kind, x, R, dc)
    f_ref = LAM * float(np.sum(w[:, r0:r1] * v[:, r0:r1] ** 2))
    assert f_ref < f_full
    rt = eb.value_magnitude(kind, x, R, dc)
    Mf = LAM * float(np.sum(w[:, r0:r1] * rt[:, r0:r1] ** 2))
    _, M = eb.reg_magnitude(kind, x, w, LAM, R, dc)
    _assert_grad_cost(f, g, f_ref, g_ref, Mf, M, dtype)
