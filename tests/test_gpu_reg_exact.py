"""The regularisers' exact gradient mode on the GPU (srmap_problem_set_regularizer_gradient; csrc/kernels_reg_direct.hip:
the Exact legs of k_reg_gradient_direct, tv_pixel / k_tv_onepass / k_tv3d_march, and k_btv_gradient_exact4) against the numpy
restatement of tests/reg_exact_restatement.py.

Bars: those of the regulariser parity tests (tests/error_bars.py: C_REG_VAL / C_REG_GRAD / C_REG_COST times the unit roundoff
times the sum of the absolute values of the terms an element sums -- reg_exact_restatement.magnitude states that sum for
the exact formulas).  Inputs are dyadic (x = k/64, weights = k/16, lambda = 2^-6, decay 0.5 or 1): the f32 cast is exact,
every sign is the same in both precisions, and in f64 every product and sum is exact.

k_btv_gradient_exact4 serves BTV R 1 .. 3 at W % 4 == 0; the Exact leg of k_reg_gradient_direct everything else."""
import json
import os

import numpy as np
import pytest

import oracle as orc
import error_bars as eb
import reg_exact_restatement as rx
import reg_matrix as rm
from conftest import GOLDEN

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


def _problem(sr, ctx, C, H, W, dtype, kind, R=0, decay=0.0, w=None, mode=None, lam=LAM):
    """a regulariser-only problem (scale 1, one frame of zeros, no blur)"""
    p = sr.Problem(ctx, W, H, C, 1, 1, [[0, 0]], 0, 0.0, dtype)
    p.set_observations(np.zeros((1, C, H, W)))
    i = p.add_regularizer(kind, lam, R, decay)
    if w is not None:
        p.set_irls_weights(i, w)
    if mode is not None:
        p.set_regularizer_gradient(i, mode)
    return p


def _reg_eval(sr, p, x):
    p.set_impl(sr.IMPL_DIRECT)
    return p.eval(x, sr.TERM_REG)


def _check(tag, f, g, f_ref, g_ref, Mf, M, dtype):
    rg = eb.bar_ratio(g, g_ref, M) / eb.U[dtype]
    print("%s: grad err/(u*M) %.3g (bar %g)" % (tag, rg, eb.C_REG_GRAD[dtype]), end="")
    assert rg <= eb.C_REG_GRAD[dtype], (tag, rg)
    if f is not None:
        rf = eb.bar_ratio([f], [f_ref], [Mf]) / eb.U[dtype]
        print(", cost err/(u*M) %.3g (bar %g)" % (rf, eb.C_REG_COST[dtype]), end="")
        assert rf <= eb.C_REG_COST[dtype], (tag, rf)
    print()


def _parity(sr, ctx, kind, R, decay, C, H, W, dtype, weighted, seed):
    """operator (accumulate off) and evaluation (accumulate on), a cost-row band, and the x[0,0] image"""
    rng = np.random.default_rng(seed)
    tag = "%s C%d %dx%d %s %s" % (rm.cell_id((kind, R, decay, C, H, W)), C, H, W, "f32" if dtype else "f64", "w" if weighted else "1")
    for x in (_x(rng, C, H, W), rx.corner_image((C, H, W), 0.5, 0.875)):
        w = eb.dyadic_weights(rng, C, H, W) if weighted else None
        wn = np.ones((C, H, W)) if w is None else w
        p = _problem(sr, ctx, C, H, W, dtype, kind, R, decay, w, sr.REG_GRADIENT_EXACT)
        # srmap_reg_values_and_gradient: the gradient constants stand for lambda * w
        gc = eb.dyadic_weights(rng, C, H, W)
        v, g = p.reg_values_and_gradient(0, x, gc)
        v_ref, g_ref = rx.gradient(kind, x, gc, rx.EXACT, R, decay)
        rv = eb.bar_ratio(v, v_ref, eb.value_magnitude(kind, x, R, decay)) / eb.U[dtype]
        assert rv <= eb.C_REG_VAL[dtype], (tag, rv)
        _check(tag + " operator", None, g, None, g_ref, None, rx.magnitude(kind, x, gc, rx.EXACT, R, decay)[1], dtype)
        # srmap_eval, regulariser terms
        f, g = _reg_eval(sr, p, x)
        _, g_ref = rx.gradient(kind, x, LAM * wn, rx.EXACT, R, decay)
        Mf, M = rx.magnitude(kind, x, LAM * wn, rx.EXACT, R, decay)
        _check(tag + " eval", f, g, rx.cost(kind, x, LAM * wn, R, decay), g_ref, Mf, M, dtype)
        f2, g2 = _reg_eval(sr, p, x)
        assert f2 == f and np.array_equal(g, g2), tag  # repeats: the same bits
        if H >= 3:  # a band of cost rows: the gradient stays whole
            p.set_cost_rows(1, H - 1)
            f, g = _reg_eval(sr, p, x)
            band = np.zeros((C, H, W)); band[:, 1:H - 1] = 1.0
            _check(tag + " band", f, g, rx.cost(kind, x, LAM * wn * band, R, decay), g_ref,
                   rx.magnitude(kind, x, LAM * wn * band, rx.EXACT, R, decay)[0], M, dtype)
    # the last x is the corner image: pixel (0, 0) is a source for its window, which the reference's gradient denies it
    if kind == rm.BTV:
        q = _problem(sr, ctx, C, H, W, dtype, kind, R, decay, w)
        g_refmode = _reg_eval(sr, q, x)[1]
        nb = [(i, j) for i in range(min(R + 1, H)) for j in range(min(R + 1, W)) if (i, j) != (0, 0)]
        for i, j in nb:
            assert g2[0, i, j] < 0.0 and g_refmode[0, i, j] == 0.0, (tag, i, j)


# H x W of the issue's list; 5 x 1028: 257 cells a row, one past a workgroup's 256
BTV_SHAPES = [(1, 1), (1, 5), (5, 1), (3, 4), (8, 8), (17, 23), (16, 64), (19, 252), (5, 1028)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", BTV_SHAPES, ids=lambda s: "%dx%d" % s)
def test_btv_exact_parity(sr, ctx, shape, R, dtype):
    """BTV on the fast kernel (R <= 3, W % 4 == 0) and on the generic leg (R = 4, ragged widths), C 1 and 3, without and
    with weights"""
    H, W = shape
    decay = 0.5 if R % 2 else 1.0
    for C, weighted in ((1, False), (3, True), (1, True)):
        _parity(sr, ctx, rm.BTV, R, decay, C, H, W, dtype, weighted, 1000 * R + 10 * H + W + C)


TV3D_CELLS = [(1, 5, 8), (2, 5, 8), (3, 6, 12), (2, 5, 7), (3, 4, 9), (17, 5, 8), (17, 5, 6)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("cell", TV3D_CELLS, ids=lambda c: "C%dH%dW%d" % c)
def test_tv3d_exact_parity(sr, ctx, cell, dtype):
    """3-D TV: the one-pass kernel (W % 4 != 0, or one channel), the channel march (W % 4 == 0; 17 channels: the chunk
    boundary), and k_reg_gradient_direct's leg through the operator"""
    C, H, W = cell
    if C == 17:
        assert len(rm.march_chunks(C, H, W)) > 1
    assert rm.grad_kernel(rm.TV3D, C, H, W, False) == ("march" if (C >= 2 and W % 4 == 0) else "onepass3d")
    for weighted in (False, True):
        _parity(sr, ctx, rm.TV3D, 0, 0.0, C, H, W, dtype, weighted, 77 * C + H + W)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_setters_and_refusals(sr, ctx, dtype):
    lib = sr.load()
    p = _problem(sr, ctx, 1, 8, 8, dtype, rm.BTV, 2, 0.5)

    def refused(call, status, *words):
        with pytest.raises(sr.SrmapError) as e:
            call()
        assert e.value.status == status, str(e.value)
        for word in words:
            assert word in str(e.value), (word, str(e.value))

    assert p.regularizer_gradient(0) == sr.REG_GRADIENT_REFERENCE  # the default
    for bad in (-1, 2, 7):
        refused(lambda: p.set_regularizer_gradient(0, bad), sr.EINVAL, "unknown regularizer gradient mode %d" % bad)
        assert p.regularizer_gradient(0) == sr.REG_GRADIENT_REFERENCE
    for reg in (-1, 1):
        refused(lambda: p.set_regularizer_gradient(reg, sr.REG_GRADIENT_EXACT), sr.EINVAL, "no regularizer %d" % reg)
        refused(lambda: p.regularizer_gradient(reg), sr.EINVAL, "no regularizer %d" % reg)
    assert lib.srmap_problem_set_regularizer_gradient(None, 0, 1) == sr.EINVAL
    assert lib.srmap_problem_get_regularizer_gradient(None, 0, None) == sr.EINVAL
    assert lib.srmap_problem_get_regularizer_gradient(p.handle, 0, None) == sr.EINVAL
    p.set_regularizer_gradient(0, sr.REG_GRADIENT_EXACT)
    assert p.regularizer_gradient(0) == sr.REG_GRADIENT_EXACT
    # the mode persists across the other setters
    p.set_regularizer_lambda(0, 0.02)
    p.set_irls_weights(0, np.ones((1, 8, 8)))
    p.set_observations(np.zeros((1, 1, 8, 8)))
    p.set_cost_rows(0, 8)
    p.set_impl(sr.IMPL_DIRECT)
    p.set_solver(sr.SOLVER_LBFGS, 5)
    assert p.regularizer_gradient(0) == sr.REG_GRADIENT_EXACT

    # sharded over more than one rank: refused, naming the setter, before any collective
    class NoExchange:
        calls = []

        class ReduceOp:
            SUM, MAX = 0, 1

        def all_reduce(self, *a, **k):
            self.calls.append("all_reduce")

        def isend(self, *a, **k):
            self.calls.append("isend")

        def irecv(self, *a, **k):
            self.calls.append("irecv")

    import torch
    fake = NoExchange()
    comm = sr.Comm(ctx, 0, 2, backend="host", dist=fake)
    x = np.full((1, 8, 8), 0.5)
    xd = torch.tensor(x, dtype=torch.float32 if dtype else torch.float64, device="cuda")
    gd = torch.zeros_like(xd)
    torch.cuda.synchronize()
    for kind in (rm.BTV, rm.TV3D):
        q = _problem(sr, ctx, 1, 8, 8, dtype, kind, 2, 0.5, mode=sr.REG_GRADIENT_EXACT)
        for mode in (sr.SHARD_FRAMES, sr.SHARD_ROWS, sr.SHARD_CHANNELS):
            sd = sr.ShardDesc()
            sd.mode = mode
            sd.own_row0, sd.own_row1, sd.own_ch0, sd.own_ch1 = 0, 8, 0, 1
            refused(lambda: q.solve(x, comm=comm, shard=sd), sr.EUNSUPPORTED, "srmap_problem_set_regularizer_gradient",
                    "not sharded", "run the solve unsharded")
            refused(lambda: q.eval_sharded_device(comm, sd, xd.data_ptr(), gd.data_ptr()), sr.EUNSUPPORTED,
                    "srmap_problem_set_regularizer_gradient", "not sharded", "evaluate unsharded")
    assert fake.calls == []


# ---------------------------------------------------------------- invariants
def _data_problem(sr, ctx, dtype, kind, R, C=1, H=24, W=128, S=2, seed=3, lam=LAM):
    """a tile-eligible geometry (tests/test_gpu_reg_kernels.py's): scale 2, integer shifts, no blur"""
    shifts = [[0, 0], [1, 0], [0, 1]]
    rng = np.random.default_rng(seed)
    x, lr = eb.dyadic_inputs(rng, len(shifts), C, H, W, S)
    w = eb.dyadic_weights(rng, C, H, W)
    p = sr.Problem(ctx, W, H, C, len(shifts), S, shifts, 0, 0.0, dtype)
    p.set_observations(lr)
    p.add_regularizer(kind, lam, R, 0.5)
    p.set_irls_weights(0, w)
    return p, x, lr, w, orc.ImageModel(scale=S, shifts=shifts)


def _few_iterations(sr):
    o = sr.default_irls_options()
    o.max_num_solver_iterations = 6
    o.max_num_irls_iterations = 2
    return o


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("impl", ["tiled", "direct"])
def test_exact_then_reference_is_an_untouched_twin(sr, ctx, impl, dtype):
    import gc
    lib = sr.load()
    # problems that earlier tests left to the collector are destroyed whenever it runs: have it run now, so that the count
    # below moves with this test's two problems alone (they are destroyed by hand at the end, as tests/model_walk.py does)
    gc.collect()
    start = int(lib.srmap_live_allocations())
    p, x, _, _, _ = _data_problem(sr, ctx, dtype, rm.BTV, 3)
    twin = _data_problem(sr, ctx, dtype, rm.BTV, 3)[0]
    for q in (p, twin):
        q.set_impl(sr.IMPL_DIRECT if impl == "direct" else sr.IMPL_AUTO)
    p.set_regularizer_gradient(0, sr.REG_GRADIENT_EXACT)
    f_ex, g_ex = p.eval(x)
    p.set_regularizer_gradient(0, sr.REG_GRADIENT_REFERENCE)
    f, g = p.eval(x)
    ft, gt = twin.eval(x)
    assert p.active_impl() == twin.active_impl() == (sr.IMPL_DIRECT if impl == "direct" else sr.IMPL_TILED)
    assert f == ft and np.array_equal(g, gt)
    assert not np.array_equal(g_ex, g)  # the mode did something in between
    xs, rep = p.solve(x, _few_iterations(sr))
    xt, rept = twin.solve(x, _few_iterations(sr))
    assert np.array_equal(xs, xt) and (rep.irls_rounds, rep.cg_iterations, rep.evaluations) == (rept.irls_rounds, rept.cg_iterations, rept.evaluations)
    for q in (p, twin):
        lib.srmap_problem_destroy(q._h)
        q._h = None
    end = int(lib.srmap_live_allocations())
    assert end == start, "%d live allocations at the start, %d after both problems are destroyed" % (start, end)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_tv_exact_is_reference_bit_for_bit_on_the_tiles(sr, ctx, dtype):
    p, x, _, _, _ = _data_problem(sr, ctx, dtype, rm.TV, 0)
    twin = _data_problem(sr, ctx, dtype, rm.TV, 0)[0]
    p.set_regularizer_gradient(0, sr.REG_GRADIENT_EXACT)
    f, g = p.eval(x)
    ft, gt = twin.eval(x)
    assert p.active_impl() == twin.active_impl() == sr.IMPL_TILED
    assert f == ft and np.array_equal(g, gt)
    xs, _ = p.solve(x, _few_iterations(sr))
    xt, _ = twin.solve(x, _few_iterations(sr))
    assert np.array_equal(xs, xt)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind,R,W", [(rm.BTV, 3, 64), (rm.BTV, 2, 23), (rm.BTV, 4, 8), (rm.TV3D, 0, 8)],
                         ids=["btv3", "btv2-ragged", "btv4", "tv3d"])
def test_values_and_irls_weights_are_the_same_in_both_modes(sr, ctx, kind, R, W, dtype):
    """srmap_reg_values: the same bits.  The IRLS weights (written on the device from another image): the regulariser cost at
    x under them, which the two modes reduce in the same order wherever one kernel template serves both -- the same bits;
    on k_btv_gradient_exact4 (btv3) another order of the same sum: the cost's bar."""
    import torch
    C, H = 2, 16
    rng = np.random.default_rng(W + R)
    x, xw = _x(rng, C, H, W), rm.weights_input(rng, C, H, W)
    xt = torch.tensor(xw, dtype=torch.float32 if dtype else torch.float64, device="cuda")
    torch.cuda.synchronize()
    out = []
    for mode in (sr.REG_GRADIENT_REFERENCE, sr.REG_GRADIENT_EXACT):
        p = _problem(sr, ctx, C, H, W, dtype, kind, R, 0.5, mode=mode)
        v = p.reg_values(0, x)
        p.update_irls_weights_device(0, xt.data_ptr())
        p.set_impl(sr.IMPL_DIRECT)
        out.append((v, p.eval(x, sr.TERM_REG, want_grad=False)[0]))
    assert np.array_equal(out[0][0], out[1][0])
    if kind == rm.BTV and R <= 3 and W % 4 == 0:
        w_ref = 1.0 / np.maximum(1e-5, rx.values(kind, xw, R, 0.5))
        Mf = rx.magnitude(kind, x, LAM * w_ref, rx.EXACT, R, 0.5)[0]
        assert abs(out[0][1] - out[1][1]) <= 2 * eb.C_REG_COST[dtype] * eb.U[dtype] * Mf
    else:
        assert out[0][1] == out[1][1]
    del xt


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("R", [2, 3])
def test_tiles_for_the_data_term_direct_kernels_for_exact_btv(sr, ctx, R, dtype):
    """Exact BTV on a tile-eligible geometry: the tiles keep the data term, the regulariser goes through the direct kernels
    (accumulating onto the tiles' gradient); the evaluation is the all-direct one within the bar, and both are the oracle's
    data term plus the restatement's exact regulariser."""
    p, x, lr, w, model = _data_problem(sr, ctx, dtype, rm.BTV, R)
    ref_p = _data_problem(sr, ctx, dtype, rm.BTV, R)[0]
    assert ref_p.eval(x)[0] > 0 and ref_p.active_impl() == sr.IMPL_TILED
    p.set_regularizer_gradient(0, sr.REG_GRADIENT_EXACT)
    f_t, g_t = p.eval(x)
    assert p.active_impl() == sr.IMPL_TILED  # what ran: the tile family (data term) ...
    p.set_impl(sr.IMPL_DIRECT)
    f_d, g_d = p.eval(x)
    assert p.active_impl() == sr.IMPL_DIRECT
    fd, gd = orc.Problem(model, lr).data_term(x)
    _, gr = rx.gradient(rm.BTV, x, LAM * w, rx.EXACT, R, 0.5)
    f_ref, g_ref = fd + rx.cost(rm.BTV, x, LAM * w, R, 0.5), gd.reshape(x.shape) + gr
    Mf, M = eb.term_magnitude(model, lr, x)
    Mfr, Mr = rx.magnitude(rm.BTV, x, LAM * w, rx.EXACT, R, 0.5)
    Mf, M = Mf + Mfr, M + Mr
    for tag, f, g in (("tiles + direct", f_t, g_t), ("all direct", f_d, g_d)):
        rg = eb.bar_ratio(g, g_ref, M) / eb.U[dtype]
        rf = eb.bar_ratio([f], [f_ref], [Mf]) / eb.U[dtype]
        print("%s: grad err/(u*M) %.3g, cost err/(u*M) %.3g" % (tag, rg, rf))
        assert rg <= eb.C_BAR[dtype] and rf <= eb.C_COST[dtype], (tag, rg, rf)
    # ... and not the reference's fused regulariser
    assert not np.array_equal(g_t, ref_p.eval(x)[1])


# ---------------------------------------------------------------- solves
@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "reg_exact_table.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def table_inputs():
    return rx.table_inputs()


@pytest.mark.parametrize("solver", ["cg", "lbfgs"])
@pytest.mark.parametrize("row", range(len(rx.TABLE_ROWS)), ids=["R%d-lambda%g" % rl for rl in rx.TABLE_ROWS])
def test_solves_of_the_table(sr, ctx, table, table_inputs, row, solver):
    """srmap_solve (f64) on the table's input with both gradient modes against tests/golden/reg_exact_table.json: the
    restatement's IRLS rounds / iterations / evaluations on every solve the generator found stable, the PSNR within ten
    times what moving the observations by 1e-13 moved the restatement's."""
    inp = table_inputs
    R, lam = rx.TABLE_ROWS[row]
    r = table["rows"][row]
    C, H, W = inp["x0"].shape
    for name, mode in (("reference", sr.REG_GRADIENT_REFERENCE), ("exact", sr.REG_GRADIENT_EXACT)):
        want = r[solver + "_" + name]
        p = sr.Problem(ctx, W, H, C, len(inp["shifts"]), inp["s"], inp["shifts"], 3, 1.0, sr.F64)
        p.set_observations(inp["y"])
        p.add_regularizer(sr.REG_BTV, lam, R, rx.TABLE_DECAY)
        p.set_regularizer_gradient(0, mode)
        if solver == "lbfgs":
            p.set_solver(sr.SOLVER_LBFGS, 5)
        x, rep = p.solve(inp["x0"])
        psnr, counts = float(orc.psnr(inp["gt"], x)), [rep.irls_rounds, rep.cg_iterations, rep.evaluations]
        print("R %d lambda %g %s %s: %.6f dB %s; table %.6f dB %s, stable %s, moved by %.1e; |GPU - table| %.1e"
              % (R, lam, solver, name, psnr, counts, want["psnr"], want["counts"], want["stable"], want["psnr_moved_by"],
                 abs(psnr - want["psnr"])))
        if want["stable"]:
            assert counts == want["counts"], (name, counts, want["counts"])
        assert abs(psnr - want["psnr"]) <= 10.0 * want["psnr_moved_by"], (name, psnr, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_split_channels_with_3d_tv(sr, ctx, dtype):
    """split_channels solves one channel at a time: a one-channel view has no next channel, so exact 3-D TV is the
    reference's there, bit for bit -- and it differs from it in the joint solve."""
    outs = {}
    for split in (1, 0):
        for mode in (sr.REG_GRADIENT_REFERENCE, sr.REG_GRADIENT_EXACT):
            p, x, _, _, _ = _data_problem(sr, ctx, dtype, rm.TV3D, 0, C=3, H=16, W=32)
            p.set_regularizer_gradient(0, mode)
            o = _few_iterations(sr)
            o.split_channels = split
            outs[(split, mode)] = p.solve(x, o)[0]
            assert np.all(np.isfinite(outs[(split, mode)]))
    assert np.array_equal(outs[(1, 0)], outs[(1, 1)])
    assert not np.array_equal(outs[(0, 0)], outs[(0, 1)])


def test_lambda_path_with_exact_gradient(sr, ctx, table_inputs):
    """a one-row path is bit for bit the calls it is made of, with the mode in force throughout and afterwards"""
    inp = table_inputs
    C, H, W = inp["x0"].shape

    def make(mode):
        p = sr.Problem(ctx, W, H, C, len(inp["shifts"]), inp["s"], inp["shifts"], 3, 1.0, sr.F64)
        p.set_observations(inp["y"])
        p.add_regularizer(sr.REG_BTV, 0.02, 1, 0.5)
        p.set_regularizer_gradient(0, mode)
        p.set_holdout(0.1, 5)
        return p
    p, twin, other = make(sr.REG_GRADIENT_EXACT), make(sr.REG_GRADIENT_EXACT), make(sr.REG_GRADIENT_REFERENCE)
    x, tab, chosen, _ = p.solve_lambda_path(inp["x0"], [0.5], final_solve=False)
    assert p.regularizer_gradient(0) == sr.REG_GRADIENT_EXACT and p.regularizer_lambda(0) == 0.01
    twin.set_regularizer_lambda(0, 0.01)
    xt, rep = twin.solve(inp["x0"])
    assert np.array_equal(x, xt) and [int(v) for v in tab[0, 6:9]] == [rep.irls_rounds, rep.cg_iterations, rep.evaluations]
    xo, tabo, _, _ = other.solve_lambda_path(inp["x0"], [0.5], final_solve=False)
    # BTV of range 1: the reference's gradient leaves the regulariser out, the exact one regularises -- a better score
    assert tab[0, 1] < tabo[0, 1]


# ---------------------------------------------------------------- outside the library
def test_host_facade_sets_the_mode_as_the_c_calls_do():
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "super-resolution_amd", "lib", "reg_exact_facade_test")
    assert os.path.exists(exe), "build() makes the facade test binary"
    o = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    print(o.stdout, o.stderr)
    assert o.returncode == 0 and "REG EXACT FACADE TESTS PASSED" in o.stdout


def test_command_line_flag(tmp_path):
    """super_resolution --regularizer_gradient on the tool's own generated frames (--generate_lr_images, noise sigma 8 / 255,
    BTV of range 1): `exact` regularises where the reference's gradient is zero -- a higher PSNR --, `reference` is the run
    without the flag, line for line, and an unknown word is refused before any GPU work, with the flag's name."""
    import subprocess
    from conftest import ROOT
    from test_gpu_apps import _ground_truth, _write_envi
    srbin = os.path.join(ROOT, "super-resolution_amd", "lib", "super_resolution")
    assert os.path.exists(srbin), "build() makes the tools"
    C, H, W, s, K = 1, 48, 64, 2, 4
    gt_cfg = _write_envi(str(tmp_path / "gt"), _ground_truth(C, H, W))
    motion = tmp_path / "motion.txt"
    motion.write_text("0 0\n1 1\n0 1\n1 0\n")
    base = [srbin, "--data_path=" + gt_cfg, "--generate_lr_images", "--number_of_frames=%d" % K, "--noise_sigma=8", "--noise_seed=3",
            "--upsampling_scale=%d" % s, "--blur_radius=3", "--blur_sigma=1.0", "--motion_sequence_path=" + str(motion),
            "--regularizer=btv", "--btv_scale_range=1", "--regularization_parameter=0.02", "--optimization_iterations=5",
            "--solver_iterations=30", "--evaluators=psnr"]

    def run(*flags):
        o = subprocess.run(base + list(flags), capture_output=True, text=True, timeout=300)
        print(o.stdout, o.stderr)
        return o

    def psnr(o):
        assert o.returncode == 0
        return float([l for l in o.stdout.splitlines() if l.startswith("PSNR score on result")][0].split(":")[1])

    plain, ref, exact = run(), run("--regularizer_gradient=reference"), run("--regularizer_gradient=exact")
    untimed = lambda o: [l for l in o.stdout.splitlines() if "seconds" not in l]  # all but the line that states the run time
    assert untimed(plain) == untimed(ref) and len(untimed(plain)) >= 2
    assert psnr(exact) > psnr(plain) + 1.0
    bad = run("--regularizer_gradient=Exact")
    assert bad.returncode != 0 and "--regularizer_gradient is reference or exact" in (bad.stdout + bad.stderr)
    assert "PSNR" not in bad.stdout
