"""The solver's n-vector passes over their covering matrix (tests/solver_matrix.py): run_cg and run_lbfgs on every cell
against ALGLIB's mincg (oracle/_ref when built, else the restatement, which is bit-exact against it) and the minlbfgs
restatement (tests/lbfgs_restatement.py).

f64: both references run on the oracle objective; the bars of the existing trajectory tests (same iterations, nfev and
termination; the cost of every accepted iterate in the GPU's evaluation log to 1e-11; x to 1e-8).  A large cell that
misses them is held to 10x the reference's own change under a 1e-14 perturbation of x0 instead (the rule of
test_cfg1_solve_matches_oracle), logged.
f32: the references run on the GPU's own f32 evaluation (p32.eval), L-BFGS with x, g, s, y and d rounded where the
device stores them, so that only the solver arithmetic differs; same counts, accepted costs and final x within 10x the
reference's own spread under a one-ulp perturbation of x0.
IRLS: whole solves with a BTV regulariser at an odd-n, three-channel geometry against the oracle's IRLS loop."""
import os
import sys

import numpy as np
import pytest

import oracle as orc
import parity_log

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_restatement as lbr  # noqa: E402
import solver_matrix as sm  # noqa: E402

pytestmark = pytest.mark.gpu

CELLS = sm.cells()


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


_DATA = {}
_REFS = {}
_F32 = {}


def _data(name):
    """(model, lr, x0, oracle problem) per geometry, shared by every cell on it."""
    if name not in _DATA:
        geo = sm.GEOS[name]
        model, lr, x0 = sm.data(geo)
        _DATA[name] = (model, lr, x0, sm.oracle_problem(geo, model, lr))
    return _DATA[name]


def _problem(sr, ctx, geo, dtype, impl, lr):
    p = sr.Problem(ctx, geo.W, geo.H, geo.C, geo.K, geo.s, geo.shifts(), geo.blur, 1.0 if geo.blur > 1 else 0.0,
                   sr.F64 if dtype == sm.F64 else sr.F32)
    p.set_impl(sr.IMPL_AUTO if impl == sm.IMPL_AUTO else sr.IMPL_DIRECT)
    p.set_observations(lr)
    if geo.tv > 0:
        p.add_regularizer(sr.REG_TV, geo.tv)
        p.set_irls_weights(0, np.ones((geo.C, geo.H, geo.W)))
    assert p.active_impl() == (sr.IMPL_TILED if geo.folds(impl) else sr.IMPL_DIRECT), "the mirror's tile rule is off"
    return p


def _fun(geo, dtype, prob):
    shape = (geo.C, geo.H, geo.W)
    if dtype == sm.F64:
        return lambda v: (lambda fg: (fg[0], fg[1].ravel()))(prob.objective(v.reshape(shape)))
    return lambda v: (lambda fg: (fg[0], fg[1].ravel()))(prob.eval(v.reshape(shape)))


def _ref(fun, x0, sol, m, eps, maxits, store=None):
    """(x, (iterations, nfev, termination), evaluation log, accepted costs) of the reference."""
    xrep, trace = [], []
    if sol == "cg":
        x, rep = orc.mincg(fun, x0, *eps, maxits, use_alglib=orc.have_ref(), trace=xrep)
    else:
        x, rep = lbr.minlbfgs(fun, x0, m, *eps, maxits, trace=trace, xrep=xrep, store=store)
    return x, (rep.iterations, rep.nfev, rep.termination_type), trace, [f for _, f in xrep], xrep


def _probe(fun, x0, sol, m, store):
    """(f, |g|, |x_i - x_{i-1}|) of every accepted iterate of an eps = 0 run (solver_matrix.eps_for)."""
    xrep = _ref(fun, x0, sol, m, (0.0, 0.0, 0.0), 40, store)[4]
    out, prev = [], None
    for x, f in xrep:
        g = fun(np.asarray(x).copy())[1]
        out.append((f, float(np.sqrt(np.sum(np.square(g)))), 0.0 if prev is None else float(np.sqrt(np.sum(np.square(x - prev))))))
        prev = x
    return out


def _gpu(p, x0, sol, m, eps, maxits):
    if sol == "cg":
        x, its, nfev, term, ft = p.cg_trace(x0, *eps, maxits)
    else:
        x, its, nfev, term, ft = p.lbfgs_trace(x0, m, *eps, maxits)
    return x.ravel(), (its, nfev, term), ft, None


@pytest.mark.parametrize("cell", CELLS, ids=[sm.cell_id(c) for c in CELLS])
def test_solver_pass_trajectory(sr, ctx, cell):
    name, dtype, impl, sol, m, maxits, term = cell
    geo = sm.GEOS[name]
    model, lr, x0, prob = _data(name)
    d = geo.dispatch(dtype)
    p = _problem(sr, ctx, geo, dtype, impl, lr)
    store = None if dtype == sm.F64 else np.float32
    # f64: one reference per (geometry, run), shared by both impls; f32: per impl (its own evaluation drives it)
    fun = _fun(geo, dtype, prob if dtype == sm.F64 else p)
    key = (name, dtype, impl if dtype == sm.F32 else None, sol, m, maxits, term)
    if key not in _REFS:
        eps = (0.0, 0.0, 0.0) if term == 5 else sm.eps_for(term, _probe(fun, x0.ravel(), sol, m, store))
        _REFS[key] = (eps, _ref(fun, x0.ravel(), sol, m, eps, maxits, store))
    eps, ref = _REFS[key]
    run = _gpu(p, x0, sol, m, eps, maxits)
    same, ef, ex = sm.compare(run, ref)
    live = sm.live_seq(m, ref[1][0]) if m else []
    print("%s: n %d V %d nb %d busy %d rounds %d %s fold %s | counts GPU %s ref %s | live max %s | f %.3e x %.3e" % (
        sm.cell_id(cell), d["n"], d["V"], d["nb"], d["busy"], d["rounds"], d["axpy"], geo.folds(impl), run[1], ref[1],
        max(live) if live else "-", ef, ex))
    assert ref[1][2] == term, "the reference did not end by the cell's termination type"
    assert len(run[2]) == run[1][1]
    if dtype == sm.F64:
        f_bar, x_bar = sm.F64_F_BAR, sm.F64_X_BAR
        if not (same and ef <= f_bar and ex <= x_bar) and geo.n > 100000:
            rng = np.random.default_rng(1)
            pert = _ref(fun, (x0 * (1 + 1e-14 * rng.standard_normal(x0.shape))).ravel(), sol, m, eps, maxits)
            assert pert[1] == ref[1], "the reference's own counts move under a 1e-14 perturbation: ill-conditioned cell"
            own_f = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(pert[3][1:], ref[3][1:]))
            own_x = sm.xerr(pert[0], ref[0])
            f_bar, x_bar = max(f_bar, 10 * own_f), max(x_bar, 10 * own_x)
            parity_log.note(own_f, "own f")
            parity_log.note(own_x, "own x")
            print("wider bars from the reference's own change: f %.3e x %.3e" % (f_bar, x_bar))
    else:
        pkey = key + ("pert",)
        if pkey not in _F32:
            _F32[pkey] = sm.spread_bars(ref, _ref(fun, sm.f32_ulp_perturb(x0.ravel()), sol, m, eps, maxits, store),
                                        sm.F32_FLOOR)
        bars = _F32[pkey]
        assert bars is not None, "the reference's own counts move under a one-ulp perturbation: ill-conditioned cell"
        f_bar, x_bar, sf, sx = bars
        parity_log.note(sf, "spread f")
        parity_log.note(sx, "spread x")
        print("f32 bars f %.3e x %.3e (reference spread f %.3e x %.3e)" % (f_bar, x_bar, sf, sx))
    parity_log.note(ef, "f")
    parity_log.note(ex, "x")
    assert run[1] == ref[1]
    assert ef <= f_bar
    assert ex <= x_bar


def _irls_case():
    geo = sm.GEOS["odd3"]
    rng = np.random.default_rng(3)
    model = orc.ImageModel(scale=geo.s, shifts=geo.shifts(), blur_ksize=3, blur_sigma=1.0)
    gt = rng.random((geo.C, geo.H, geo.W))
    lr = np.stack([model.apply(gt, k) for k in range(geo.K)]) + 0.01 * rng.standard_normal((geo.K, geo.C, geo.h(), geo.w()))
    x0 = np.stack([orc.resize_nearest(lr[0, c], geo.W, geo.H) for c in range(geo.C)])
    return geo, model, gt, lr, x0, (orc.REG_BTV, 0.01, 2, 0.5)


@pytest.mark.parametrize("dtype", [sm.F64, sm.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("sol", ["cg", "lbfgs"])
def test_irls_solve_odd_n_three_channels(sr, ctx, sol, dtype):
    """A whole IRLS solve (every round restarts the ring and the reductions) against the oracle's IRLS loop with the same
    inner solver: f64 to the bars of test_gpu_lbfgs.py::_compare, f32 to the f32 solve's PSNR bar (0.05 dB) and cost."""
    geo, model, gt, lr, x0, reg = _irls_case()
    ref = orc.Problem(model, lr)
    ref.add_regularizer(*reg)
    if sol == "cg":
        x_ref, rr = ref.solve(x0, use_alglib=orc.have_ref())
    else:
        x_ref, rr = lbr.oracle_solve(ref, x0, m=5)
    p = sr.Problem(ctx, geo.W, geo.H, geo.C, geo.K, geo.s, geo.shifts(), 3, 1.0, sr.F64 if dtype == sm.F64 else sr.F32)
    p.set_observations(lr)
    p.add_regularizer(*reg)
    p.set_solver(sr.SOLVER_CG if sol == "cg" else sr.SOLVER_LBFGS, 5)
    x, rep = p.solve(x0)
    dpsnr = abs(orc.psnr(gt, x) - orc.psnr(gt, x_ref))
    dcost = abs(rep.final_cost - rr.final_cost) / abs(rr.final_cost)
    dx = float(np.max(np.abs(x - x_ref)))
    print("n %d: IRLS rounds %d/%d, iterations %d/%d, evaluations %d/%d, PSNR %.3e cost %.3e x %.3e" % (
        geo.n, rep.irls_rounds, rr.irls_rounds, rep.cg_iterations, rr.cg_iterations, rep.evaluations, rr.nfev, dpsnr, dcost, dx))
    parity_log.note(dpsnr, "psnr")
    parity_log.note(dcost, "cost")
    parity_log.note(dx, "x")
    assert dpsnr < (0.01 if dtype == sm.F64 else 0.05)  # f32: test_solver_psnr_parity_with_cpu_reference's bar
    if dtype == sm.F64:
        assert (rep.irls_rounds, rep.cg_iterations, rep.evaluations) == (rr.irls_rounds, rr.cg_iterations, rr.nfev)
        assert dcost <= 1e-9
        assert dx <= 1e-7
    else:
        assert dcost <= 1e-4
