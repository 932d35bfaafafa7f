"""The oracle's nonlinear-CG restatement (sro_mincg) against trajectories of the
reference's vendored ALGLIB 3.10.0 (tests/golden/cg_trajectories.json, made by
tests/golden/make_cg_trajectories.py): recorded, and live as well when oracle/_ref
is present."""
import json
import os

import numpy as np
import pytest

import oracle as orc
from conftest import GOLDEN


@pytest.fixture(scope="module")
def traj():
    with open(os.path.join(GOLDEN, "cg_trajectories.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["quadratic16_default", "quadratic16_tight"])
def test_quadratic_trajectory(traj, name):
    T = traj[name]
    A, b = np.array(T["A"]), np.array(T["b"])
    trace = []
    x, rep = orc.mincg(lambda v: (0.5 * v @ A @ v - b @ v, A @ v - b), np.array(T["x0"]), trace=trace, **T["opts"])
    assert rep.iterations == T["iterations"]
    assert rep.nfev == T["nfev"]
    assert rep.termination_type == T["termination_type"]
    assert len(trace) == len(T["trace_f"])
    # same operations in the same order: bit-exact on this platform, but allow
    # libm/BLAS differences in the numpy objective across hosts
    assert np.allclose([t[1] for t in trace], T["trace_f"], rtol=1e-12, atol=1e-14)
    assert np.allclose(x, T["x"], rtol=1e-9, atol=1e-12)
    assert rep.f == pytest.approx(T["f"], rel=1e-12)


def _toy(T):
    model = orc.ImageModel(scale=T["scale"], shifts=T["shifts"], blur_ksize=T["blur"][0], blur_sigma=T["blur"][1])
    gt = np.array(T["gt"])
    lr = np.stack([model.apply(gt, k) for k in range(len(T["shifts"]))])
    prob = orc.Problem(model, lr)
    prob.add_regularizer(orc.REG_TV, T["lambda"])
    prob.set_irls_weights(0, np.array(T["weights"]))
    return prob


def test_tv_toy_trajectory(traj):
    T = traj["tv_toy_8x8"]
    prob = _toy(T)
    trace = []
    x, rep = orc.mincg(lambda v: prob.objective(v), np.array(T["x0"]), trace=trace, **T["opts"])
    assert (rep.iterations, rep.nfev, rep.termination_type) == (T["iterations"], T["nfev"], T["termination_type"])
    assert np.allclose([t[1] for t in trace], T["trace_f"], rtol=1e-12, atol=0)
    assert np.allclose(x, T["x"], rtol=1e-9, atol=1e-12)


def _rosen_like(A, b):
    """Non-quadratic, exercises the bracketing cases.  Elementwise numpy only (no BLAS): the same bits on every host,
    as in tests/golden/make_cg_trajectories.py, which recorded ALGLIB on it."""
    def fun(v):
        Av = (A * v).sum(axis=1)
        return 0.5 * (v * Av).sum() - (b * v).sum() + 0.1 * (v * v * v * v).sum(), Av - b + 0.4 * (v * v * v)
    return fun


def _alglib_results(recorded, run):
    """ALGLIB's answers: the recorded ones (tests/golden, made by the reference's vendored ALGLIB) and, when
    oracle/_ref is built, the live ones of this process."""
    out = [("recorded", recorded)]
    if orc.have_ref():
        out.append(("live", run()))
    return out


def test_live_alglib_bit_exact(traj):
    """Restatement vs the real ALGLIB on the same objective: identical iterates (bit for bit)."""
    L = traj["alglib_live"]
    R = L["rosen_like"]
    cases = ((_rosen_like(np.array(R["A"]), np.array(R["b"])), np.array(R["x0"]), R),
             (lambda v: _toy(traj["tv_toy_8x8"]).objective(v), np.array(L["tv_toy_8x8"]["x0"]), L["tv_toy_8x8"]))
    for fun, x0, rec in cases:
        ta = []
        xa, ra = orc.mincg(fun, x0, trace=ta, maxits=40)

        def run():
            tb = []
            xb, rb = orc.mincg(fun, x0, trace=tb, maxits=40, use_alglib=True)
            return {"x": xb.tolist(), "trace_f": [t[1] for t in tb], "iterations": rb.iterations, "nfev": rb.nfev,
                    "termination_type": rb.termination_type, "f": rb.f}

        for how, b in _alglib_results(rec, run):
            assert (ra.iterations, ra.nfev, ra.termination_type) == (b["iterations"], b["nfev"], b["termination_type"]), how
            assert np.array_equal(xa, np.array(b["x"])), how
            assert [t[1] for t in ta] == b["trace_f"], how
            assert ra.f == b["f"], how


def test_irls_solve_with_alglib_matches(traj):
    """IRLS loop driven by the real ALGLIB == driven by the restatement."""
    rng = np.random.default_rng(5)
    gt = rng.random((2, 12, 12))
    shifts = [[0, 0], [1, 0], [0, 1], [1, 1], [2, 1]]
    model = orc.ImageModel(scale=3, shifts=shifts, blur_ksize=3, blur_sigma=1.0)
    lr = np.stack([model.apply(gt, k) for k in range(5)])

    def solve(use):
        prob = orc.Problem(model, lr)
        prob.add_regularizer(orc.REG_BTV, 0.01, btv_range=3, btv_decay=0.5)
        opts = orc.default_irls_options()
        opts.max_num_irls_iterations = 3
        x, rep = prob.solve(np.full((2, 12, 12), 0.5), opts, use_alglib=use)
        return {"x": x.ravel().tolist(), "cg_iterations": rep.cg_iterations, "nfev": rep.nfev,
                "final_cost": rep.final_cost}

    a = solve(False)
    for how, b in _alglib_results(traj["alglib_live"]["irls_btv_12x12"], lambda: solve(True)):
        assert (a["cg_iterations"], a["nfev"], a["final_cost"]) == (b["cg_iterations"], b["nfev"], b["final_cost"]), how
        assert np.array_equal(np.array(a["x"]), np.array(b["x"])), how
