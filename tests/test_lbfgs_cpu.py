"""The numpy restatement of ALGLIB's L-BFGS (tests/lbfgs_restatement.py) against runs of the reference's vendored
ALGLIB 3.10.0 minlbfgs (tests/golden/lbfgs_trajectories.json, recorded by tests/golden/make_lbfgs_trajectories.py):
bit for bit.  The restatement is what the GPU L-BFGS tests compare the device solver with (tests/test_gpu_lbfgs.py)."""
import json
import os
import sys

import numpy as np
import pytest

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_restatement as lbr  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


LB = _load("lbfgs_trajectories.json")
CG = _load("cg_trajectories.json")


def _rosen_like(A, b):
    def fun(v):
        Av = (A * v).sum(axis=1)
        return 0.5 * (v * Av).sum() - (b * v).sum() + 0.1 * (v * v * v * v).sum(), Av - b + 0.4 * (v * v * v)
    return fun


def _objective(name):
    if name == "quadratic16":
        T = CG["quadratic16_default"]
        A, b = np.array(T["A"]), np.array(T["b"])
        return lambda v: (0.5 * v @ A @ v - b @ v, A @ v - b)
    if name == "rosen_like":
        T = CG["alglib_live"]["rosen_like"]
        return _rosen_like(np.array(T["A"]), np.array(T["b"]))
    T = CG["tv_toy_8x8"]
    model = orc.ImageModel(scale=T["scale"], shifts=T["shifts"], blur_ksize=T["blur"][0], blur_sigma=T["blur"][1])
    gt = np.array(T["gt"])
    prob = orc.Problem(model, np.stack([model.apply(gt, k) for k in range(len(T["shifts"]))]))
    prob.add_regularizer(orc.REG_TV, T["lambda"])
    prob.set_irls_weights(0, np.array(T["weights"]))
    return lambda v: prob.objective(v)


def test_fixture_covers_the_issue_matrix():
    cases = LB["cases"].values()
    assert {c["m"] for c in cases} >= {1, 3, 5, 7}
    assert {c["objective"] for c in cases} == {"quadratic16", "rosen_like", "tv_toy_8x8"}
    terms = {c["termination_type"] for c in cases}
    assert 5 in terms and (terms & {1, 4})
    assert "provenance" in LB


@pytest.mark.parametrize("name", sorted(LB["cases"]))
def test_restatement_bit_exact(name):
    T = LB["cases"][name]
    xrep = []
    x, rep = lbr.minlbfgs(_objective(T["objective"]), np.array(T["x0"]), T["m"], trace=None, xrep=xrep, **T["opts"])
    assert (rep.iterations, rep.nfev, rep.termination_type) == (T["iterations"], T["nfev"], T["termination_type"])
    assert [f for _, f in xrep] == T["trace_f"]
    assert x.tolist() == T["x"]
    assert rep.f == T["f"]


def test_trace_logs_every_evaluation():
    T = LB["cases"]["rosen_like_m5"]
    trace, xrep = [], []
    _, rep = lbr.minlbfgs(_objective("rosen_like"), np.array(T["x0"]), 5, trace=trace, xrep=xrep, **T["opts"])
    assert len(trace) == rep.nfev
    assert all(f in trace for _, f in xrep)


def test_adapter_drives_the_oracle_irls_solve_on_configs0():
    """configs[0] (4 frames, 2x, TV 0.01, the reference motion order; 256 x 256 HR): the oracle's IRLS loop runs
    to its end with L-BFGS as the inner solver, and the last inner run is the restatement's own run on the last
    weights."""
    import bench
    s, K, W, H = 2, 4, 256, 256
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    gt = bench.synth_ground_truth(W, H, 1)
    model = orc.ImageModel(scale=s, shifts=shifts)
    lr = np.stack([model.apply(gt, k) for k in range(K)])
    lr = lr + (5.0 / 255.0) * np.random.default_rng(777).standard_normal(lr.shape)
    x0 = bench.bilinear_upsample(lr[0], s)
    prob = orc.Problem(model, lr)
    prob.add_regularizer(orc.REG_TV, 0.01)
    x, rep = lbr.oracle_solve(prob, x0, m=5)
    x_cg, rep_cg = prob.solve(x0)
    print("L-BFGS: IRLS rounds %d, iterations %d, nfev %d, cost %.10g, PSNR %.4f | CG: %d, %d, %d, %.10g, PSNR %.4f" % (
        rep.irls_rounds, rep.cg_iterations, rep.nfev, rep.final_cost, orc.psnr(gt, x), rep_cg.irls_rounds,
        rep_cg.cg_iterations, rep_cg.nfev, rep_cg.final_cost, orc.psnr(gt, x_cg)))
    assert rep.irls_rounds >= 1 and rep.cg_iterations >= rep.irls_rounds and rep.nfev > rep.cg_iterations
    assert np.all(np.isfinite(x))
    assert orc.psnr(gt, x) > orc.psnr(gt, x0)
    # the two minimisers reach the same IRLS minimiser to within the stopping thresholds
    assert abs(orc.psnr(gt, x) - orc.psnr(gt, x_cg)) < 0.5
