"""Runs the reference's vendored ALGLIB 3.10.0 nonlinear CG (compiled from
/root/reference by oracle/Makefile into oracle/_ref/libalglib_ref.so) on two
small objectives and stores the trajectories as tests/golden/cg_trajectories.json:
every point reported through the xupdated callback, its cost, the final x,
iteration count, nfev and termination type -- and, under "alglib_live", what ALGLIB
returns on the inputs of the tests that compare the restatement with it live
(test_oracle_cg.py).  Inputs are seeded and stored too,
so the fixture is self-contained on machines without /root/reference.

    python tests/golden/make_cg_trajectories.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as orc  # noqa: E402


def quad_problem():
    rng = np.random.default_rng(7)
    B = rng.standard_normal((16, 16))
    A = B @ B.T + 0.5 * np.eye(16)
    b = rng.standard_normal(16)
    return A, b


def rosen_like(A, b):
    """Non-quadratic objective of tests/test_oracle_cg.py::test_live_alglib_bit_exact.  Products and sums are
    elementwise numpy (no BLAS), so its values are the same bits on every host."""
    def fun(v):
        Av = (A * v).sum(axis=1)
        return 0.5 * (v * Av).sum() - (b * v).sum() + 0.1 * (v * v * v * v).sum(), Av - b + 0.4 * (v * v * v)
    return fun


def toy_problem(T):
    model = orc.ImageModel(scale=T["scale"], shifts=T["shifts"], blur_ksize=T["blur"][0], blur_sigma=T["blur"][1])
    gt = np.array(T["gt"])
    prob = orc.Problem(model, np.stack([model.apply(gt, k) for k in range(len(T["shifts"]))]))
    prob.add_regularizer(orc.REG_TV, T["lambda"])
    prob.set_irls_weights(0, np.array(T["weights"]))
    return prob


def live_cases(toy):
    """What the reference's ALGLIB returns on the inputs of test_live_alglib_bit_exact and
    test_irls_solve_with_alglib_matches: the tests compare the restatement with it bit for bit when ALGLIB itself
    cannot be built."""
    def rec(x, rep, trace):
        return {"x": x.ravel().tolist(), "trace_f": [t[1] for t in trace], "iterations": rep.iterations,
                "nfev": rep.nfev, "termination_type": rep.termination_type, "f": rep.f}

    rng = np.random.default_rng(3)
    B = rng.standard_normal((24, 24))
    A = B @ B.T + np.eye(24)
    b = rng.standard_normal(24)
    x0 = rng.standard_normal(24) * 3
    trace = []
    x, rep = orc.mincg(rosen_like(A, b), x0, trace=trace, maxits=40, use_alglib=True)
    live = {"rosen_like": dict(rec(x, rep, trace), A=A.tolist(), b=b.tolist(), x0=x0.tolist())}
    x0 = rng.random(64)
    trace = []
    x, rep = orc.mincg(lambda v: toy_problem(toy).objective(v), x0, trace=trace, maxits=40, use_alglib=True)
    live["tv_toy_8x8"] = dict(rec(x, rep, trace), x0=x0.tolist())

    rng = np.random.default_rng(5)
    gt = rng.random((2, 12, 12))
    shifts = [[0, 0], [1, 0], [0, 1], [1, 1], [2, 1]]
    model = orc.ImageModel(scale=3, shifts=shifts, blur_ksize=3, blur_sigma=1.0)
    prob = orc.Problem(model, np.stack([model.apply(gt, k) for k in range(5)]))
    prob.add_regularizer(orc.REG_BTV, 0.01, btv_range=3, btv_decay=0.5)
    opts = orc.default_irls_options()
    opts.max_num_irls_iterations = 3
    x, rep = prob.solve(np.full((2, 12, 12), 0.5), opts, use_alglib=True)
    live["irls_btv_12x12"] = {"x": x.ravel().tolist(), "cg_iterations": rep.cg_iterations, "nfev": rep.nfev,
                              "final_cost": rep.final_cost}
    return live


def main():
    assert orc.have_ref(), "oracle/_ref/libalglib_ref.so missing (needs /root/reference)"
    out = {}
    A, b = quad_problem()

    def quad(x):
        return 0.5 * x @ A @ x - b @ x, A @ x - b

    for name, kw in (("quadratic16_default", dict(epsg=1e-6, epsf=1e-6, epsx=1e-6, maxits=50)),
                     ("quadratic16_tight", dict(epsg=1e-10, epsf=0.0, epsx=0.0, maxits=200))):
        trace = []
        x, rep = orc.mincg(quad, np.zeros(16), use_alglib=True, trace=trace, **kw)
        out[name] = {"A": A.tolist(), "b": b.tolist(), "x0": [0.0] * 16, "opts": kw,
                     "trace_f": [t[1] for t in trace], "trace_x": [t[0].tolist() for t in trace],
                     "x": x.tolist(), "iterations": rep.iterations, "nfev": rep.nfev,
                     "termination_type": rep.termination_type, "f": rep.f}

    # 8x8 HR, scale 2, 4 frames, blur 3/1.0, TV lambda 0.05 with non-unit weights
    rng = np.random.default_rng(11)
    gt = rng.random((1, 8, 8))
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    model = orc.ImageModel(scale=2, shifts=shifts, blur_ksize=3, blur_sigma=1.0)
    lr = np.stack([model.apply(gt, k) for k in range(4)])
    prob = orc.Problem(model, lr)
    prob.add_regularizer(orc.REG_TV, 0.05)
    w = 0.5 + rng.random((1, 8, 8))
    prob.set_irls_weights(0, w)
    x0 = rng.random(64)
    trace = []
    kw = dict(epsg=1e-6, epsf=1e-6, epsx=1e-6, maxits=50)
    x, rep = orc.mincg(lambda v: prob.objective(v), x0, use_alglib=True, trace=trace, **kw)
    out["tv_toy_8x8"] = {"gt": gt.tolist(), "shifts": shifts, "scale": 2, "blur": [3, 1.0],
                         "lambda": 0.05, "weights": w.tolist(), "x0": x0.tolist(), "opts": kw,
                         "trace_f": [t[1] for t in trace], "x": x.tolist(),
                         "iterations": rep.iterations, "nfev": rep.nfev,
                         "termination_type": rep.termination_type, "f": rep.f}
    out["alglib_live"] = live_cases(out["tv_toy_8x8"])
    with open(os.path.join(HERE, "cg_trajectories.json"), "w") as f:
        json.dump(out, f)
    for k, v in list(out.items()) + list(out["alglib_live"].items()):
        if "iterations" in v:
            print(k, v["iterations"], v["nfev"], v["termination_type"], v["f"])
        elif k != "alglib_live":
            print(k, v["cg_iterations"], v["nfev"], v["final_cost"])


if __name__ == "__main__":
    main()
