"""Records the reference's vendored ALGLIB 3.10.0 L-BFGS (minlbfgs) on small objectives and stores the runs as
tests/golden/lbfgs_trajectories.json: for every case its inputs, the cost of every point reported through the xupdated
callback, the final x, iteration count, nfev and termination type.  The fixture is self-contained: the tests need
neither ALGLIB nor this script.

    python tests/golden/make_lbfgs_trajectories.py DRIVER.so

DRIVER.so is a shared library, linked against ALGLIB's optimisation unit, that exports

    void ref_minlbfgs(int n, int m, double* x, double epsg, double epsf, double epsx, int maxits,
                      sro_fg_fn fg, sro_rep_fn rep, void* ctx, sro_cg_report* report);

and drives minlbfgscreate(m) / minlbfgssetcond / minlbfgssetxrep(true) / minlbfgsoptimize / minlbfgsresults as the
reference does (src/optimization/alglib_objective.cpp:111-140), with the types of oracle/srmap_oracle.h.  It is not
part of this repository."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import oracle as orc  # noqa: E402
from make_cg_trajectories import quad_problem, rosen_like, toy_problem  # noqa: E402

MS = (1, 3, 5, 7)


def run(lib, fun, x0, m, epsg, epsf, epsx, maxits):
    x = np.array(x0, dtype=np.float64).ravel().copy()
    n = x.size
    trace = []

    def _fg(_ctx, px, pg):
        f, g = fun(np.ctypeslib.as_array(px, shape=(n,)).copy())
        np.ctypeslib.as_array(pg, shape=(n,))[:] = g
        return float(f)

    def _rep(_ctx, px, f):
        trace.append(float(f))

    rep = orc.CgReport()
    lib.ref_minlbfgs(n, m, x.ctypes.data_as(orc.c_double_p), epsg, epsf, epsx, maxits, orc.FG_FN(_fg), orc.REP_FN(_rep),
                     None, C.byref(rep))
    return {"m": m, "opts": dict(epsg=epsg, epsf=epsf, epsx=epsx, maxits=maxits), "x0": np.asarray(x0).ravel().tolist(),
            "trace_f": trace, "x": x.tolist(), "iterations": rep.iterations, "nfev": rep.nfev,
            "termination_type": rep.termination_type, "f": rep.f}


def main(driver):
    lib = C.CDLL(os.path.abspath(driver))
    lib.ref_minlbfgs.argtypes = [C.c_int, C.c_int, orc.c_double_p, C.c_double, C.c_double, C.c_double, C.c_int,
                                 orc.FG_FN, orc.REP_FN, C.c_void_p, C.POINTER(orc.CgReport)]
    with open(os.path.join(HERE, "cg_trajectories.json")) as f:
        cg = json.load(f)
    A, b = quad_problem()

    def quad(x):
        return 0.5 * x @ A @ x - b @ x, A @ x - b

    rl = cg["alglib_live"]["rosen_like"]
    Ar, br = np.array(rl["A"]), np.array(rl["b"])
    toy = cg["tv_toy_8x8"]
    prob = toy_problem(toy)
    objectives = {
        "quadratic16": (quad, np.zeros(16)),
        "rosen_like": (rosen_like(Ar, br), np.array(rl["x0"])),
        "tv_toy_8x8": (lambda v: prob.objective(v), np.array(toy["x0"])),
    }
    cases = {}
    for name, (fun, x0) in objectives.items():
        for m in MS:
            cases["%s_m%d" % (name, m)] = dict(run(lib, fun, x0, m, 1e-6, 1e-6, 1e-6, 50), objective=name)
    # ends on maxits; tight epsg with epsf = epsx = 0
    cases["rosen_like_m5_maxits"] = dict(run(lib, objectives["rosen_like"][0], objectives["rosen_like"][1], 5, 0.0, 0.0,
                                             0.0, 6), objective="rosen_like")
    cases["quadratic16_m3_tight"] = dict(run(lib, quad, np.zeros(16), 3, 1e-10, 0.0, 0.0, 200), objective="quadratic16")
    out = {"provenance": "ALGLIB 3.10.0 minlbfgs as vendored by the reference (libs/alglib/src/optimization.cpp), "
                         "compiled with -O2 -ffp-contract=off, driven as alglib_objective.cpp:111-140 drives it; "
                         "recorded by tests/golden/make_lbfgs_trajectories.py.  Objectives: quadratic16 and the "
                         "rosen_like inputs of cg_trajectories.json (quad_problem, alglib_live.rosen_like), and the "
                         "TV toy problem tv_toy_8x8 of cg_trajectories.json.",
           "cases": cases}
    with open(os.path.join(HERE, "lbfgs_trajectories.json"), "w") as f:
        json.dump(out, f)
    for k, v in cases.items():
        print(k, v["iterations"], v["nfev"], v["termination_type"], v["f"])


if __name__ == "__main__":
    main(sys.argv[1])
