"""The solver matrix (tests/solver_matrix.py) without a GPU: its cells reach every dispatch the issue of the solver passes
lists, every geometry is one the oracle accepts, and plausible pass bugs planted in the minlbfgs restatement
(tests/lbfgs_restatement.py plant=...) fail the bars of tests/test_gpu_solver_matrix.py on the cells meant to catch them,
in f64 and with the device's f32 storage (store=np.float32)."""
import os
import sys

import numpy as np
import pytest

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_restatement as lbr  # noqa: E402
import solver_matrix as sm  # noqa: E402

F64, F32 = sm.F64, sm.F32
CELLS = sm.cells()
_DATA = {}


def _fun(name):
    if name not in _DATA:
        geo = sm.GEOS[name]
        model, lr, x0 = sm.data(geo)
        prob = sm.oracle_problem(geo, model, lr)
        shape = (geo.C, geo.H, geo.W)
        _DATA[name] = (lambda v: (lambda fg: (fg[0], fg[1].ravel()))(prob.objective(v.reshape(shape))), x0.ravel())
    return _DATA[name]


def _run(name, m, maxits, store=None, plant=None, x0=None):
    fun, x = _fun(name)
    xrep, trace = [], []
    xs, rep = lbr.minlbfgs(fun, x if x0 is None else x0, m, 0.0, 0.0, 0.0, maxits, trace=trace, xrep=xrep, store=store,
                           plant=plant)
    return xs, (rep.iterations, rep.nfev, rep.termination_type), trace, [f for _, f in xrep], rep


def _dispatches(dtype):
    return [(c, sm.GEOS[c[0]].dispatch(dtype)) for c in CELLS if c[1] == dtype]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_matrix_reaches_every_dispatch_cell(dtype):
    ds = _dispatches(dtype)
    kv = sm.kvec(dtype)
    assert any(d["n"] < 64 and d["n"] % 2 == 1 for _, d in ds)
    rag = [d for _, d in ds if d["n"] % 4 == 2]
    assert rag and all(d["V"] == (2 if dtype == F64 else 1) for d in rag)
    assert any(d["n"] % 4 == 0 and d["V"] == kv and d["busy"] < d["nb"] for _, d in ds)
    for V in (kv, 1):
        big = [d for _, d in ds if d["V"] == V and d["nb"] == sm.RED_BLOCKS and d["rounds"] >= 2 and
               d["n"] % (sm.RED_BLOCKS * sm.BLOCK * V) != 0]
        assert big, (dtype, V)
    if dtype == F32:
        assert any(d["V"] == 4 and d["n"] > 1048576 and d["rounds"] >= 2 for _, d in ds)
    assert any(d["V"] == 1 and d["n"] > 262144 and d["n"] % 2 == 1 and d["rounds"] >= 2 for _, d in ds)
    geos = {sm.GEOS[c[0]] for c, _ in ds}
    assert {g.C for g in geos} >= {1, 3}
    assert {g.kind for g in geos} == {"phases", "subpix"}
    for c, d in ds:
        geo = sm.GEOS[c[0]]
        assert geo.C in (1, 3) or geo.n % 4 == 2
    # impl: the fold (IMPL_AUTO on a tile geometry) and the stored d (IMPL_DIRECT, and AUTO off the tile plan), both
    # trial-point passes on the stored-d path, sub-pixel included in the fold
    folded = {(c[0], c[3]) for c, _ in ds if sm.GEOS[c[0]].folds(c[2])}
    stored = [(c, d) for c, d in ds if not sm.GEOS[c[0]].folds(c[2])]
    assert {"cg", "lbfgs"} <= {s for _, s in folded}
    assert ("subpix", "cg") in folded and ("subpix", "lbfgs") in folded
    assert {d["axpy"] for c, d in stored if c[3] == "cg"} == {"k_axpy_out4", "k_axpy_out"}
    assert {d["axpy"] for c, d in stored if c[3] == "lbfgs"} == {"k_axpy_out4", "k_axpy_out"}
    # termination: 1, 2, 4 forced through eps, 5 through maxits, by both solvers
    for sol in ("cg", "lbfgs"):
        assert {c[6] for c, _ in ds if c[3] == sol} == {1, 2, 4, 5}


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_lbfgs_history_cells(dtype):
    """Per (T, V): one run with m = 8 that reaches live = 8, and one whose ring wraps at least twice (k >= 2 m + 1);
    every live = 1 .. 8 launched at both V.  The successful iterations are the restatement's on the oracle objective."""
    seen = {}
    for c, d in _dispatches(dtype):
        name, _, _, sol, m, maxits, term = c
        if sol != "lbfgs" or term != 5 or sm.GEOS[name].n > 100000:
            continue
        k = _run(name, m, maxits)[4].updates
        lives = set(sm.live_seq(m, k))
        s = seen.setdefault(d["V"], {"live": set(), "m8": False, "wrap2": False})
        s["live"] |= lives
        s["m8"] |= m == 8 and 8 in lives
        s["wrap2"] |= k >= 2 * m + 1
    assert set(seen) == {sm.kvec(dtype), 1}
    for V, s in seen.items():
        assert s["live"] == set(range(1, 9)) and s["m8"] and s["wrap2"], (V, s)


@pytest.mark.parametrize("name", sorted(sm.GEOS))
def test_oracle_accepts_every_geometry(name):
    geo = sm.GEOS[name]
    fun, x0 = _fun(name)
    f, g = fun(x0)
    assert np.isfinite(f) and g.shape == (geo.n,) and np.all(np.isfinite(g)) and np.any(g != 0)


def test_termination_cells_end_by_their_type():
    """The eps of every termination cell, derived from a probe run, ends the restatement and ALGLIB's mincg by that type
    (f64, oracle objective; the GPU file asserts the same for both dtypes)."""
    from test_gpu_solver_matrix import _probe, _ref
    fun, x0 = _fun(sm.TERM_GEO)
    for sol, m, maxits, term in sm.runs(sm.TERM_GEO):
        if term == 5:
            continue
        eps = sm.eps_for(term, _probe(fun, x0, sol, m, None))
        assert _ref(fun, x0, sol, m, eps, maxits)[1][2] == term, (sol, term)


# ---- planted bugs ----------------------------------------------------------------------------------------------------
def _caught(name, m, maxits, plant, store):
    """Whether the bars of the GPU file fail for the planted restatement against the clean one."""
    clean = _run(name, m, maxits, store)
    bad = _run(name, m, maxits, store, plant)
    if store is None:
        same, ef, ex = sm.compare(bad, clean)
        print("%s f64 %s: counts %s/%s f %.3e x %.3e" % (name, plant, bad[1], clean[1], ef, ex))
        return not sm.passes(bad, clean, sm.F64_F_BAR, sm.F64_X_BAR)
    pert = _run(name, m, maxits, store, x0=sm.f32_ulp_perturb(_fun(name)[1]))
    bars = sm.spread_bars(clean, pert, sm.F32_FLOOR)
    assert bars is not None, "the clean f32 restatement is ill-conditioned on %s" % name
    same, ef, ex = sm.compare(bad, clean)
    print("%s f32 %s: counts %s/%s f %.3e (bar %.3e) x %.3e (bar %.3e)" % (name, plant, bad[1], clean[1], ef, bars[0], ex,
                                                                           bars[1]))
    return not sm.passes(bad, clean, bars[0], bars[1])


def _tail(name, dtype):
    n = sm.GEOS[name].n
    return ("lose", n - n % sm.kvec(dtype))


PLANTS = [
    # the vector path taken on a ragged n: the last n % V elements left out (odd and 2 mod 4 cells)
    ("tail", "tiny", F64, 8, 12), ("tail", "odd3", F64, 2, 8), ("tail", "tiny", F32, 8, 12), ("tail", "rag2", F32, 2, 8),
    # elements past the first grid-stride round left out (multi-round cells)
    ("rounds", "bigodd", F64, 3, 6), ("rounds", "big2", F64, 3, 6), ("rounds", "bigodd", F32, 3, 6),
    # s_p.y_j and y_p.s_j swapped for j != p (live >= 2)
    # (on the TV cell: the data term alone is quadratic, its s_a.y_b = y_a.s_b, and the swap changes nothing there)
    ("swap", "tv", F64, 8, 12),
    # the oldest pair dropped once the ring has wrapped
    ("drop_oldest", "odd3", F64, 2, 8), ("drop_oldest", "subpix", F32, 2, 8),
]


@pytest.mark.parametrize("bug,name,dtype,m,maxits", PLANTS, ids=["%s-%s-%s" % (p[0], p[1], "f64" if p[2] == F64 else "f32")
                                                                 for p in PLANTS])
def test_planted_bug_fails_the_bars(bug, name, dtype, m, maxits):
    assert (name, dtype, sm.IMPL_AUTO, "lbfgs", m, maxits, 5) in CELLS
    d = sm.GEOS[name].dispatch(dtype)
    if bug == "tail":
        assert d["V"] == 1 and sm.GEOS[name].n % sm.kvec(dtype) != 0
        plant = _tail(name, dtype)
    elif bug == "rounds":
        assert d["rounds"] >= 2
        plant = ("lose", sm.first_round(d["n"], dtype))
    else:
        plant = (bug, None)
    store = None if dtype == F64 else np.float32
    assert _caught(name, m, maxits, plant, store)


def test_drop_oldest_needs_a_wrap():
    """The planted drop of the oldest pair changes nothing before the ring wraps: only the wrapping cells can catch it."""
    k = _run("odd3", 2, 2)[4].updates
    assert k <= 2
    assert not _caught("odd3", 2, 2, ("drop_oldest", None), None)


@pytest.mark.parametrize("name", ["rag2", "idle"])
def test_max_norm_as_a_sum_only_moves_rounding(name):
    """max|dn| reduced as a sum is a bug no trajectory bar can see: linminnormalized scales d by s1 = 1 / max|d| and
    then by 1 / |d s1|, and divides the step by both, so s1 cancels up to rounding.  The planted bug stays within the f64
    bars (a guard against reading the matrix as a check of that row of the direction pass's reduction)."""
    assert not _caught(name, 8, 12, ("maxsum", None), None)
