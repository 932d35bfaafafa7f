"""The covering matrix of the solver's n-vector passes (csrc/solver.hip run_cg / run_lbfgs; csrc/solver_passes.hip,
csrc/kernels_lbfgs.hip): a mirror of their dispatch, the geometries and solver settings that reach every cell of it, and the trajectory bars.
Shared by tests/test_gpu_solver_matrix.py (HIP against ALGLIB's mincg / the minlbfgs restatement) and
tests/test_solver_matrix_cpu.py (the matrix reaches every cell; planted bugs in the restatement fail the same bars).

Dispatch (DeviceCG): every pass runs nb = min(ceil(n / 256), 1024) workgroups of 256 threads, each thread V consecutive
elements per step, V = 16 / sizeof(T) when n % V == 0 else 1, striding by nb * 256 * V; only ceil(n / (256 V))
workgroups find work in the first round.  The line search's own trial-point pass is k_axpy_out4 when n % 4 == 0 else
k_axpy_out, and runs only where the evaluation does not form the trial point itself (the fold: tile plan, IMPL_AUTO).
Without the fold, k_normalize stores the normalised direction d.  L-BFGS launches its passes with live = min(k, m - 1) + 1
history pairs at its k-th successful iteration.
"""
import math

import numpy as np

BLOCK = 256
RED_BLOCKS = 1024
F64, F32 = 0, 1
IMPL_AUTO, IMPL_DIRECT = 0, 1
DTYPES = {F64: ("f64", 8, np.float64), F32: ("f32", 4, np.float32)}


def kvec(dtype):
    return 16 // DTYPES[dtype][1]


def vec(n, dtype):
    """DeviceCG::vec(): the width of the pass instances that run (kVec, or 1 on a ragged n)."""
    return kvec(dtype) if n % kvec(dtype) == 0 else 1


def nb(n):
    return min((n + BLOCK - 1) // BLOCK, RED_BLOCKS)


def rounds(n, dtype):
    """Grid-stride rounds of the busiest thread."""
    return -(-n // (nb(n) * BLOCK * vec(n, dtype)))


def busy(n, dtype):
    """Workgroups that find work in the first round."""
    return min(nb(n), -(-n // (BLOCK * vec(n, dtype))))


def first_round(n, dtype):
    """Elements the first grid-stride round covers."""
    return min(n, nb(n) * BLOCK * vec(n, dtype))


def axpy(n):
    return "k_axpy_out4" if n & 3 == 0 else "k_axpy_out"


def live_seq(m, ks):
    """live of the k-th successful L-BFGS iteration, k = 0 .. ks - 1."""
    return [min(k, m - 1) + 1 for k in range(ks)]


class Geo:
    """HR W x H x C, scale s, K frames, blur (ksize, sigma), shifts: 'phases' (integer, every phase of the first K) or
    'subpix' (uniform in (-1.5, 1.5), no rounding ties).  The data term is quadratic, so s_a.y_b = y_a.s_b there: a
    geometry with tv > 0 adds a TV term, the smooth non-quadratic part on which a transposed Gram table shows."""

    def __init__(self, name, s, W, H, C, K, shifts="phases", blur=3, tv=0.0):
        self.name, self.s, self.W, self.H, self.C, self.K, self.kind, self.blur = name, s, W, H, C, K, shifts, blur
        self.tv = tv  # lambda of a TV term (weights 1): 0 = data term only
        self.n = W * H * C

    def h(self):
        return self.H // self.s

    def w(self):
        return self.W // self.s

    def shifts(self):
        s, K = self.s, self.K
        if self.kind == "subpix":
            rng = np.random.default_rng(1000 + self.n)
            out = [[0.0, 0.0]] + [[float(rng.uniform(-1.5, 1.5)), float(rng.uniform(-1.5, 1.5))] for _ in range(K - 1)]
            return out
        return [[k % s - s // 2, (k // s) % s - s // 2] for k in range(K)]  # both signs: every border pixel is seen

    def reach(self):
        return int(math.ceil(max(max(abs(a), abs(b)) for a, b in self.shifts())))

    def tiles(self):
        """Whether ztile_plan accepts the geometry (ztile_plan.hip): 2 <= s <= 4, blur 1 / 3, a border frame that
        fits -- then IMPL_AUTO evaluates on the tile kernel, whose g.d instance forms the trial points (the fold)."""
        if not (2 <= self.s <= 4 and self.blur in (1, 3)):
            return False
        hb = self.blur // 2
        if self.kind == "subpix":
            Dr = self.reach() + 2 + hb
            return self.W > 4 * Dr + 2 * self.s and self.H > 4 * Dr + 2 * self.s
        return self.H > 4 * self.reach() + 2 * self.s

    def folds(self, impl):
        return impl == IMPL_AUTO and self.tiles()

    def dispatch(self, dtype):
        n = self.n
        return {"n": n, "V": vec(n, dtype), "nb": nb(n), "busy": busy(n, dtype), "rounds": rounds(n, dtype),
                "axpy": axpy(n)}

    def __repr__(self):
        return "%s(s%d %dx%dx%d K%d %s)" % (self.name, self.s, self.W, self.H, self.C, self.K, self.kind)


GEOS = {g.name: g for g in (
    Geo("tiny", 3, 15, 3, 1, 9),                  # n = 45: odd, < 64, one workgroup
    Geo("rag2", 3, 18, 9, 3, 9),                  # n = 486 = 2 mod 4: f64 V = 2, f32 V = 1; C = 3
    Geo("tv", 3, 18, 9, 1, 9, tv=2.0 ** -6),      # n = 162, with TV: f64 only (in f32 one ulp of x0 moves its counts)
    Geo("odd3", 3, 15, 9, 3, 9),                  # n = 405 odd, C = 3 (the IRLS cells)
    Geo("idle", 4, 96, 80, 1, 16),                # n = 7680: 30 workgroups, 15 (f64) / 8 (f32) busy; tiles
    Geo("subpix", 2, 70, 50, 1, 4, "subpix"),     # sub-pixel shifts: the SP plan's fold
    Geo("big2", 4, 1020, 540, 1, 4),              # f64 V = 2, 2 rounds (partial); f32 V = 4, 1 round
    Geo("bigodd", 3, 603, 453, 1, 4),             # odd: V = 1 in both, 2 rounds
    Geo("big4", 4, 1028, 1028, 1, 4),             # f32 V = 4, 2 rounds; f64 V = 2, 3 rounds
)}

# Solver runs per geometry: (solver, m, maxits).  m = None: CG.  Every small geometry runs L-BFGS with m = 8 far enough to
# reach live = 8 and with m = 2 far enough (k >= 2 m + 1) for the ring to wrap twice; the large ones run m = 3 past a
# wrap.  Termination by maxits (type 5) unless the run names another type, forced below through eps.
SMALL_RUNS = [("cg", None, 12), ("lbfgs", 8, 12), ("lbfgs", 2, 8)]
LARGE_RUNS = [("cg", None, 6), ("lbfgs", 3, 6)]
TERM_GEO = "rag2"   # the geometry whose runs also end by types 1, 2 and 4
TERMS = (1, 2, 4)


def runs(geo_name):
    g = GEOS[geo_name]
    out = list(LARGE_RUNS if g.n > 100000 else SMALL_RUNS)
    if geo_name == TERM_GEO:
        out += [(sol, m, 40, t) for sol, m in (("cg", None), ("lbfgs", 5)) for t in TERMS]
    return [r if len(r) == 4 else r + (5,) for r in out]


def impls(geo):
    """IMPL_AUTO always; IMPL_DIRECT as well where AUTO folds (elsewhere the two are the same path)."""
    return [IMPL_AUTO, IMPL_DIRECT] if geo.tiles() else [IMPL_AUTO]


def cells():
    """[(geo name, dtype, impl, solver, m, maxits, termination)]: every run on both dtypes and every impl."""
    return [(name, dt, impl) + r for name in GEOS for dt in (F64, F32) for impl in impls(GEOS[name]) for r in runs(name)
            if dt == F64 or GEOS[name].tv == 0]


def cell_id(c):
    name, dt, impl, sol, m, maxits, term = c
    return "%s-%s-%s-%s%s-t%d" % (name, DTYPES[dt][0], "auto" if impl == IMPL_AUTO else "direct", sol,
                                 "" if m is None else str(m), term)


def data(geo):
    """(lr, x0) of a smooth data-term-only problem on geo: random ground truth seen through the model, 1 % noise; x0 the
    nearest-neighbour upsampling of frame 0."""
    import oracle as orc
    rng = np.random.default_rng(7 + geo.n)
    model = orc.ImageModel(scale=geo.s, shifts=geo.shifts(), blur_ksize=geo.blur, blur_sigma=1.0 if geo.blur > 1 else 0.0)
    gt = rng.random((geo.C, geo.H, geo.W))
    lr = np.stack([model.apply(gt, k) for k in range(geo.K)])
    lr = lr + 0.01 * rng.standard_normal(lr.shape)
    x0 = np.stack([orc.resize_nearest(lr[0, c], geo.W, geo.H) for c in range(geo.C)])
    return model, lr, x0


def oracle_problem(geo, model, lr):
    import oracle as orc
    prob = orc.Problem(model, lr)
    if geo.tv > 0:
        prob.add_regularizer(orc.REG_TV, geo.tv)
        prob.set_irls_weights(0, np.ones((geo.C, geo.H, geo.W)))
    return prob


def eps_for(term, probe):
    """(epsg, epsf, epsx) that end a run by `term` at an iteration the probe run (eps 0) passes through, with the
    threshold a geometric mean between the values on either side (a margin of >= 2 %, far above what reduction order
    moves).  probe: per accepted iterate i = 0 .. (start point first) (f_i, |g_i|, |x_i - x_{i-1}|)."""
    f = [p[0] for p in probe]
    gn = [p[1] for p in probe]
    st = [p[2] for p in probe]
    for j in range(2, len(probe)):
        if term == 4:
            lo, hi = gn[j], min(gn[:j])
        elif term == 1:
            r = [(f[i - 1] - f[i]) / max(abs(f[i - 1]), abs(f[i]), 1.0) for i in range(1, j + 1)]
            lo, hi = r[-1], min(r[:-1])
        else:
            lo, hi = st[j], min(st[1:j])
        if lo > 0 and hi > 1.02 * lo:
            e = math.sqrt(lo * hi)
            return {4: (e, 0.0, 0.0), 1: (0.0, e, 0.0), 2: (0.0, 0.0, e)}[term]
    raise AssertionError("no iterate separates termination type %d in the probe" % term)


# ---- bars ------------------------------------------------------------------------------------------------------------
F64_F_BAR, F64_X_BAR = 1e-11, 1e-8


def f_worst(ftrace, f_accepted):
    """Largest distance of an accepted cost from the nearest cost in the other run's evaluation log (relative to
    max(1, |f|))."""
    ft = np.asarray(ftrace, dtype=float)
    return max([float(np.min(np.abs(ft - f) / max(1.0, abs(f)))) for f in f_accepted] or [0.0])


def xerr(a, b):
    a, b = np.asarray(a, dtype=float).ravel(), np.asarray(b, dtype=float).ravel()
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def compare(run, ref):
    """run, ref: (x, (iterations, nfev, termination), evaluation log, accepted costs).  Returns (counts equal, worst
    accepted-cost error, x error)."""
    return run[1] == ref[1], f_worst(run[2], ref[3][1:]), xerr(run[0], ref[0])


def passes(run, ref, f_bar, x_bar):
    same, ef, ex = compare(run, ref)
    return same and ef <= f_bar and ex <= x_bar


def spread_bars(ref, pert, floor):
    """The f32 bars: 10x the reference's own spread (accepted costs, final x) under a perturbation of x0, never below
    `floor`.  None when the perturbation changed the reference's counts (an ill-conditioned cell)."""
    if ref[1] != pert[1]:
        return None
    sf = max([abs(a - b) / max(1.0, abs(b)) for a, b in zip(pert[3][1:], ref[3][1:])] or [0.0])
    sx = xerr(pert[0], ref[0])
    return max(10 * sf, floor), max(10 * sx, floor), sf, sx


def f32_ulp_perturb(x0, seed=5):
    """x0 rounded to f32, every element moved by one f32 ulp in a random direction (a 2^-24 .. 2^-23 relative change
    that survives the f32 upload)."""
    rng = np.random.default_rng(seed)
    a = np.asarray(x0, dtype=np.float32)
    sgn = np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf).astype(np.float32)
    return np.nextafter(a, sgn).astype(np.float64)


F32_FLOOR = 2.0 ** -22
