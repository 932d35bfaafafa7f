"""A numpy restatement of the regularisers' values and of BOTH gradient modes (include/srmap.h,
srmap_problem_set_regularizer_gradient), written from the formulas and from nothing of the library:

  values    BTV   r[p] = sum_{i,j in [0,R], p+(i,j) inside} a^(i+j) |x[p] - x[p+(i,j)]|
            TV    r[p] = |x[p+(1,0)] - x[p]| + |x[p+(0,1)] - x[p]|          (what lies outside contributes 0)
            TV3D  the same + |x[c+1][p] - x[c][p]| where the next channel exists
  cost      sum_p c[p] r[p]^2,  c = lambda w  (held fixed: the IRLS weights are constants of the gradient)
  gradient  REFERENCE  the reference's, bug for bug: BTV differentiates the window [0, R-1] and never takes the absolute
                       pixel (0, 0) as a source for its neighbours; TV3D has no -sgn dz in the self term
            EXACT      the gradient of the cost above:
                       BTV   g[p] += 2 c[p] r[p] sum_{i,j in [0,R]} a^(i+j) sgn(x[p] - x[p+(i,j)])
                                   - sum_{(i,j) != (0,0), q = p-(i,j) inside} 2 c[q] r[q] a^(i+j) sgn(x[q] - x[p])
                       TV3D  self term -sgn dx - sgn dy - sgn dz
                       TV    the reference's (it is the true one)
Arrays are [C][H][W] float64; sgn(0) = 0."""
import numpy as np

TV, TV3D, BTV = 0, 1, 2
REFERENCE, EXACT = 0, 1


def values(kind, x, R=0, decay=0.0):
    x = np.asarray(x, dtype=np.float64)
    C, H, W = x.shape
    r = np.zeros_like(x)
    if kind == BTV:
        for i in range(R + 1):
            for j in range(R + 1):
                if i >= H or j >= W:
                    continue
                r[:, :H - i, :W - j] += decay ** (i + j) * np.abs(x[:, :H - i, :W - j] - x[:, i:, j:])
        return r
    r[:, :H - 1, :] += np.abs(x[:, 1:, :] - x[:, :-1, :])
    r[:, :, :W - 1] += np.abs(x[:, :, 1:] - x[:, :, :-1])
    if kind == TV3D:
        r[:C - 1] += np.abs(x[1:] - x[:-1])
    return r


def cost(kind, x, c, R=0, decay=0.0):
    """sum c r^2 (c: lambda * IRLS weights, [C][H][W])"""
    r = values(kind, x, R, decay)
    return float(np.sum(np.asarray(c, dtype=np.float64) * r * r))


def gradient(kind, x, c, mode, R=0, decay=0.0):
    """(values, gradient) with the constants c[q] held fixed"""
    x = np.asarray(x, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    C, H, W = x.shape
    r = values(kind, x, R, decay)
    m = 2.0 * c * r
    g = np.zeros_like(x)
    if kind == BTV:
        E = R + 1 if mode == EXACT else R  # the window differentiated: [0, E)
        for i in range(E):
            for j in range(E):
                if i >= H or j >= W:
                    continue
                # q = [:H-i, :W-j] and its tap q + (i, j)
                s = decay ** (i + j) * np.sign(x[:, :H - i, :W - j] - x[:, i:, j:])
                g[:, :H - i, :W - j] += m[:, :H - i, :W - j] * s  # q's own term
                if i == 0 and j == 0:
                    continue  # sgn(0) = 0 in both modes
                src = m[:, :H - i, :W - j].copy()
                if mode == REFERENCE:
                    src[:, 0, 0] = 0.0  # the absolute pixel (0, 0) is never a source
                g[:, i:, j:] -= src * s  # q as a source of p = q + (i, j)
        return r, g
    dx = np.sign(x[:, :, 1:] - x[:, :, :-1])  # sgn(x[q + (0,1)] - x[q])
    dy = np.sign(x[:, 1:, :] - x[:, :-1, :])
    g[:, :, :W - 1] -= m[:, :, :W - 1] * dx   # self terms
    g[:, :H - 1, :] -= m[:, :H - 1, :] * dy
    g[:, :, 1:] += m[:, :, :W - 1] * dx       # the left / upper neighbour as a source
    g[:, 1:, :] += m[:, :H - 1, :] * dy
    if kind == TV3D:
        dz = np.sign(x[1:] - x[:-1])
        g[1:] += m[:C - 1] * dz               # the previous channel as a source
        if mode == EXACT:
            g[:C - 1] -= m[:C - 1] * dz       # the self term the reference leaves out
    return r, g


def magnitude(kind, x, c, mode, R=0, decay=0.0):
    """(M_cost, M_grad) in the sense of tests/error_bars.py: the cost and the gradient of `mode` with every sign taken as +1
    and every |x_p - x_q| as |x_p| + |x_q| -- the sum of the absolute values of the terms an element sums."""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    c = np.asarray(c, dtype=np.float64)
    C, H, W = ax.shape
    if kind == BTV:
        E = R + 1 if mode == EXACT else R
        vt = [(0, i, j, decay ** (i + j)) for i in range(R + 1) for j in range(R + 1) if (i, j) != (0, 0)]
        gt = [(0, i, j, decay ** (i + j)) for i in range(E) for j in range(E) if (i, j) != (0, 0)]
        own = back = gt
    else:
        vt = [(0, 1, 0, 1.0), (0, 0, 1, 1.0)] + ([(1, 0, 0, 1.0)] if kind == TV3D else [])
        own = vt if (mode == EXACT or kind == TV) else vt[:2]
        back = vt
    rt = np.zeros_like(ax)
    for dc, i, j, a in vt:
        if dc < C and i < H and j < W:
            rt[:C - dc, :H - i, :W - j] += a * (ax[:C - dc, :H - i, :W - j] + ax[dc:, i:, j:])
    m = 2.0 * c * rt
    g = np.zeros_like(ax)
    for dc, i, j, a in own:
        if dc < C and i < H and j < W:
            g[:C - dc, :H - i, :W - j] += m[:C - dc, :H - i, :W - j] * a
    for dc, i, j, a in back:
        if dc < C and i < H and j < W:
            g[dc:, i:, j:] += m[:C - dc, :H - i, :W - j] * a
    return float(np.sum(c * rt * rt)), g


def min_tap_difference(kind, x, R=0):
    """the smallest |x[p] - x[tap]| over every non-self tap of every value: no sign flips within less than this"""
    x = np.asarray(x, dtype=np.float64)
    C, H, W = x.shape
    best = np.inf
    taps = [(i, j) for i in range(R + 1) for j in range(R + 1) if (i, j) != (0, 0)] if kind == BTV else [(1, 0), (0, 1)]
    for i, j in taps:
        if i < H and j < W:
            d = np.abs(x[:, :H - i, :W - j] - x[:, i:, j:])
            if d.size:
                best = min(best, float(d.min()))
    if kind == TV3D and C > 1:
        best = min(best, float(np.abs(x[1:] - x[:-1]).min()))
    return best


def separated_point(rng, shape):
    """a random image whose entries are pairwise at least 0.75 / n apart (n = its size): a shuffled ramp with jitter"""
    n = int(np.prod(shape))
    return ((rng.permutation(n) + 0.25 * rng.random(n)) / n).reshape(shape)


def central_differences(kind, x, c, R=0, decay=0.0, eps=1e-6):
    x = np.array(x, dtype=np.float64)  # a contiguous copy: entries are moved in place below
    g = np.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for k in range(flat.size):
        keep = flat[k]
        flat[k] = keep + eps
        fp = cost(kind, x, c, R, decay)
        flat[k] = keep - eps
        fm = cost(kind, x, c, R, decay)
        flat[k] = keep
        gf[k] = (fp - fm) / (2.0 * eps)
    return g


def corner_image(shape, base=0.5, corner=0.9):
    """only x[0][0][0] differs from a constant"""
    x = np.full(shape, base)
    x[0, 0, 0] = corner
    return x


# ---- the solve with either gradient (the table of tests/golden/reg_exact_table.json) ----
class Report:
    def __init__(self):
        self.irls_rounds = self.cg_iterations = self.nfev = 0
        self.final_cost = 0.0


def irls_solve(model, y, x0, reg, mode, options=None, use_alglib=None, solver="cg", m=5):
    """IRLSMapSolver::Solve (irls_map_solver.cpp:192-265, thresholds scaled as map_solver.cpp:16-26 /
    irls_map_solver.cpp:161-171; one channel block) with the regulariser's gradient in `mode`: the oracle's data term, this
    file's regulariser, the oracle's mincg (use_alglib: the reference's ALGLIB; None = when it is built) or
    tests/lbfgs_restatement.py's minlbfgs.  reg = (kind, lambda, range, decay).  Returns (x, Report)."""
    import oracle as orc
    kind, lam, R, decay = reg
    y = np.ascontiguousarray(y, dtype=np.float64)
    shape = np.asarray(x0).shape
    n = int(np.asarray(x0).size)
    ref = orc.Problem(model, y)
    o = orc.default_irls_options() if options is None else options
    thr = [o.gradient_norm_threshold, o.cost_decrease_threshold, o.parameter_variation_threshold,
           o.irls_cost_difference_threshold]
    scale = float(n) * lam
    if not (scale < 1.0):
        thr = [t * scale for t in thr]
    if use_alglib is None:
        use_alglib = orc.have_ref()
    w = np.ones(shape)

    def fg(v):
        xx = v.reshape(shape)
        f, g = ref.data_term(xx)
        c = lam * w
        r, gr = gradient(kind, xx, c, mode, R, decay)
        return f + float(np.sum(c * r * r)), (g.reshape(shape) + gr).ravel()

    x = np.array(x0, dtype=np.float64).ravel().copy()
    rep = Report()
    prev, diff = np.inf, thr[3] + 1.0
    while abs(diff) >= thr[3]:
        if solver == "lbfgs":
            import lbfgs_restatement as lbr
            x, cr = lbr.minlbfgs(fg, x, m, thr[0], thr[1], thr[2], o.max_num_solver_iterations)
        else:
            x, cr = orc.mincg(fg, x, thr[0], thr[1], thr[2], o.max_num_solver_iterations, use_alglib=use_alglib)
        rep.cg_iterations += cr.iterations
        rep.nfev += cr.nfev
        rep.final_cost = cr.f
        w = 1.0 / np.maximum(1e-5, values(kind, x.reshape(shape), R, decay))
        diff = prev - cr.f
        prev = cr.f
        rep.irls_rounds += 1
        if o.max_num_irls_iterations > 0 and rep.irls_rounds >= o.max_num_irls_iterations:
            break
    return x.reshape(shape), rep


TABLE_ROWS = [(R, lam) for lam in (0.005, 0.02) for R in (1, 2, 3)]
TABLE_DECAY = 0.5


def table_inputs():
    """the robust table's noise input (tests/robust_restatement.py: 96 x 128, scale 2, 6 frames, sigma 0.01) and the
    README tables' start, the bilinear upsample of frame 0"""
    import robust_restatement as rr
    P = rr.prototype_inputs()
    y = [yy for name, yy, _ in P["inputs"] if name == "noise"][0]
    return dict(model=P["model"], y=y, x0=rr.bilinear(y[0], P["s"]), gt=P["gt"], s=P["s"], shifts=P["shifts"])


def table_solve(inp, R, lam, mode, y=None, solver="cg"):
    """(PSNR dB, [IRLS rounds, iterations, evaluations]) of one solve of the table"""
    import oracle as orc
    x, rep = irls_solve(inp["model"], inp["y"] if y is None else y, inp["x0"], (BTV, lam, R, TABLE_DECAY), mode, solver=solver)
    return float(orc.psnr(inp["gt"], x)), [rep.irls_rounds, rep.cg_iterations, rep.nfev]
