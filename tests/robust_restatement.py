"""numpy restatement of the robust data term (include/srmap.h: srmap_set_data_weights, srmap_problem_set_data_loss), built
from the CPU oracle's Python API only -- the checker of tests/test_robust_cpu.py and tests/test_gpu_robust.py.

  data cost     s^2 sum_k sum_i w[k][i] r[k][i]^2,   r[k] = A_k x - y_k
  gradient      2 s^2 sum_k A_k^T (w[k] .* r[k])
  Huber weight  w = 1 where |r| <= delta, delta / |r| elsewhere

composed from ImageModel.apply / apply_transpose (image_model.cpp:86-101), and the IRLS loop of
irls_map_solver.cpp:192-265 (thresholds scaled as map_solver.cpp:16-26 / irls_map_solver.cpp:161-171) around the oracle's
mincg -- or tests/lbfgs_restatement.py's minlbfgs -- with the data weights re-derived where the regulariser's are.
"""
import os
import sys

import numpy as np

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def residuals(model, y, x):
    """r[k] = A_k x - y_k, [K][C][h][w]."""
    return np.stack([model.apply(x, k) - y[k] for k in range(y.shape[0])])


def weighted_data_term(model, y, w, x, want_grad=True, cost_rows=None):
    """(cost, gradient) of the weighted data term; w None = all ones.  cost_rows = (hr_row0, hr_row1): only the
    residuals of LR rows [hr_row0 / s, hr_row1 / s) count in the COST (srmap_problem_set_cost_rows); the gradient is
    always whole."""
    s = model.scale
    f, g = 0.0, (np.zeros_like(np.asarray(x, dtype=np.float64)) if want_grad else None)
    for k in range(y.shape[0]):
        r = model.apply(x, k) - y[k]
        wr = r if w is None else w[k] * r
        if cost_rows is None:
            f += s * s * np.sum(wr * r)
        else:
            i0, i1 = cost_rows[0] // s, -(-cost_rows[1] // s)
            f += s * s * np.sum((wr * r)[:, i0:i1])
        if want_grad:
            g += 2 * s * s * model.apply_transpose(wr, k)
    return f, g


def huber_weights(r, delta):
    """w = 1 where |r| <= delta, delta / |r| elsewhere."""
    a = np.abs(r)
    return np.where(a <= delta, 1.0, delta / np.where(a > 0, a, 1.0))


class Report:
    def __init__(self):
        self.irls_rounds = 0
        self.cg_iterations = 0
        self.nfev = 0
        self.final_cost = 0.0


def irls_solve(model, y, x0, reg=None, loss="l2", delta=None, weights=None, solver="cg", m=5, options=None,
               use_alglib=None, composed=None):
    """IRLSMapSolver::Solve (one channel block, no split_channels) with a weighted / Huber data term.

    reg: (kind, lambda, btv_range, btv_decay) or None.  loss "l2": the weights (None = ones) stay as given; "huber": they
    start at 1 and are re-derived from the iterate after every inner run.  solver "cg" (oracle.mincg; use_alglib: the
    reference's ALGLIB when oracle/_ref is built) or "lbfgs" (lbfgs_restatement.minlbfgs with m pairs).  composed: take
    the data term from weighted_data_term even when all weights are 1 (default: only when there are weights; without
    them the objective is oracle.Problem.objective itself).  Returns (x, Report, final weights or None)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    shape = np.asarray(x0).shape
    n = int(np.asarray(x0).size)
    ref = orc.Problem(model, y)
    lam = 0.0
    if reg is not None:
        ref.add_regularizer(*reg)
        ref.set_irls_weights(0, np.ones(shape))
        lam = reg[1]
    o = orc.default_irls_options() if options is None else options
    thr = [o.gradient_norm_threshold, o.cost_decrease_threshold, o.parameter_variation_threshold,
           o.irls_cost_difference_threshold]
    scale = float(int(n)) * lam
    if not (scale < 1.0):
        thr = [t * scale for t in thr]
    huber = loss == "huber"
    assert loss in ("l2", "huber") and (not huber or (delta is not None and delta > 0))
    w = np.ones_like(y) if huber else (None if weights is None else np.asarray(weights, dtype=np.float64))
    if composed is None:
        composed = w is not None
    if composed and w is None:
        w = np.ones_like(y)
    if use_alglib is None:
        use_alglib = orc.have_ref()

    def fg(v):
        xx = v.reshape(shape)
        if not composed:
            f, g = ref.objective(xx)
            return f, g.ravel()
        f, g = weighted_data_term(model, y, w, xx)
        if reg is not None:
            fr, gr = ref.reg_term(0, xx)
            f, g = f + fr, g + gr.reshape(shape)
        return f, g.ravel()

    if solver == "lbfgs":
        import lbfgs_restatement as lbr
    x = np.array(x0, dtype=np.float64).ravel().copy()
    rep = Report()
    prev, diff = np.inf, thr[3] + 1.0
    while abs(diff) >= thr[3]:
        if solver == "lbfgs":
            x, cr = lbr.minlbfgs(fg, x, m, thr[0], thr[1], thr[2], o.max_num_solver_iterations)
        else:
            x, cr = orc.mincg(fg, x, thr[0], thr[1], thr[2], o.max_num_solver_iterations, use_alglib=use_alglib)
        rep.cg_iterations += cr.iterations
        rep.nfev += cr.nfev
        rep.final_cost = cr.f
        if reg is None and not huber:
            rep.irls_rounds += 1
            break
        xx = x.reshape(shape)
        if reg is not None:
            vals = orc.reg_values(reg[0], xx, reg[2], reg[3])
            ref.set_irls_weights(0, 1.0 / np.maximum(1e-5, vals))
        if huber:
            w = huber_weights(residuals(model, y, xx), delta)
        diff = prev - cr.f
        prev = cr.f
        rep.irls_rounds += 1
        if o.max_num_irls_iterations > 0 and rep.irls_rounds >= o.max_num_irls_iterations:
            break
    return x.reshape(shape), rep, w


# ---- the three inputs of the robust data term's figures (README, profiles/r08_robust.txt) ----
def prototype_ground_truth(C, H, W):
    v, u = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = 0.5 + 0.25 * np.sin(2 * np.pi * 2 * u) * np.cos(2 * np.pi * 3 * v) + 0.2 * ((u - .5) ** 2 + (v - .5) ** 2 < .08)
    return np.stack([np.clip(base * (0.7 + 0.3 * c / max(1, C - 1)), 0, 1) for c in range(C)])


def bilinear(im, s):
    import bench
    return np.stack([bench.bilinear_upsample(im[c:c + 1], s)[0] for c in range(im.shape[0])])


def prototype_inputs():
    """96 x 128 HR, scale 2, 6 frames, blur 3 / sigma 1, noise sigma 0.01 (seed 7): noise only; 3 % salt-and-pepper in
    the LR frames; frame 4 generated with shift (3, -2) instead of (1, 1).  Returns a dict with the geometry, the ground
    truth, the model, and inputs = [(name, y, corrupted mask or None)]."""
    C, H, W, s, K = 1, 96, 128, 2, 6
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0], [1, 1], [0, 1]]
    gt = prototype_ground_truth(C, H, W)
    model = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=3, blur_sigma=1.0)
    clean = np.stack([model.apply(gt, k) for k in range(K)])
    rng = np.random.default_rng(7)
    y_noise = clean + 0.01 * rng.standard_normal(clean.shape)
    mask = rng.random(clean.shape) < 0.03
    y_sp = np.where(mask, rng.integers(0, 2, clean.shape).astype(float), clean + 0.01 * rng.standard_normal(clean.shape))
    wrong = orc.ImageModel(scale=s, shifts=[[3, -2]] * K, blur_ksize=3, blur_sigma=1.0).apply(gt, 0)
    y_mis = np.stack([clean[k] if k != 4 else wrong for k in range(K)]) + 0.01 * rng.standard_normal(clean.shape)
    return dict(C=C, H=H, W=W, s=s, K=K, shifts=shifts, blur=(3, 1.0), gt=gt, model=model,
                reg=(orc.REG_BTV, 0.005, 2, 0.5), delta=0.02,
                inputs=[("noise", y_noise, None), ("salt_pepper", y_sp, mask), ("misregistered", y_mis, None)])
