"""numpy restatement of the persistent prior on the data weights (include/srmap.h: srmap_set_data_prior) -- the checker of
tests/test_data_prior_cpu.py and tests/test_gpu_data_prior.py.

  effective weights   w_eff = m .* w
  under L2            w = the caller's weights, or ones: robust_restatement.irls_solve(weights=m * w) as it stands
  under HUBER         the reset at the start of a solve gives w_eff = m; every re-weighting gives m .* huber(r) from the
                      UNWEIGHTED residual r = A x - y

irls_solve below is robust_restatement.irls_solve's loop (IRLSMapSolver::Solve, one channel block) with that one change.
"""
import os
import sys

import numpy as np

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_restatement as rr  # noqa: E402


def effective_weights(m, w=None):
    """m .* w in double (w None = ones)."""
    m = np.asarray(m, dtype=np.float64)
    return m.copy() if w is None else m * np.asarray(w, dtype=np.float64)


def huber_prior_weights(m, r, delta):
    """m .* huber(r): the re-weighting step of a problem with a prior."""
    return np.asarray(m, dtype=np.float64) * rr.huber_weights(r, delta)


def irls_solve(model, y, x0, m, reg=None, delta=None, options=None, use_alglib=None):
    """The Huber IRLS solve with the prior m ([K][C][h][w], or anything that broadcasts to y): weights start at m and are
    m .* huber(A x - y) after every inner run.  Returns (x, robust_restatement.Report, final effective weights)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    m = np.ascontiguousarray(np.broadcast_to(np.asarray(m, dtype=np.float64), y.shape))
    shape = np.asarray(x0).shape
    n = int(np.asarray(x0).size)
    assert delta is not None and delta > 0
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
    if use_alglib is None:
        use_alglib = orc.have_ref()
    state = {"w": m.copy()}

    def fg(v):
        xx = v.reshape(shape)
        f, g = rr.weighted_data_term(model, y, state["w"], xx)
        if reg is not None:
            fr, gr = ref.reg_term(0, xx)
            f, g = f + fr, g + gr.reshape(shape)
        return f, g.ravel()

    x = np.array(x0, dtype=np.float64).ravel().copy()
    rep = rr.Report()
    prev, diff = np.inf, thr[3] + 1.0
    while abs(diff) >= thr[3]:
        x, cr = orc.mincg(fg, x, thr[0], thr[1], thr[2], o.max_num_solver_iterations, use_alglib=use_alglib)
        rep.cg_iterations += cr.iterations
        rep.nfev += cr.nfev
        rep.final_cost = cr.f
        xx = x.reshape(shape)
        if reg is not None:
            vals = orc.reg_values(reg[0], xx, reg[2], reg[3])
            ref.set_irls_weights(0, 1.0 / np.maximum(1e-5, vals))
        state["w"] = huber_prior_weights(m, rr.residuals(model, y, xx), delta)
        diff = prev - cr.f
        prev = cr.f
        rep.irls_rounds += 1
        if o.max_num_irls_iterations > 0 and rep.irls_rounds >= o.max_num_irls_iterations:
            break
    return x.reshape(shape), rep, state["w"]


def plane_of(y, channel):
    """The plane srmap_problem_register_flow registers: y [K][C][h][w] -> [K][h][w]; channel >= 0 that channel, -1 the
    mean over the channels -- the sum in ascending channel order from 0.0, one division by C."""
    y = np.asarray(y, dtype=np.float64)
    if channel >= 0:
        return y[:, channel].copy()
    acc = np.zeros(y[:, 0].shape)
    for c in range(y.shape[1]):
        acc = acc + y[:, c]
    return acc / float(y.shape[1])


def problem_register_flow(y, channel, scale, hr_scale=1, dtype=np.float64, **options):
    """srmap_problem_register_flow on observations y [K][C][h][w] as the problem stores them: the plane by plane_of, the
    registration of flow_registration_restatement at the PROBLEM's scale (hr_scale must be 1 or that scale), the field
    rounded once to the problem's dtype.  Returns (field [K][2][s h][s w] as doubles, prior [K][C][h][w], quality [K][3]);
    the quality is that of the double field."""
    import flow_registration_restatement as fq
    y = np.asarray(y, dtype=np.float64)
    if y.ndim != 4 or y.shape[0] == 0:
        raise fq.FlowRegistrationError("no observations")
    if not (-1 <= channel < y.shape[1]):
        raise fq.FlowRegistrationError("channel %d of %d" % (channel, y.shape[1]))
    if hr_scale not in (1, scale):
        raise fq.FlowRegistrationError("hr_scale %d is neither 1 nor the problem's scale %d" % (hr_scale, scale))
    flow, valid, q = fq.register_flow(plane_of(y, channel), hr_scale=scale, **options)
    prior = np.ascontiguousarray(np.broadcast_to(valid[:, None], y.shape))
    return flow.astype(dtype).astype(np.float64), prior, q
