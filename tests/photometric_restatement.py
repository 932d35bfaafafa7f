"""numpy restatement of the photometric frame model and of its fit (include/srmap.h: srmap_problem_set_photometric,
srmap_fit_photometric), built from the CPU oracle's Python API and written from the definitions -- the
checker of tests/test_photometric_cpu.py and tests/test_gpu_photometric.py.

  model      y_k = a_k (D B M_k x) + b_k + noise; the problem solves against yn_k = (y_k - b_k) / a_k
  normalise  per element, in double on the stored value: the subtraction, a true division, one rounding to the dtype
  sums       per frame S = {sum w, sum w s, sum w y, sum w s^2, sum w s y, sum w y^2}, s = (A_k x)(c, u) from any model with
             an .apply (orc.ImageModel, affine_restatement / blur_kernel_restatement models), y the RAW frame
  solve      model 0: the 2 x 2 normal equations of E(a, b) = sum w (a s + b - y)^2; model 1: a alone, b held; model 2: b
             alone, a held; statuses 0 fitted / 2 gain outside the bounds / 3 degenerate (sum w = 0, or a determinant
             <= 1e-12 sum w sum w s^2); the gauge frame keeps its parameters
  loop       fit at x0, solve, then rounds x (fit at x, warm solve) around robust_restatement.irls_solve
"""
import os
import sys

import numpy as np

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_restatement as rr  # noqa: E402

SUMS = 6
GAIN_BIAS, GAIN_ONLY, BIAS_ONLY = 0, 1, 2
STATUS_OK, STATUS_GAIN_BOUNDS, STATUS_DEGENERATE = 0, 2, 3
DET_RTOL = 1e-12

TABLE_GAINS = (1.0, 1.08, 0.94, 1.05, 0.90, 1.03)
TABLE_BIASES = (0.0, 0.03, -0.02, 0.01, 0.04, -0.03)


def normalise(y, gain_bias, dtype=np.float64):
    """yn[k] = (y[k] - bias_k) / gain_k on the values as the problem stores them (rounded to dtype first), rounded once."""
    y = np.asarray(y, dtype=np.float64).astype(dtype).astype(np.float64)
    gb = np.asarray(gain_bias, dtype=np.float64).reshape(-1, 2)
    shape = (-1,) + (1,) * (y.ndim - 1)
    return ((y - gb[:, 1].reshape(shape)) / gb[:, 0].reshape(shape)).astype(dtype)


def apply_photometric(clean, gain_bias):
    """a_k * clean[k] + b_k."""
    gb = np.asarray(gain_bias, dtype=np.float64).reshape(-1, 2)
    shape = (-1,) + (1,) * (np.ndim(clean) - 1)
    return gb[:, 0].reshape(shape) * np.asarray(clean, dtype=np.float64) + gb[:, 1].reshape(shape)


def predictions(model, x, K):
    """s[k] = A_k x, [K][C][h][w]."""
    return np.stack([model.apply(x, k) for k in range(K)])


def frame_sums(s, y, w=None, order="natural"):
    """The six sums of one frame; s, y, w [C][h][w] (w None = ones).  order: the order the observations enter the sums in
    ("natural", "reversed", "transposed": the sensitivity probe)."""
    s, y = np.asarray(s, dtype=np.float64), np.asarray(y, dtype=np.float64)
    w = np.ones_like(y) if w is None else np.asarray(w, dtype=np.float64)
    if order == "transposed":
        s, y, w = (np.ascontiguousarray(np.swapaxes(v, -1, -2)) for v in (s, y, w))
    s, y, w = s.ravel(), y.ravel(), w.ravel()
    if order == "reversed":
        s, y, w = s[::-1], y[::-1], w[::-1]
    return np.array([np.sum(w), np.sum(w * s), np.sum(w * y), np.sum(w * s * s), np.sum(w * s * y), np.sum(w * y * y)])


def sums(model, x, y, w=None, order="natural"):
    """[K][6] for the raw frames y [K][C][h][w]."""
    K = y.shape[0]
    return np.stack([frame_sums(model.apply(x, k), y[k], None if w is None else w[k], order) for k in range(K)])


def energy(S, a, b):
    """E(a, b) = sum w (a s + b - y)^2 from the six sums."""
    return a * a * S[3] + 2 * a * b * S[1] + b * b * S[0] - 2 * (a * S[4] + b * S[2]) + S[5]


def solve_frame(S, model=GAIN_BIAS, current=(1.0, 0.0), min_gain=0.25, max_gain=4.0):
    """(gain, bias, E at `current`, E at the result, status) of one frame."""
    a0, b0 = float(current[0]), float(current[1])
    e0 = energy(S, a0, b0)
    keep = (a0, b0, e0, e0)
    sw, ss, sy, sss, ssy = S[:5]
    if not sw > 0.0:
        return keep + (STATUS_DEGENERATE,)
    a, b = a0, b0
    if model == GAIN_BIAS:
        det = sw * sss - ss * ss
        if not det > DET_RTOL * sw * sss:
            return keep + (STATUS_DEGENERATE,)
        a, b = np.linalg.solve(np.array([[sss, ss], [ss, sw]]), np.array([ssy, sy]))
    elif model == GAIN_ONLY:
        if not sss > 0.0:
            return keep + (STATUS_DEGENERATE,)
        a = (ssy - b0 * ss) / sss
    else:
        b = (sy - a0 * ss) / sw
    if not (np.isfinite(a) and np.isfinite(b)):
        return keep + (STATUS_DEGENERATE,)
    if not (min_gain <= a <= max_gain):
        return keep + (STATUS_GAIN_BOUNDS,)
    return float(a), float(b), e0, energy(S, a, b), STATUS_OK


def fit(model, x, y, w=None, current=None, kind=GAIN_BIAS, gauge_frame=0, min_gain=0.25, max_gain=4.0, order="natural"):
    """(gain_bias [K][2], quality [K][4] = E at the parameters in force, E at the result, sum w, status, sums [K][6]) from
    the RAW frames y; current: the parameters in force (None = ones and zeros)."""
    K = y.shape[0]
    cur = np.tile([1.0, 0.0], (K, 1)) if current is None else np.asarray(current, dtype=np.float64).reshape(K, 2)
    S = sums(model, x, y, w, order)
    gb, q = np.zeros((K, 2)), np.zeros((K, 4))
    for k in range(K):
        a, b, e0, e1, st = solve_frame(S[k], kind, cur[k], min_gain, max_gain)
        if k == gauge_frame:
            a, b, e1, st = cur[k, 0], cur[k, 1], e0, STATUS_OK
        gb[k] = (a, b)
        q[k] = (e0, e1, S[k, 0], st)
    return gb, q, S


def solve_photometric(model, y, x0, reg=None, rounds=3, options=None, use_alglib=None, **fit_kw):
    """Problem.solve_photometric: fit at x0, a solve from x0, then `rounds` x (fit at x, warm solve).  Returns (x, [Report
    per solve], [(gain_bias, quality) per fit])."""
    y = np.asarray(y, dtype=np.float64)
    gb, q, _ = fit(model, x0, y, **fit_kw)
    fits = [(gb, q)]
    x, rep, _ = rr.irls_solve(model, normalise(y, gb), x0, reg=reg, options=options, use_alglib=use_alglib)
    reports = [rep]
    for _ in range(rounds):
        gb, q, _ = fit(model, x, y, current=gb, **fit_kw)
        fits.append((gb, q))
        x, rep, _ = rr.irls_solve(model, normalise(y, gb), x, reg=reg, options=options, use_alglib=use_alglib)
        reports.append(rep)
    return x, reports, fits


def table_inputs():
    """The robust table's input (96 x 128 HR, scale 2, 6 frames, blur 3 / sigma 1, BTV(2, 0.5) lambda 0.005, noise sigma
    0.01, seed 7) with the frames generated under TABLE_GAINS / TABLE_BIASES: y_k = a_k (A_k gt) + b_k + noise."""
    P = rr.prototype_inputs()
    gt, model, K = P["gt"], P["model"], P["K"]
    clean = predictions(model, gt, K)
    truth = np.stack([TABLE_GAINS, TABLE_BIASES], axis=1)
    noise = 0.01 * np.random.default_rng(7).standard_normal(clean.shape)
    out = dict(P)
    out.update(clean=clean, truth=truth, y=apply_photometric(clean, truth) + noise)
    del out["inputs"]
    return out
