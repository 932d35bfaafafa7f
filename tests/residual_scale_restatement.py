"""numpy restatement of the residual scale (include/srmap.h: srmap_residual_scale, srmap_problem_set_huber_scale) -- the
checker of tests/test_residual_scale_cpu.py and tests/test_gpu_residual_scale.py.

  scale          1.4826 * lower median of |r| over the counted observations; 0 when none counts
  lower median   the order statistic of 0-based rank (n - 1) // 2: an element of the input, never an average
  counting rule  L2: effective weight > 0 (all without weights); Huber: prior > 0 (all without a prior)
  MAD delta      max(tuning * scale over ALL frames, min_delta), re-derived at every Huber re-weighting

lower_median is np.partition; radix_lower_median restates the digit passes of csrc/select_host.hpp literally on the bit
patterns; irls_solve_mad is robust_restatement.irls_solve with delta re-derived where the weights are.
"""
import os
import sys

import numpy as np

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import robust_restatement as rr  # noqa: E402

MAD_TO_SIGMA = 1.4826
DIGITS = {np.dtype(np.float32): (11, 10, 10), np.dtype(np.float64): (11, 11, 11, 10, 10, 10)}


def counted(values, mask=None):
    """|values| of the counted elements, flat, in the values' dtype."""
    a = np.abs(np.asarray(values)).ravel()
    return a if mask is None else a[np.asarray(mask).ravel() > 0]


def lower_median(values, mask=None):
    """(lower median of |values| over the counted elements, n); (0, 0) when nothing counts."""
    a = counted(values, mask)
    n = a.size
    if n == 0:
        return a.dtype.type(0), 0
    keys = a.view(np.uint32 if a.dtype == np.float32 else np.uint64)  # NaNs order by their bits, above +inf
    k = (n - 1) // 2
    return np.partition(keys, k)[k:k + 1].view(a.dtype)[0], n


def radix_lower_median(values, mask=None):
    """The same by the digit passes: per pass a histogram of one digit over the elements whose higher digits equal the
    prefix, a scan of its bins, the bin that holds the remaining rank."""
    a = counted(values, mask)
    ut = np.uint32 if a.dtype == np.float32 else np.uint64
    total = a.dtype.itemsize * 8 - 1
    keys = np.ascontiguousarray(a).view(ut) & ut((1 << total) - 1)
    n = keys.size
    if n == 0:
        return a.dtype.type(0), 0
    rank, prefix, shift = (n - 1) // 2, 0, total
    for bits in DIGITS[a.dtype]:
        hb, shift = shift, shift - bits
        match = (keys >> ut(hb)) == ut(prefix >> hb) if hb < total else np.ones(n, bool)
        hist = np.bincount(((keys[match] >> ut(shift)) & ut((1 << bits) - 1)).astype(np.int64), minlength=1 << bits)
        cum = np.cumsum(hist)
        b = int(np.searchsorted(cum, rank, side="right"))
        rank -= int(cum[b] - hist[b])
        prefix |= b << shift
    assert shift == 0 and rank >= 0
    return np.array([prefix], dtype=ut).view(a.dtype)[0], n


def patterns(dtype, n, rng, denormals=True):
    """{name: n values of dtype} that exercise the select: ties, zeros, equal values, infinities, values that differ in
    one digit only.  Signs are mixed: the select sees |v|."""
    dt = np.dtype(dtype)
    ut, total = (np.uint32, 31) if dt == np.float32 else (np.uint64, 63)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(dt)
    base = np.array([0.3], dtype=dt).view(ut)[0]
    low_bits = DIGITS[dt][-1]
    top_shift = total - DIGITS[dt][0]
    mant = DIGITS[dt][0] - (8 if dt == np.float32 else 11)
    out = {
        "random": rng.standard_normal(n).astype(dt),
        "all equal": np.full(n, 0.37, dtype=dt) * sign,
        "eight values, heavy ties": rng.choice(np.array([0.0, 0.01, 0.02, 0.02 + 2.0 ** -20, 0.5, 0.75, 1.0, 3.0], dtype=dt), n) * sign,
        "more than half zeros": np.where(rng.random(n) < 0.6, 0.0, rng.random(n)).astype(dt) * sign,
        "signed zeros": np.zeros(n, dtype=dt) * sign,
        "with +inf": np.where(rng.random(n) < 0.3, np.inf, rng.random(n)).astype(dt),
        "mostly +inf": np.where(rng.random(n) < 0.7, np.inf, rng.random(n)).astype(dt) * sign,
        "lowest digit only": (base + rng.integers(0, 1 << low_bits, n).astype(ut)).view(dt) * sign,
        # the leading digit holds the exponent and m mantissa bits: every normal exponent, nothing else set
        "highest digit only": (rng.integers(1 << mant, ((1 << DIGITS[dt][0]) - 1) >> mant << mant, n).astype(ut) << ut(top_shift)).view(dt) * sign,
    }
    if denormals:
        tiny = np.finfo(dt).tiny
        out["denormals"] = (rng.integers(0, 1000, n) * np.finfo(dt).smallest_subnormal).astype(dt) * sign
        out["denormals and normals"] = np.where(rng.random(n) < 0.5, tiny * rng.random(n) * 0.5, rng.random(n)).astype(dt) * sign
    return out


def residual_scales(r, mask=None, median=lower_median):
    """(scales [1 + K], counts [1 + K]) of residuals r [K][...]: [0] over all frames, [1 + k] of frame k."""
    K = r.shape[0]
    sel = [(r, mask)] + [(r[k], None if mask is None else mask[k]) for k in range(K)]
    out = [median(v, m) for v, m in sel]
    return np.array([MAD_TO_SIGMA * float(m) for m, _ in out]), np.array([float(n) for _, n in out])


def mad_delta(scale, tuning, min_delta):
    d = tuning * scale
    return d if d > min_delta else min_delta


def irls_solve_mad(model, y, x0, reg, tuning=1.345, min_delta=1e-4, per_frame=False, solver="cg", m=5, options=None,
                   use_alglib=None):
    """robust_restatement.irls_solve for a Huber loss whose delta is re-derived, where the weights are, from the scale of
    the iterate's residuals over all frames (per_frame: from each frame's own scale -- the variant the design rejects).
    Returns (x, Report, final weights, [delta per round], per-frame scales [K] of the last round).

    robust_restatement.py may not change, so its loop is restated here and the two must stay in step: the threshold scaling
    (irls_solve's `thr` / `scale` lines), the inner call and the report's sums, the regulariser's re-weighting, the order
    "weights, then diff / prev, then the round count and its cap", and the stopping test of the while.  The only
    difference is the line that forms w: delta comes from residual_scales() of the same residuals."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    shape = np.asarray(x0).shape
    n = int(np.asarray(x0).size)
    ref = orc.Problem(model, y)
    ref.add_regularizer(*reg)
    ref.set_irls_weights(0, np.ones(shape))
    o = orc.default_irls_options() if options is None else options
    thr = [o.gradient_norm_threshold, o.cost_decrease_threshold, o.parameter_variation_threshold,
           o.irls_cost_difference_threshold]
    scale = float(n) * reg[1]
    if not (scale < 1.0):
        thr = [t * scale for t in thr]
    if use_alglib is None:
        use_alglib = orc.have_ref()
    w = np.ones_like(y)

    def fg(v):
        xx = v.reshape(shape)
        f, g = rr.weighted_data_term(model, y, w, xx)
        fr, gr = ref.reg_term(0, xx)
        return f + fr, (g + gr.reshape(shape)).ravel()

    if solver == "lbfgs":
        import lbfgs_restatement as lbr
    x = np.array(x0, dtype=np.float64).ravel().copy()
    rep, deltas, frames = rr.Report(), [], None
    prev, diff = np.inf, thr[3] + 1.0
    while abs(diff) >= thr[3]:
        if solver == "lbfgs":
            x, cr = lbr.minlbfgs(fg, x, m, thr[0], thr[1], thr[2], o.max_num_solver_iterations)
        else:
            x, cr = orc.mincg(fg, x, thr[0], thr[1], thr[2], o.max_num_solver_iterations, use_alglib=use_alglib)
        rep.cg_iterations += cr.iterations
        rep.nfev += cr.nfev
        rep.final_cost = cr.f
        xx = x.reshape(shape)
        ref.set_irls_weights(0, 1.0 / np.maximum(1e-5, orc.reg_values(reg[0], xx, reg[2], reg[3])))
        r = rr.residuals(model, y, xx)
        scales, _ = residual_scales(r)
        frames = scales[1:]
        if per_frame:
            ds = [mad_delta(s, tuning, min_delta) for s in frames]
            w = np.stack([rr.huber_weights(r[k], ds[k]) for k in range(len(ds))])
            deltas.append(float(np.median(ds)))
        else:
            deltas.append(mad_delta(scales[0], tuning, min_delta))
            w = rr.huber_weights(r, deltas[-1])
        diff = prev - cr.f
        prev = cr.f
        rep.irls_rounds += 1
        if o.max_num_irls_iterations > 0 and rep.irls_rounds >= o.max_num_irls_iterations:
            break
    return x.reshape(shape), rep, w, deltas, frames


def seed11_input(sigma):
    """The salt-and-pepper input of robust_restatement.prototype_inputs at another noise level: 3 % salt-and-pepper,
    noise `sigma`, seed 11."""
    P = rr.prototype_inputs()
    clean = np.stack([P["model"].apply(P["gt"], k) for k in range(P["K"])])
    rng = np.random.default_rng(11)
    mask = rng.random(clean.shape) < 0.03
    salt = rng.integers(0, 2, clean.shape).astype(float)
    return np.where(mask, salt, clean + sigma * rng.standard_normal(clean.shape))


def psnr(x, gt):
    return float(10.0 * np.log10(1.0 / np.mean((np.asarray(x) - gt) ** 2)))
