"""Per-element error bars of the parity tests, scaled to the terms each element sums.

A kernel's result g_i is a sum of terms; rounding moves it by at most (a few) unit roundoffs times the sum of the
absolute values of those terms, M_i.  The bar of every comparison here is

    |g_i - g_ref_i| <= C_BAR[dtype] * U[dtype] * M_i      (and the same for the cost, with M_f over all its terms)

so an element that sums small terms gets a small bar: one far BTV tap dropped at one pixel (tests/test_error_bars_cpu.py)
exceeds it, where the relative bar max|g - g_ref| / max(1, |g_ref|) <= 2e-5 of the f32 tests would not.  Near the image
edges the tile path subtracts out-of-image terms again (ring corrections), so there M is widened (with_ring).

M is computed in f64 from the same formulas with every sign taken as +1:
  data term   the oracle's data gradient evaluated at (|x|, -|y|): blur and bilinear warp weights are non-negative, so
              2 s^2 sum_k A_k^T (A_k |x| + |y_k|) bounds every product that enters g_i; its cost bounds the data cost's;
  regulariser the IRLS gradient 2 lambda w r sum alpha^(l+m) sgn(.) (tv_regularizer.cpp / btv_regularizer.cpp, restated
              in tests/test_oracle_crosscheck.py) with sgn -> 1 on every in-image tap and r -> r~, the value with each
              difference |x_p - x_q| replaced by |x_p| + |x_q|; the cost lambda sum w r~^2.

Inputs come from dyadic grids (x = k/64, y = k/256, IRLS weights = k/16, lambda = 2^-6, decay in {0.5, 0.625}): the f32
cast is exact, the oracle sees the numbers the GPU sees, every BTV sign is the same in both precisions, and what is
left between kernel and oracle is rounding alone.
"""
import numpy as np

import oracle as orc
from parity_log import note

F64, F32 = 0, 1
U = {F64: 2.0 ** -53, F32: 2.0 ** -24}

# Bar constants: the worst err / (u * M) over tests/test_gpu_tile_edges.py on an MI355X, times at least 4.
#   gradient  f64: worst measured 3.54 (S = 3, B = 3, BTV 3, E = 0 geometry);  f32: 2.36 (S = 3, B = 3, TV, E = 0)
#   cost      f64: worst measured 12.97 (sub-pixel S = 4, B = 3, TV);          f32: 0.020 (fp64 cost reductions)
C_BAR = {F64: 16.0, F32: 10.0}
C_COST = {F64: 64.0, F32: 1.0}
# The direct regulariser kernels (tests/test_gpu_reg_kernels.py over tests/reg_matrix.py), measured the same way:
#   values    M = value_magnitude.  f64 and f32: worst measured 0 -- with dyadic inputs every term and every partial sum
#             is exact; the constant 1 is a floor, like the f32 cost's above.
#   gradient  M = reg_magnitude.  f64: worst measured 0 (every product and sum exact, also with the f64 weights the
#             GPU wrote); f32: 1.29 (IMPL_AUTO, BTV 3 in the tile kernel + 3-D TV in the march), 0.73 over the direct
#             matrix, 3.38 with GPU-written IRLS weights (BTV 4, decay 1), whose bar adds weights_rel(kind, R).
#   cost      M_f = reg_magnitude's cost.  f64: worst measured 5.15 (GPU-written weights, BTV 3, decay 1, 41 x 260: the
#             fp64 reduction of non-dyadic terms), 0 otherwise; f32: 0.060 (GPU-written weights, BTV 4).
C_REG_VAL = {F64: 1.0, F32: 1.0}
C_REG_GRAD = {F64: 1.0, F32: 6.0}
C_REG_COST = {F64: 24.0, F32: 1.0}

LAMBDA = 2.0 ** -6
DECAYS = (0.5, 0.625)


def dyadic_inputs(rng, K, C, H, W, s):
    """x = k/64 in [0, 1], lr = k/256 in [0, 1], IRLS weights = k/16 in [1/16, 2]: exact in f32."""
    x = rng.integers(0, 65, size=(C, H, W)) / 64.0
    lr = rng.integers(0, 257, size=(K, C, H // s, W // s)) / 256.0
    return x, lr


def dyadic_weights(rng, C, H, W):
    return rng.integers(1, 33, size=(C, H, W)) / 16.0


def _shifted(a, i, j, dc=0):
    """b[p] = a[p + (dc, i, j)] where p + (dc, i, j) lies in the image, else 0 (dc, i, j >= 0)."""
    C, H, W = a.shape
    b = np.zeros_like(a)
    if dc < C and i < H and j < W:
        b[:C - dc, :H - i, :W - j] = a[dc:, i:, j:]
    return b


def _inside(shape, i, j, dc=0):
    C, H, W = shape
    m = np.zeros(shape)
    if dc < C and i < H and j < W:
        m[:C - dc, :H - i, :W - j] = 1.0
    return m


def _add_back(dst, src, i, j, dc=0):
    """dst[p + (dc, i, j)] += src[p] for p + (dc, i, j) in the image."""
    C, H, W = dst.shape
    if dc < C and i < H and j < W:
        dst[dc:, i:, j:] += src[:C - dc, :H - i, :W - j]


def reg_taps(kind, R=0, decay=0.0):
    """(value taps, own gradient taps, neighbour gradient taps) of one regulariser, each [(dc, i, j, weight)].

    A value r_p sums weight * |x_p - x_(p + tap)| over its value taps inside the image.  The gradient at p has its own
    terms 2 c_p r_p * weight * sgn over the own taps, and 2 c_q r_q * weight * sgn of every q = p - tap over the
    neighbour taps.  TV3D has a value tap to the next channel but no own z term (tv_regularizer.cpp:154-170, the
    reference's quirk that k_reg_gradient_direct documents); its previous channel does contribute.  BTV's gradient
    window excludes the row and column R (btv_regularizer.cpp:105-166)."""
    if kind == orc.REG_TV:
        v = [(0, 0, 1, 1.0), (0, 1, 0, 1.0)]
        return v, v, v
    if kind == orc.REG_TV3D:
        v = [(0, 0, 1, 1.0), (0, 1, 0, 1.0)]
        return v + [(1, 0, 0, 1.0)], v, v + [(1, 0, 0, 1.0)]
    if kind == orc.REG_BTV:
        v = [(0, i, j, decay ** (i + j)) for i in range(R + 1) for j in range(R + 1) if (i, j) != (0, 0)]
        g = [(0, i, j, decay ** (i + j)) for i in range(R) for j in range(R) if (i, j) != (0, 0)]
        return v, g, g
    raise ValueError("unknown regulariser kind %r" % kind)


def value_magnitude(kind, x, R=0, decay=0.0):
    """M of every regulariser value: r~_p, the sum of weight * (|x_p| + |x_q|) over the taps inside the image."""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    rt = np.zeros_like(ax)
    for dc, i, j, a in reg_taps(kind, R, decay)[0]:
        rt += a * (ax + _shifted(ax, i, j, dc)) * _inside(ax.shape, i, j, dc)
    return rt


def weights_rel(kind, R=0):
    """Relative error bound of an IRLS weight 1 / max(1e-5, r), in units of u: every value term is non-negative, so the
    sum of `taps` rounded terms is within taps * u of r (the differences of the dyadic inputs are exact), and the
    division adds one more."""
    return len(reg_taps(kind, R, 0.5)[0]) + 1


def reg_magnitude(kind, x, w, lam, R=0, decay=0.0):
    """(M_cost, M_grad) of one IRLS regulariser term (kind 0 TV, 1 TV3D, 2 BTV) at x with weights w."""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    w = np.asarray(w, dtype=np.float64)
    g = np.zeros_like(ax)
    _, own, back = reg_taps(kind, R, decay)
    rt = value_magnitude(kind, ax, R, decay)
    cr = 2.0 * lam * w * rt
    for dc, i, j, a in own:
        g += cr * a * _inside(ax.shape, i, j, dc)   # the element's own differences
    for dc, i, j, a in back:
        _add_back(g, cr * a, i, j, dc)               # its neighbours' differences that contain it
    return float(lam * np.sum(w * rt * rt)), g


def term_magnitude(model, lr, x, regs=()):
    """(M_cost, M_grad [C][H][W]): the sums of |terms| of the objective and of every gradient element.

    regs: iterable of (kind, lam, R, decay, weights)."""
    x = np.asarray(x, dtype=np.float64)
    fd, gd = orc.Problem(model, -np.abs(lr)).data_term(np.abs(x))
    mf, mg = float(fd), gd.reshape(x.shape).copy()
    for kind, lam, R, decay, w in regs:
        f, g = reg_magnitude(kind, x, w, lam, R, decay)
        mf += f
        mg += g
    return mf, mg


def with_ring(M, E, S, hb):
    """The tile path evaluates the border frame (width about 2E) as the interior formula minus the terms that fall outside
    the image (k_border / k_finish_eval ring corrections): there an element's rounding scales with terms that cancel,
    which M does not count.  Within 2E + S + 2 hb of an edge, M is replaced by its maximum over the (2E + S + 2 hb)-
    neighbourhood (E rounded up, plus one for the bilinear taps); the interior keeps its own M.  Without motion and
    blur (E = hb = 0) nothing is corrected and M is returned as it is."""
    from scipy.ndimage import maximum_filter
    M = np.asarray(M, dtype=np.float64)
    if E == 0 and hb == 0:
        return M
    r = 2 * (E + 1) + S + 2 * hb
    C, H, W = M.shape
    near = np.zeros((H, W), dtype=bool)
    near[:r, :] = near[-r:, :] = near[:, :r] = near[:, -r:] = True
    Mx = maximum_filter(M, size=(1, 2 * r + 1, 2 * r + 1), mode="nearest")
    return np.where(near[None], np.maximum(M, Mx), M)


def bar_ratio(a, ref, M):
    """max_i |a_i - ref_i| / (M_i): infinite where an element with M_i = 0 differs at all."""
    a = np.asarray(a, dtype=np.float64).ravel()
    ref = np.asarray(ref, dtype=np.float64).ravel()
    M = np.broadcast_to(np.asarray(M, dtype=np.float64).ravel(), ref.shape)
    err = np.abs(a - ref)
    if np.any((M == 0) & (err != 0)):
        return float("inf")
    nz = M > 0
    return float(np.max(err[nz] / M[nz])) if np.any(nz) else 0.0


def check_gradient(g, g_ref, M, dtype, what="grad"):
    """err / (u * M) of a gradient, logged; the caller asserts it against C_BAR[dtype]."""
    return note(bar_ratio(g, g_ref, M) / U[dtype], "%s err/(u*M) %s" % (what, "f64" if dtype == F64 else "f32"))


def check_cost(f, f_ref, Mf, dtype, what="cost"):
    return note(bar_ratio([f], [f_ref], [Mf]) / U[dtype], "%s err/(u*M) %s" % (what, "f64" if dtype == F64 else "f32"))


def within_bar(g, g_ref, M, dtype, c=None):
    """True where |g - g_ref| <= C_BAR * u * M (c: another constant, C_COST for costs), per element."""
    c = C_BAR[dtype] if c is None else c
    return np.abs(np.asarray(g) - np.asarray(g_ref)) <= c * U[dtype] * np.asarray(M)
