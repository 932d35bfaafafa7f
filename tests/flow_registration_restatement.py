"""numpy restatement of the dense flow registration (include/srmap.h: srmap_register_flow) -- the checker
of tests/test_flow_registration_cpu.py and tests/test_gpu_flow_registration.py, written from the definition, not from the
kernels.

For every image k >= 1 find a field u_k on image k's grid with I_0(q + u_k(q)) ~= I_k(q): the convention of the
displacement-field motion model (tests/flow_restatement.py), image 0 playing x.  Image 0 gets u = 0.

  pyramid   2 x 2 box means (an odd last row / column dropped), halved while min(w, h) >= 32, at most 12 levels
  start     u = 0 at the coarsest level, or u(q) = F^-1(q) - q of a caller's matrix taken down the pyramid
  transfer  u_fine(q) = 2 * bilinear(u_coarse at (q - 1/2) / 2), coordinates clamped to the coarse image
  pass      s = q + u(q); m = the four bilinear taps of I_0 at s are inside; Tw, Tx, Ty = bilinear samples of I_0 and of its
            central-difference gradient planes (one-sided at the border); e = Tw - I_k; all three 0 where m = 0;
            (a, b, c, p, q) = window sums of (Tx Tx, Tx Ty, Ty Ty, Tx e, Ty e), the window separable and triangular with
            weight 2 r + 1 - |d|, |d| <= 2 r, per axis: along x first, d ascending, then along y, d ascending;
            lambda = damping * (0.5 * (a + c)); a' = a + lambda, c' = c + lambda, det = a' c' - b b;
            du = -((c' p - b q) / det, (a' q - b p) / det) where det > 0, else 0, each component clipped to [-1, 1];
            u <- box mean of u + du over radius smooth_radius, rows then columns ascending, divided by the number of
            in-image pixels of the box
  output    U(Q) = s * bilinear(u at Q / s), clamped; valid = m at the result and q at least valid_margin px from every edge
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_registration_restatement as rg  # noqa: E402
import affine_restatement as ar  # noqa: E402

MAX_LEVELS = 12
MIN_SIZE = 16
DEFAULTS = dict(warps=8, window_radius=4, damping=0.05, smooth_radius=2, valid_margin=3, max_levels=0)


class FlowRegistrationError(ValueError):
    """SRMAP_EINVAL."""


def num_levels(w, h, max_levels=0):
    n = 1
    while min(w, h) >= 32 and n < MAX_LEVELS:
        w, h, n = w // 2, h // 2, n + 1
    return n if max_levels <= 0 else min(n, max_levels)


def gradients(img):
    """(gx, gy): central differences, one-sided at the border."""
    gx, gy = np.empty_like(img), np.empty_like(img)
    gx[:, 1:-1] = 0.5 * (img[:, 2:] - img[:, :-2])
    gx[:, 0], gx[:, -1] = img[:, 1] - img[:, 0], img[:, -1] - img[:, -2]
    gy[1:-1, :] = 0.5 * (img[2:, :] - img[:-2, :])
    gy[0, :], gy[-1, :] = img[1, :] - img[0, :], img[-1, :] - img[-2, :]
    return gx, gy


def grid(h, w):
    return np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")


def inside(u):
    """m [h][w] (bool): the four taps at q + u(q) are inside, and the positions."""
    h, w = u.shape[1:]
    qy, qx = grid(h, w)
    sx, sy = qx + u[0], qy + u[1]
    with np.errstate(invalid="ignore"):
        m = (sx >= 0) & (sx < w - 1) & (sy >= 0) & (sy < h - 1)
    return m, sx, sy


def sample(planes, m, sx, sy):
    """Four-tap bilinear samples of every plane at (sx, sy) where m, 0 elsewhere."""
    sxs, sys_ = np.where(m, sx, 0.0), np.where(m, sy, 0.0)
    x0, y0 = np.floor(sxs).astype(np.int64), np.floor(sys_).astype(np.int64)
    fx, fy = sxs - x0, sys_ - y0
    out = []
    for p in planes:
        v = (1 - fy) * ((1 - fx) * p[y0, x0] + fx * p[y0, x0 + 1]) + fy * ((1 - fx) * p[y0 + 1, x0] + fx * p[y0 + 1, x0 + 1])
        out.append(np.where(m, v, 0.0))
    return out


def _shifted(a, d, axis):
    """a moved so that out[i] = a[i + d] along axis, 0 outside."""
    out = np.zeros_like(a)
    n = a.shape[axis]
    if abs(d) >= n:
        return out
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis] = slice(max(0, d), n + min(0, d))
    dst[axis] = slice(max(0, -d), n - max(0, d))
    out[tuple(dst)] = a[tuple(src)]
    return out


def window_sum(a, r, order="stated"):
    """The separable triangular window sum of one plane.  order = "stated": along x then along y, d ascending; "permuted":
    along y then along x, d descending (the sensitivity probe)."""
    ds = list(range(-2 * r, 2 * r + 1))
    axes = (1, 0)
    if order == "permuted":
        ds, axes = ds[::-1], (0, 1)
    elif order != "stated":
        raise ValueError(order)
    for axis in axes:
        acc = np.zeros_like(a)
        for d in ds:
            acc = acc + float(2 * r + 1 - abs(d)) * _shifted(a, d, axis)
        a = acc
    return a


def box_mean(v, radius, order="stated"):
    """The normalised box mean: rows, then columns ascending; divisor = number of in-image pixels."""
    h, w = v.shape[-2:]
    acc = np.zeros_like(v)
    ds = list(range(-radius, radius + 1))
    if order == "permuted":
        ds = ds[::-1]
    for dy in ds:
        for dx in ds:
            acc = acc + _shifted(_shifted(v, dy, v.ndim - 2), dx, v.ndim - 1)
    ny = np.minimum(np.arange(h) + radius, h - 1) - np.maximum(np.arange(h) - radius, 0) + 1
    nx = np.minimum(np.arange(w) + radius, w - 1) - np.maximum(np.arange(w) - radius, 0) + 1
    return acc / (ny[:, None] * nx[None, :]).astype(np.float64)


def lk_step(i0, ik, u, window_radius=4, damping=0.05, order="stated", grads=None):
    """u + du [2][h][w] of one pass, before the smoothing."""
    gx, gy = gradients(i0) if grads is None else grads
    m, sx, sy = inside(u)
    tw, tx, ty = sample((i0, gx, gy), m, sx, sy)
    e = np.where(m, tw - ik, 0.0)
    a, b, c, p, q = (window_sum(z, window_radius, order) for z in (tx * tx, tx * ty, ty * ty, tx * e, ty * e))
    lam = damping * (0.5 * (a + c))
    a1, c1 = a + lam, c + lam
    det = a1 * c1 - b * b
    ok = det > 0
    safe = np.where(ok, det, 1.0)
    dux = np.where(ok, -((c1 * p - b * q) / safe), 0.0)
    duy = np.where(ok, -((a1 * q - b * p) / safe), 0.0)
    return np.stack([u[0] + np.clip(dux, -1.0, 1.0), u[1] + np.clip(duy, -1.0, 1.0)])


def lk_pass(i0, ik, u, window_radius=4, damping=0.05, smooth_radius=2, order="stated", grads=None):
    """One warp pass at one level: u in -> u out."""
    return box_mean(lk_step(i0, ik, u, window_radius, damping, order, grads), smooth_radius, order)


def resample(u, out_h, out_w, sub, div, gain):
    """gain * bilinear(u at (Q - sub) / div), coordinates clamped to u's image."""
    h, w = u.shape[-2:]
    qy, qx = grid(out_h, out_w)
    cx = np.clip((qx - sub) / div, 0.0, w - 1.0)
    cy = np.clip((qy - sub) / div, 0.0, h - 1.0)
    x0 = np.minimum(np.floor(cx).astype(np.int64), w - 2)
    y0 = np.minimum(np.floor(cy).astype(np.int64), h - 2)
    fx, fy = cx - x0, cy - y0
    return np.stack([gain * ((1 - fy) * ((1 - fx) * p[y0, x0] + fx * p[y0, x0 + 1]) +
                             fy * ((1 - fx) * p[y0 + 1, x0] + fx * p[y0 + 1, x0 + 1])) for p in u])


def to_finer(u, h, w):
    return resample(u, h, w, 0.5, 2.0, 2.0)


def to_output(u, scale):
    h, w = u.shape[-2:]
    return resample(u, scale * h, scale * w, 0.0, float(scale), float(scale))


def affine_start(F, levels, h, w):
    """u(q) = F_l^-1(q) - q at the coarsest level ([h][w] there) for a matrix F of the input level."""
    F = np.array(F, dtype=np.float64).reshape(2, 3)
    if not np.all(np.isfinite(F)) or rg.deviation(F) > rg.MAX_DEVIATION:
        raise FlowRegistrationError("initial matrix is not finite or outside the model's domain")
    for _ in range(levels - 1):
        F = rg.to_coarser(F)
    qy, qx = grid(h, w)
    sx, sy = ar.source_coords(ar.inverse_map(F), qx, qy)
    return np.stack([sx - qx, sy - qy])


def valid_mask(u, margin):
    h, w = u.shape[1:]
    m, _, _ = inside(u)
    qy, qx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return m & (qx >= margin) & (qx <= w - 1 - margin) & (qy >= margin) & (qy <= h - 1 - margin)


def max_neighbour_sum(U):
    """max dx + max dy of one field [2][H][W]: what srmap_problem_set_flow's sufficient condition reads."""
    dx = np.max(np.abs(U[:, :, 1:] - U[:, :, :-1])) if U.shape[2] > 1 else 0.0
    dy = np.max(np.abs(U[:, 1:, :] - U[:, :-1, :])) if U.shape[1] > 1 else 0.0
    return float(dx + dy)


def register_pair(i0, ik, hr_scale=1, init=None, order="stated", **options):
    """(U [2][s h][s w], valid [h][w] of 0 / 1, quality [3], u at the input level)."""
    o = dict(DEFAULTS, **options)
    h, w = i0.shape
    L = num_levels(w, h, o["max_levels"])
    p0, pk = rg.pyramid(i0, L), rg.pyramid(ik, L)
    ch, cw = p0[-1].shape
    u = np.zeros((2, ch, cw)) if init is None else affine_start(init, L, ch, cw)
    for l in range(L - 1, -1, -1):
        g = gradients(p0[l])
        for _ in range(o["warps"]):
            u = lk_pass(p0[l], pk[l], u, o["window_radius"], o["damping"], o["smooth_radius"], order, g)
        if l > 0:
            u = to_finer(u, *p0[l - 1].shape)
    U = to_output(u, hr_scale)
    valid = valid_mask(u, o["valid_margin"])
    m, sx, sy = inside(u)
    e = np.where(valid, sample((i0,), m, sx, sy)[0] - ik, 0.0)
    n = int(np.count_nonzero(valid))
    q = [float(np.sqrt(np.sum(e * e) / n)) if n else 0.0, n / float(w * h), max_neighbour_sum(U)]
    return U, valid.astype(np.float64), q, u


def check_options(hr_scale, o):
    if (hr_scale < 1 or o["warps"] < 1 or not 1 <= o["window_radius"] <= 8 or not o["damping"] >= 0.0 or
            not np.isfinite(o["damping"]) or not 0 <= o["smooth_radius"] <= 8 or o["valid_margin"] < 0 or o["max_levels"] < 0):
        raise FlowRegistrationError("bad options")


def register_flow(images, hr_scale=1, init=None, order="stated", **options):
    """images [n][h][w] -> (flow [n][2][s h][s w], valid [n][h][w], quality [n][3]); image 0: u = 0, valid 1, (0, 1, 0)."""
    images = np.asarray(images, dtype=np.float64)
    n, h, w = images.shape
    check_options(hr_scale, dict(DEFAULTS, **options))
    flow, valid, q = np.zeros((n, 2, hr_scale * h, hr_scale * w)), np.ones((n, h, w)), np.zeros((n, 3))
    if n == 0:
        return flow, valid, q
    if h < MIN_SIZE or w < MIN_SIZE:
        raise FlowRegistrationError("flow registration needs images of at least 16 x 16")
    if not np.all(np.isfinite(images)):
        raise FlowRegistrationError("images are not finite")
    q[0] = [0.0, 1.0, 0.0]
    for k in range(1, n):
        flow[k], valid[k], q[k], _ = register_pair(images[0], images[k], hr_scale,
                                                   None if init is None else np.asarray(init).reshape(n, 2, 3)[k], order, **options)
    return flow, valid, q


def endpoint_error(U, truth, border=8):
    """Mean |U - truth| (Euclidean) over the pixels at least `border` px from every edge."""
    d = np.hypot(U[0] - truth[0], U[1] - truth[1])
    return float(np.mean(d[border:-border, border:-border]))
