"""numpy restatement of the affine per-frame motion model (include/srmap.h: srmap_problem_set_affine_motion) -- the
checker of tests/test_affine_cpu.py and tests/test_gpu_affine.py.

Frame k has a 2 x 3 matrix [a b tx; c d ty] in HR pixel coordinates, (x, y) order: F(p) = L p + t, content at p in the HR
image sits at F(p) in the frame's HR-grid image.  The warp is stated as explicit (row, col, weight) triplets of its
matrix: (M x)(q) = sum of four bilinear taps of x at s = F^-1(q), taps outside the image dropped.  Forward is a weighted
gather over the triplets, the adjoint np.add.at over the SAME triplets (the literal transpose); D B and its transpose come
from the CPU checker's ImageModel(shifts=None).  gather_adjoint states the library kernel's algorithm independently: per
HR pixel p the candidates q are the integers inside F(p) +- (|a|+|b|, |c|+|d|), weights recomputed from s = F^-1(q).
"""
import os
import sys

import numpy as np

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_restatement as rr  # noqa: E402

MAX_DEVIATION = 0.25  # max(|a-1|+|b|, |c|+|d-1|): the domain of the entry point


def deviation(M):
    M = np.asarray(M, dtype=np.float64).reshape(2, 3)
    return max(abs(M[0, 0] - 1) + abs(M[0, 1]), abs(M[1, 0]) + abs(M[1, 1] - 1))


def inverse_map(M):
    """[ia ib itx; ic id ity] of F^-1, formed as the library forms it."""
    (a, b, tx), (c, d, ty) = np.asarray(M, dtype=np.float64).reshape(2, 3)
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    return np.array([[ia, ib, -(ia * tx + ib * ty)], [ic, id_, -(ic * tx + id_ * ty)]])


def source_coords(Minv, qx, qy):
    sx = Minv[0, 0] * qx + (Minv[0, 1] * qy + Minv[0, 2])
    sy = Minv[1, 0] * qx + (Minv[1, 1] * qy + Minv[1, 2])
    return sx, sy


def warp_triplets(M, W, H):
    """(rows, cols, weights) of the H*W x H*W warp matrix: row = q (warped image), col = p (HR image), row-major."""
    Minv = inverse_map(M)
    qy, qx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    sx, sy = source_coords(Minv, qx.ravel(), qy.ravel())
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    q = np.arange(H * W)
    rows, cols, wts = [], [], []
    for dy, dx, w in ((0, 0, (1 - fy) * (1 - fx)), (0, 1, (1 - fy) * fx), (1, 0, fy * (1 - fx)), (1, 1, fy * fx)):
        px, py = x0 + dx, y0 + dy
        ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        rows.append(q[ok])
        cols.append((py[ok] * W + px[ok]).astype(np.int64))
        wts.append(w[ok])
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(wts)


def warp_forward(trip, x):
    """x [C][H][W] -> M x."""
    rows, cols, w = trip
    C, H, W = x.shape
    out = np.zeros((C, H * W))
    flat = x.reshape(C, -1)
    for c in range(C):
        np.add.at(out[c], rows, w * flat[c, cols])
    return out.reshape(C, H, W)


def warp_transpose(trip, u):
    """u [C][H][W] -> M^T u: np.add.at over the same triplets."""
    rows, cols, w = trip
    C, H, W = u.shape
    out = np.zeros((C, H * W))
    flat = u.reshape(C, -1)
    for c in range(C):
        np.add.at(out[c], cols, w * flat[c, rows])
    return out.reshape(C, H, W)


def _axis_weight(s, p):
    s0 = np.floor(s)
    f = s - s0
    return np.where(s0 == p, 1.0 - f, np.where(s0 + 1.0 == p, f, 0.0))


def gather_adjoint(M, u, return_counts=False):
    """M^T u in the kernel's gather form: per HR pixel p, at most 3 x 3 candidates q = ceil(F(p) - radius) + (0..2)^2 in
    row-major order, weight = axis weight of p for a sample at s = F^-1(q) (the forward's (1 - f) / f, else 0)."""
    Mm = np.asarray(M, dtype=np.float64).reshape(2, 3)
    Minv = inverse_map(Mm)
    C, H, W = u.shape
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cx = Mm[0, 0] * px + (Mm[0, 1] * py + Mm[0, 2])
    cy = Mm[1, 0] * px + (Mm[1, 1] * py + Mm[1, 2])
    rx = abs(Mm[0, 0]) + abs(Mm[0, 1]) + 1e-9
    ry = abs(Mm[1, 0]) + abs(Mm[1, 1]) + 1e-9
    qx0, qy0 = np.ceil(cx - rx), np.ceil(cy - ry)
    out = np.zeros((C, H, W))
    counts = np.zeros((H, W), dtype=np.int64)
    for dy in range(3):
        for dx in range(3):
            qx, qy = qx0 + dx, qy0 + dy
            ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            sx, sy = source_coords(Minv, qx, qy)
            w = np.where(ok, _axis_weight(sy, py) * _axis_weight(sx, px), 0.0)
            counts += w != 0
            iy, ix = np.clip(qy, 0, H - 1).astype(np.int64), np.clip(qx, 0, W - 1).astype(np.int64)
            out += w[None] * u[:, iy, ix]
    if return_counts:
        # candidates outside the 3 x 3 box would be missed: count what the full footprint test finds
        return out, counts
    return out


class AffineImageModel(orc.ImageModel):
    """ImageModel with the MotionModule replaced by per-frame affine warps: A_k = D B M_k."""

    def __init__(self, scale, matrices, blur_ksize=0, blur_sigma=0.0):
        self.matrices = np.ascontiguousarray(matrices, dtype=np.float64).reshape(-1, 2, 3)
        super().__init__(scale, None, blur_ksize, blur_sigma, num_frames=len(self.matrices))
        self._db = orc.ImageModel(scale=scale, shifts=None, blur_ksize=blur_ksize, blur_sigma=blur_sigma)
        self._trip = {}

    def triplets(self, k, W, H):
        key = (k, W, H)
        if key not in self._trip:
            self._trip[key] = warp_triplets(self.matrices[k], W, H)
        return self._trip[key]

    def apply(self, hr, k):
        x = np.ascontiguousarray(hr, dtype=np.float64)
        _, H, W = x.shape
        return self._db.apply(warp_forward(self.triplets(k, W, H), x), k)

    def apply_transpose(self, lr, k):
        u = self._db.apply_transpose(np.ascontiguousarray(lr, dtype=np.float64), k)
        _, H, W = u.shape
        return warp_transpose(self.triplets(k, W, H), u)

    def apply_transpose_gather(self, lr, k):
        u = self._db.apply_transpose(np.ascontiguousarray(lr, dtype=np.float64), k)
        return gather_adjoint(self.matrices[k], u)


def translation(dx, dy):
    return np.array([[1.0, 0.0, dx], [0.0, 1.0, dy]])


def rotation_about_centre(deg, shift, W, H, scale=1.0):
    """[a b tx; c d ty] of p -> scale * R(deg) (p - centre) + centre + shift, centre = ((W-1)/2, (H-1)/2)."""
    th = np.deg2rad(deg)
    L = scale * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    t = c - L @ c + np.asarray(shift, dtype=np.float64)
    return np.hstack([L, t[:, None]])


def random_matrix(rng, dev, shift=3.0, at_bound=False):
    """A matrix whose deviation max(|a-1|+|b|, |c|+|d-1|) is `dev` in one row (at_bound) or below it."""
    M = np.zeros((2, 3))
    for r in range(2):
        v = rng.uniform(-1, 1, 2)
        v *= (dev if at_bound else dev * rng.uniform(0.2, 1.0)) / np.sum(np.abs(v))
        M[r, :2] = v
    M[0, 0] += 1.0
    M[1, 1] += 1.0
    if at_bound:
        # rounding must not push the sum past the bound
        while deviation(M) > dev:
            M[:, :2] = np.eye(2) + (M[:, :2] - np.eye(2)) * (1 - 1e-15)
    M[:, 2] = rng.uniform(-shift, shift, 2)
    return M


# ---- the two inputs of the affine model's figures (README) ----
TABLE_SHIFTS = [[0, 0], [1.25, .75], [.5, 1], [1, .25], [-.75, 1.5], [.25, -1]]
TABLE_ROTATIONS = {"0.5deg": [0, .5, -.3, .2, -.5, .4], "2deg": [0, 2, -1.2, .8, -2, 1.6]}


def table_inputs():
    """96 x 128 HR, scale 2, 6 frames, blur 3 / sigma 1, BTV(2, 0.5) lambda 0.005, noise sigma 0.01 (seed 7), the sub-pixel
    shifts above, each frame rotated about the image centre.  Returns the geometry, the ground truth, the translation-only
    model, and inputs = {name: (matrices, affine model, y)}."""
    C, H, W, s, K = 1, 96, 128, 2, 6
    gt = rr.prototype_ground_truth(C, H, W)
    inputs = {}
    for name, degs in TABLE_ROTATIONS.items():
        mats = np.stack([rotation_about_centre(degs[k], TABLE_SHIFTS[k], W, H) for k in range(K)])
        model = AffineImageModel(s, mats, 3, 1.0)
        clean = np.stack([model.apply(gt, k) for k in range(K)])
        y = clean + 0.01 * np.random.default_rng(7).standard_normal(clean.shape)
        inputs[name] = (mats, model, y)
    trans = orc.ImageModel(scale=s, shifts=TABLE_SHIFTS, blur_ksize=3, blur_sigma=1.0)
    return dict(C=C, H=H, W=W, s=s, K=K, shifts=TABLE_SHIFTS, blur=(3, 1.0), gt=gt, translation_model=trans,
                reg=(orc.REG_BTV, 0.005, 2, 0.5), delta=0.02, inputs=inputs)
