"""numpy / scipy.sparse restatement of the dense displacement-field motion model (include/srmap.h: srmap_problem_set_flow;
DESIGN.md 3.11) -- the checker of tests/test_flow_cpu.py and tests/test_gpu_flow.py, written from the definition, not from
the kernels.

  forward    A_k = D B M_k as explicit sparse matrices.  M_k: row q holds the four bilinear taps of x at s = q + u_k(q),
             taps outside the image dropped; B and D are tests/blur_kernel_restatement.py's (the literal correlation, one 1
             per LR pixel).  The field is first rounded to the storage dtype, as the library stores it; s is then exact.
  adjoint    the literal transpose (scipy's .T).
  gather     the library's way to that transpose, stated independently (seeds, window_violations, gather_adjoint): a seed
             per HR pixel p from the fixed-point iteration q <- round(p - u(clamp(q))), the (2 r + 1)^2 window around it,
             the weights recomputed from s; and the set-time check that every (q, p) pair of M lies inside p's window.
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import blur_kernel_restatement as bk  # noqa: E402
import robust_restatement as rr  # noqa: E402

RADIUS = 2            # the gather scans (2 * RADIUS + 1)^2 candidates around the seed
SEED_STEPS = 16       # fixed-point steps (the iteration stops early at a fixed point)
MAX_DISPLACEMENT = 2.0 ** 20
NEIGHBOUR_BOUND = 0.4  # dx + dy of neighbour_differences(): the documented sufficient condition


# ------------------------------------------------------------------------------------------- the warp
def stored(field, dtype=np.float64):
    """The field as the library keeps it: rounded once to the problem's dtype."""
    return np.asarray(field, dtype=np.float64).astype(dtype).astype(np.float64)


def warp_triplets(field, W, H):
    """(rows, cols, weights) of M for one frame's field [2][H][W]: row = q (warped image), col = p (HR image)."""
    field = np.asarray(field, dtype=np.float64).reshape(2, H, W)
    qy, qx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    sx, sy = (qx + field[0]).ravel(), (qy + field[1]).ravel()
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


def warp_matrix(field, W, H):
    rows, cols, w = warp_triplets(field, W, H)
    return sp.csr_matrix((w, (rows, cols)), shape=(H * W, H * W))


class FlowModel(bk.BlurKernelModel):
    """A_k = D B M_k with per-frame displacement fields [K][2][H][W]; taps: the blur's ksize x ksize taps ([[1]] = none)."""

    def __init__(self, scale, fields, taps, dtype=np.float64):
        fields = np.asarray(fields, dtype=np.float64)
        K, _, H, W = fields.shape
        super().__init__(scale, K, H, W, taps, motion=None)
        self.fields = stored(fields, dtype)
        self.Mk = [warp_matrix(self.fields[k], W, H) for k in range(K)]
        self.A = [(self.D @ self.B @ M).tocsr() for M in self.Mk]
        self.At = [A.T.tocsr() for A in self.A]


def gaussian_model(scale, fields, blur_ksize=0, blur_sigma=0.0, dtype=np.float64):
    return FlowModel(scale, fields, bk.gaussian_taps(blur_ksize, blur_sigma), dtype)


# ------------------------------------------------------------------------------------------- the gather, restated
def seeds(field, W, H, steps=SEED_STEPS):
    """(qx, qy) int arrays [H][W]: per HR pixel p the iterate of q <- round(p - u(clamp(q))) from q = p (ties to even),
    stopped at a fixed point, then clamped to the image widened by RADIUS."""
    field = np.asarray(field, dtype=np.float64).reshape(2, H, W)
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    qx, qy = px.copy(), py.copy()
    live = np.ones((H, W), dtype=bool)
    for _ in range(steps):
        cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
        nx = np.rint(px - field[0][cy, cx]).astype(np.int64)
        ny = np.rint(py - field[1][cy, cx]).astype(np.int64)
        moved = live & ((nx != qx) | (ny != qy))
        qx, qy = np.where(moved, nx, qx), np.where(moved, ny, qy)
        live = moved
        if not live.any():
            break
    return np.clip(qx, -RADIUS, W - 1 + RADIUS), np.clip(qy, -RADIUS, H - 1 + RADIUS)


def window_violations(field, W, H, seed=None, radius=RADIUS):
    """The number of (q, p) pairs of M (weight not zero, p inside the image) with q outside the window around p's seed:
    0 = the gather is complete."""
    rows, cols, w = warp_triplets(field, W, H)
    sx, sy = seeds(field, W, H) if seed is None else seed
    rows, cols = rows[w != 0], cols[w != 0]
    qy, qx = rows // W, rows % W
    py, px = cols // W, cols % W
    return int(np.sum((np.abs(qx - sx[py, px]) > radius) | (np.abs(qy - sy[py, px]) > radius)))


def max_seed_distance(field, W, H):
    """The largest per-axis distance between a contributing q and its p's seed (<= RADIUS for an accepted field)."""
    rows, cols, w = warp_triplets(field, W, H)
    sx, sy = seeds(field, W, H)
    rows, cols = rows[w != 0], cols[w != 0]
    if len(rows) == 0:
        return 0
    qy, qx = rows // W, rows % W
    py, px = cols // W, cols % W
    return int(max(np.max(np.abs(qx - sx[py, px])), np.max(np.abs(qy - sy[py, px]))))


def gather_adjoint(field, u, radius=RADIUS):
    """M^T u in the kernel's gather form: per HR pixel p the (2 r + 1)^2 candidates around its seed in row-major order,
    weight = the forward's axis weights of p for a sample at s = q + u(q)."""
    C, H, W = u.shape
    field = np.asarray(field, dtype=np.float64).reshape(2, H, W)
    sx0, sy0 = seeds(field, W, H)
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros((C, H, W))
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            qx, qy = sx0 + dx, sy0 + dy
            ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            ix, iy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            sx, sy = ix + field[0][iy, ix], iy + field[1][iy, ix]
            w = np.where(ok, ar._axis_weight(sy, py) * ar._axis_weight(sx, px), 0.0)
            out += w[None] * u[:, iy, ix]
    return out


def classify(field, W, H):
    """What srmap_problem_set_flow answers for one frame's (stored) field: "ok", "einval" (not finite), "eunsupported"
    (beyond 2^20, or a pair outside its window)."""
    field = np.asarray(field, dtype=np.float64)
    if not np.all(np.isfinite(field)):
        return "einval"
    if np.any(np.abs(field) > MAX_DISPLACEMENT):
        return "eunsupported"
    return "ok" if window_violations(field, W, H) == 0 else "eunsupported"


# ------------------------------------------------------------------------------------------- fields
def neighbour_differences(field):
    """(dx, dy): the largest max-norm difference of u between horizontal / vertical neighbours."""
    f = np.asarray(field, dtype=np.float64)
    f = f.reshape((-1,) + f.shape[-3:])
    dx = np.max(np.abs(f[..., :, 1:] - f[..., :, :-1])) if f.shape[-1] > 1 else 0.0
    dy = np.max(np.abs(f[..., 1:, :] - f[..., :-1, :])) if f.shape[-2] > 1 else 0.0
    return float(dx), float(dy)


def from_shifts(shifts, H, W):
    """MotionShift (dx, dy) -> u = (-dx, -dy)."""
    s = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    out = np.empty((len(s), 2, H, W))
    out[:, 0] = -s[:, 0, None, None]
    out[:, 1] = -s[:, 1, None, None]
    return out


def from_affine(matrices, H, W):
    """u(q) = F^-1(q) - q, with F^-1 and its evaluation as the affine restatement forms them."""
    m = np.asarray(matrices, dtype=np.float64).reshape(-1, 2, 3)
    qy, qx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.empty((len(m), 2, H, W))
    for k, M in enumerate(m):
        sx, sy = ar.source_coords(ar.inverse_map(M), qx, qy)
        out[k, 0], out[k, 1] = sx - qx, sy - qy
    return out


def sinusoid(H, W, amplitude, wavelength, offset=(0.0, 0.0), phase=0.0):
    """u = offset + amplitude * (sin, cos) of crossed plane waves of the given wavelength."""
    qy, qx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a = 2 * np.pi / wavelength
    ux = offset[0] + amplitude * np.sin(a * (qx + 0.5 * qy) + phase)
    uy = offset[1] + amplitude * np.cos(a * (0.6 * qx - qy) + 2 * phase)
    return np.stack([ux, uy])


def at_bound(field, bound=NEIGHBOUR_BOUND, keep_mean=True):
    """The field's variation about its mean scaled so that dx + dy of neighbour_differences() is `bound` (from below)."""
    f = np.asarray(field, dtype=np.float64)
    mean = f.mean(axis=(-2, -1), keepdims=True) if keep_mean else 0.0
    v = f - mean
    dx, dy = neighbour_differences(v)
    v = v * (bound / (dx + dy))
    while sum(neighbour_differences(mean + v)) > bound:
        v = v * (1 - 1e-12)
    return mean + v


def smooth_random(rng, H, W, amplitude, spacing=24, cap=0.35):
    """A smooth random field: smoothstep interpolation of a coarse random grid (nodes `spacing` px apart) of the given
    amplitude, scaled down where needed so that dx + dy of neighbour_differences() stays within `cap`."""
    gy, gx = max(2, H // spacing + 1), max(2, W // spacing + 1)
    out = np.empty((2, H, W))
    for c in range(2):
        coarse = rng.uniform(-1, 1, (gy, gx))
        yy = np.linspace(0, gy - 1, H)
        xx = np.linspace(0, gx - 1, W)
        y0, x0 = np.minimum(yy.astype(int), gy - 2), np.minimum(xx.astype(int), gx - 2)
        fy, fx = (yy - y0)[:, None], (xx - x0)[None, :]
        fy, fx = fy * fy * (3 - 2 * fy), fx * fx * (3 - 2 * fx)
        a, b = coarse[y0][:, x0], coarse[y0][:, x0 + 1]
        c_, d = coarse[y0 + 1][:, x0], coarse[y0 + 1][:, x0 + 1]
        out[c] = amplitude * ((1 - fy) * ((1 - fx) * a + fx * b) + fy * ((1 - fx) * c_ + fx * d))
    d = sum(neighbour_differences(out))
    return out * (cap / d) if d > cap else out


def folded(H, W):
    """A field that folds: over the middle third of the columns every pixel of a row samples the SAME source column, so one
    HR pixel has a whole run of contributing q -- no 5 x 5 window holds them."""
    qy, qx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    lo, hi = W // 3, 2 * W // 3
    ux = np.where((qx >= lo) & (qx < hi), (lo + 0.5) - qx, 0.0)
    return np.stack([ux, np.zeros((H, W))])


# ------------------------------------------------------------------------------------------- the table's inputs
TABLE_AMPLITUDE = 1.5


def table_fields(H, W, shifts):
    """Frame 0: its translation alone.  Frames 1...5: the translation plus a smooth deformation of amplitude 1.5 HR px and
    wavelength 64 ... 96 px (largest neighbour difference 1.5 * 2 pi / 64 = 0.147 px)."""
    K = len(shifts)
    out = from_shifts(shifts, H, W)
    qy, qx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for k in range(1, K):
        lam_x, lam_y = 64.0 + 8.0 * (k - 1), 96.0 - 8.0 * (k - 1)
        out[k, 0] += TABLE_AMPLITUDE * np.sin(2 * np.pi * qy / lam_x + 0.9 * k)
        out[k, 1] += TABLE_AMPLITUDE * np.sin(2 * np.pi * qx / lam_y + 1.7 * k)
    return out


def table_inputs():
    """The robust table's geometry (96 x 128 HR, scale 2, 6 frames, blur 3 / sigma 1, BTV(2, 0.5) lambda 0.005, noise sigma
    0.01 seed 7) with the affine table's sub-pixel shifts.  `deformed`: frames made through table_fields(); `undeformed`:
    frames made through the translations alone (the ceiling a perfect motion model reaches)."""
    C, H, W, s, K = 1, 96, 128, 2, 6
    shifts = ar.TABLE_SHIFTS
    gt = rr.prototype_ground_truth(C, H, W)
    fields = table_fields(H, W, shifts)
    model = gaussian_model(s, fields, 3, 1.0)
    trans = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=3, blur_sigma=1.0)

    def frames(m):
        clean = np.stack([m.apply(gt, k) for k in range(K)])
        return clean + 0.01 * np.random.default_rng(7).standard_normal(clean.shape)

    return dict(C=C, H=H, W=W, s=s, K=K, shifts=shifts, blur=(3, 1.0), gt=gt, fields=fields, model=model,
                translation_model=trans, y=frames(model), y_undeformed=frames(trans),
                reg=(orc.REG_BTV, 0.005, 2, 0.5), delta=0.02)


# PSNR in dB (IRLS rounds, CG iterations, evaluations) of rr.irls_solve(..., composed=True) from the bilinear upsampling of
# frame 0, with the reference's ALGLIB (oracle/_ref) as the inner minimiser.  test_flow_cpu.py re-derives and pins them.
TABLE = {
    "bilinear": (32.534, None),
    "translation_l2": (21.463, (8, 120, 181)),
    "translation_huber": (28.065, (8, 153, 226)),
    "flow_l2": (38.102, (7, 112, 170)),
    "flow_huber": (38.139, (7, 110, 166)),
    "flow_lbfgs": (38.048, (6, 111, 148)),
    "undeformed_l2": (38.026, (8, 126, 189)),
}
