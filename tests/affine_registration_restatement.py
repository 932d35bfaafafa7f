"""numpy restatement of the affine registration (include/srmap.h: srmap_register_affine) -- the checker of
tests/test_affine_registration_cpu.py and tests/test_gpu_affine_registration.py, written from the definition, not from
the kernels.

For every frame k >= 1 find F_k(p) = L_k p + t_k with I_k(F_k(p)) ~= I_0(p) (the affine model's and MotionShift's
convention: content at p of frame 0 sits at F_k(p) in frame k), as a 2 x 3 matrix [a b tx; c d ty], (x, y) order.

  pyramid   2 x 2 box means (an odd last row / column dropped), halved while min(w, h) >= 64, at most 12 levels
  seed      coarsest level, integer u in [-R, R]^2, R = max(4, min(16, min side / 4)): mean squared difference of
            I_k(p + u) - I_0(p) over the FIXED template window [R, w-R) x [R, h-R); first minimum in row-major order
  GN        inverse compositional, coarse to fine.  Per pass, over template pixels p at least 1 px from the border whose
            four bilinear taps of I_k at s = F(p) are all inside: e = I_k(s) - I_0(p), (gx, gy) central differences of
            I_0, (u, v) = p - c, c = ((w-1)/2, (h-1)/2), J = (gx u, gx v, gx, gy u, gy v, gy); H = sum J J^T, g = sum J e.
            Cholesky H D = g; W(p) = p + [D0 D1; D3 D4](p - c) + (D2, D5); F <- F o W^-1.
  transfer  fine p = 2 u + 1/2: L unchanged, t_fine = 2 t_coarse + (1/2, 1/2) - L (1/2, 1/2).
"""
import numpy as np

MAX_DEVIATION = 0.25
MAX_LEVELS = 12
CHOLESKY_PIVOT_RTOL = 1e-12  # a pivot at or below this fraction of its diagonal entry: no texture


class RegistrationError(ValueError):
    """Could not determine motion between images (SRMAP_EINVAL)."""


def deviation(M):
    M = np.asarray(M, dtype=np.float64).reshape(2, 3)
    return max(abs(M[0, 0] - 1) + abs(M[0, 1]), abs(M[1, 0]) + abs(M[1, 1] - 1))


def identity():
    return np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def down2(img):
    h2, w2 = img.shape[0] // 2, img.shape[1] // 2
    a = img[:2 * h2, :2 * w2]
    return 0.25 * ((a[0::2, 0::2] + a[0::2, 1::2]) + (a[1::2, 0::2] + a[1::2, 1::2]))


def num_levels(w, h, max_levels=0):
    n = 1
    while min(w, h) >= 64 and n < MAX_LEVELS:
        w, h, n = w // 2, h // 2, n + 1
    return n if max_levels <= 0 else min(n, max_levels)


def pyramid(img, levels):
    out = [np.ascontiguousarray(img, dtype=np.float64)]
    for _ in range(levels - 1):
        out.append(down2(out[-1]))
    return out


def to_finer(M):
    M = np.asarray(M, dtype=np.float64).reshape(2, 3)
    L, half = M[:, :2], np.array([0.5, 0.5])
    return np.hstack([L, (2.0 * M[:, 2] + half - L @ half)[:, None]])


def to_coarser(M):
    M = np.asarray(M, dtype=np.float64).reshape(2, 3)
    L, half = M[:, :2], np.array([0.5, 0.5])
    return np.hstack([L, (0.5 * (M[:, 2] - half + L @ half))[:, None]])


def apply_map(M, pts):
    """pts [n][2] (x, y) -> M pts."""
    M = np.asarray(M, dtype=np.float64).reshape(2, 3)
    return np.asarray(pts, dtype=np.float64) @ M[:, :2].T + M[:, 2]


def corner_displacement(A, B, w, h):
    """Largest distance between A(p) and B(p) over the four image corners p."""
    c = np.array([[0.0, 0.0], [w - 1.0, 0.0], [0.0, h - 1.0], [w - 1.0, h - 1.0]])
    return float(np.max(np.hypot(*(apply_map(A, c) - apply_map(B, c)).T)))


def increment_matrix(delta, w, h):
    """[A | t] of W(p) = p + D (p - c) + d."""
    D = np.array([[delta[0], delta[1]], [delta[3], delta[4]]])
    d = np.array([delta[2], delta[5]])
    c = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    return np.hstack([np.eye(2) + D, (d - D @ c)[:, None]])


def compose_with_inverse(F, Wm):
    """F o W^-1."""
    F = np.asarray(F, dtype=np.float64).reshape(2, 3)
    Ainv = np.linalg.inv(Wm[:, :2])
    L = F[:, :2] @ Ainv
    return np.hstack([L, (F[:, 2] - L @ Wm[:, 2])[:, None]])


def sample_positions(F, w, h):
    """s = F(p) for the interior template pixels, every operation rounded on its own: a x + (b y + t)."""
    F = np.asarray(F, dtype=np.float64).reshape(2, 3)
    py, px = np.meshgrid(np.arange(1, h - 1, dtype=np.float64), np.arange(1, w - 1, dtype=np.float64), indexing="ij")
    sx = F[0, 0] * px + (F[0, 1] * py + F[0, 2])
    sy = F[1, 0] * px + (F[1, 1] * py + F[1, 2])
    return px, py, sx, sy


def _total(a, order):
    """Sum of a 2-D array's entries, taken in one of several orders (the sensitivity probe of the GPU tests)."""
    if order == "rows":
        return float(np.sum(np.sum(a, axis=1)))
    if order == "cols":
        return float(np.sum(np.sum(a, axis=0)))
    if order == "reversed":
        return float(np.sum(np.sum(a[::-1, ::-1], axis=1)))
    raise ValueError(order)


def gn_sums(ref, img, F, order="rows"):
    """(H [6][6], g [6], sum e^2, n) of one pass."""
    h, w = ref.shape
    px, py, sx, sy = sample_positions(F, w, h)
    with np.errstate(invalid="ignore"):
        ok = (sx >= 0) & (sx < w - 1) & (sy >= 0) & (sy < h - 1)
    sxs, sys_ = np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)
    x0, y0 = np.floor(sxs).astype(np.int64), np.floor(sys_).astype(np.int64)
    fx, fy = sxs - x0, sys_ - y0
    val = (1 - fy) * ((1 - fx) * img[y0, x0] + fx * img[y0, x0 + 1]) + fy * ((1 - fx) * img[y0 + 1, x0] + fx * img[y0 + 1, x0 + 1])
    m = ok.astype(np.float64)
    e = m * (val - ref[1:-1, 1:-1])
    gx = m * 0.5 * (ref[1:-1, 2:] - ref[1:-1, :-2])
    gy = m * 0.5 * (ref[2:, 1:-1] - ref[:-2, 1:-1])
    u, v = px - (w - 1) / 2.0, py - (h - 1) / 2.0
    J = [gx * u, gx * v, gx, gy * u, gy * v, gy]
    H = np.zeros((6, 6))
    g = np.zeros(6)
    for i in range(6):
        g[i] = _total(J[i] * e, order)
        for j in range(i, 6):
            H[i, j] = H[j, i] = _total(J[i] * J[j], order)
    return H, g, _total(e * e, order), int(np.count_nonzero(ok))


def cholesky_solve(H, g):
    """Solution of H x = g by Cholesky, or None where a pivot is not above CHOLESKY_PIVOT_RTOL of its diagonal entry."""
    n = len(g)
    Lc = np.zeros((n, n))
    for j in range(n):
        p = H[j, j] - np.dot(Lc[j, :j], Lc[j, :j])
        if not (H[j, j] > 0.0 and p > CHOLESKY_PIVOT_RTOL * H[j, j]):
            return None
        Lc[j, j] = np.sqrt(p)
        for i in range(j + 1, n):
            Lc[i, j] = (H[i, j] - np.dot(Lc[i, :j], Lc[j, :j])) / Lc[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (g[i] - np.dot(Lc[i, :i], y[:i])) / Lc[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - np.dot(Lc[i + 1:, i], x[i + 1:])) / Lc[i, i]
    return x


def gn_step(ref, img, F, order="rows"):
    """One Gauss-Newton pass: (new F or None on a Cholesky failure, sum e^2, n)."""
    h, w = ref.shape
    H, g, ee, n = gn_sums(ref, img, F, order)
    delta = cholesky_solve(H, g)
    if delta is None:
        return None, ee, n
    return compose_with_inverse(F, increment_matrix(delta, w, h)), ee, n


def search_radius(w, h):
    return max(4, min(16, min(w, h) // 4))


def search_separation(msd, bi):
    """1 - best / runner-up of a square candidate table (row-major; a negative entry: not evaluated), the runner-up being
    the smallest entry at least 2 cells (Chebyshev) from the best one `bi`; 0 without a positive runner-up."""
    msd = np.asarray(msd, dtype=np.float64)
    n1 = msd.shape[0]
    by, bx = divmod(int(bi), n1)
    yy, xx = np.mgrid[0:n1, 0:n1]
    far = (np.maximum(np.abs(xx - bx), np.abs(yy - by)) >= 2) & (msd >= 0)
    runner = np.min(msd[far]) if np.any(far) else -1.0
    return float(1.0 - msd[by, bx] / runner) if runner > 0 else 0.0


def coarse_seed(ref, img):
    """((ux, uy), separation): exhaustive search over the fixed central window.  An empty window answers (0, 0), 0."""
    h, w = ref.shape
    R = search_radius(w, h)
    if w - 2 * R <= 0 or h - 2 * R <= 0:
        return (0, 0), 0.0
    n1 = 2 * R + 1
    t = ref[R:h - R, R:w - R]
    msd = np.zeros((n1, n1))
    for iy in range(n1):
        for ix in range(n1):
            d = img[iy:iy + h - 2 * R, ix:ix + w - 2 * R] - t
            msd[iy, ix] = np.sum(d * d) / t.size
    bi = int(np.argmin(msd))  # first minimum, row-major
    by, bx = divmod(bi, n1)
    return (bx - R, by - R), search_separation(msd, bi)


def register_pair(ref_img, img, init=None, max_iterations=30, step_tolerance=1e-4, max_levels=0):
    """(F at full resolution, quality [4], iterations per level coarse to fine)."""
    h, w = ref_img.shape
    L = num_levels(w, h, max_levels)
    pr, pi = pyramid(ref_img, L), pyramid(img, L)
    if init is None:
        (ux, uy), sep = coarse_seed(pr[-1], pi[-1])
        F = np.array([[1.0, 0.0, float(ux)], [0.0, 1.0, float(uy)]])
    else:
        F = np.array(init, dtype=np.float64).reshape(2, 3)
        if not np.all(np.isfinite(F)) or deviation(F) > MAX_DEVIATION:
            raise RegistrationError("bad initial matrix")
        sep = 1.0
        for _ in range(L - 1):
            F = to_coarser(F)
    its = []
    for l in range(L - 1, -1, -1):
        a, b = pr[l], pi[l]
        lh, lw = a.shape
        n_it = 0
        for _ in range(max_iterations):
            Fn, _, n = gn_step(a, b, F)
            n_it += 1
            if n < 0.25 * lw * lh:
                raise RegistrationError("Could not determine motion between images.")
            if Fn is None:
                break
            if deviation(Fn) > MAX_DEVIATION or not np.all(np.isfinite(Fn)):
                raise RegistrationError("Could not determine motion between images.")
            step = corner_displacement(Fn, F, lw, lh)
            F = Fn
            if step < step_tolerance:
                break
        its.append(n_it)
        if l > 0:
            F = to_finer(F)
    _, _, ee, n = gn_sums(pr[0], pi[0], F)
    q = [sep, float(np.sqrt(ee / n)) if n > 0 else 0.0, n / float(w * h), float(sum(its))]
    return F, q, its


def register_affine(images, hr_scale=1, init=None, max_iterations=30, step_tolerance=1e-4, max_levels=0,
                    with_quality=False):
    """images [n][H][W] -> [n][2][3] (and quality [n][4]); image 0 gets the identity; t is multiplied by hr_scale."""
    images = np.asarray(images, dtype=np.float64)
    n = images.shape[0]
    out, q = np.zeros((n, 2, 3)), np.zeros((n, 4))
    if n == 0:
        return (out, q) if with_quality else out
    if images.shape[1] < 8 or images.shape[2] < 8:
        raise RegistrationError("registration needs images of at least 8 x 8")
    for k in range(n):
        if not np.all(np.isfinite(images[k])):
            raise RegistrationError("affine registration: image %d is not finite" % k)
    out[0], q[0] = identity(), [1.0, 0.0, 1.0, 0.0]
    for k in range(1, n):
        F, qk, _ = register_pair(images[0], images[k], None if init is None else np.asarray(init).reshape(n, 2, 3)[k],
                                 max_iterations, step_tolerance, max_levels)
        F[:, 2] *= hr_scale
        out[k], q[k] = F, qk
    return (out, q) if with_quality else out
