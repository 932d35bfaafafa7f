"""numpy / scipy.sparse restatement of the free-form blur kernel and of its calibration fit (include/srmap.h:
srmap_problem_set_blur_kernel, srmap_fit_blur) -- the checker of tests/test_blur_kernel_cpu.py and
tests/test_gpu_blur_kernel.py, written from the definition, not from the kernels.

  forward    A_k = D B M_k as explicit sparse matrices:
             M_k   the warp: from the CPU checker's warpAffine tables for a translation (source row / column << 5 | 1/32-px
                   fraction, the float32 products of BilinearTab_f), from affine_restatement's triplets for an affine matrix,
                   the identity without motion;
             B     the literal correlation (B z)(R, C) = sum_{a,e} taps[a][e] z(R + a - hb, C + e - hb), zero outside;
             D     one 1 per LR pixel at its decimation source;
  adjoint    the literal transpose A_k^T = M_k^T B^T D^T of those matrices (scipy's .T): for the correlation that IS the
             correlation with the kernel flipped in both axes -- and not with the matrix-transposed kernel, which
             blur_transpose_matrix(..., "matrix_transpose") builds so that a test can show the difference;
  fit        columns s_t = (M_k x)(R0 + a - hb, C0 + e - hb) (0 outside the image) per LR pixel and channel, the Gram of
             [s_0 ... s_{n-1}, y] under w by S.T @ (w * S), the taps by the KKT system of
             min (h^T (G + mu I) h - 2 h^T (b + mu h_cur)) subject to (optionally) sum h = 1.
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import robust_restatement as rr  # noqa: E402

STATUS_OK, STATUS_NO_TEXTURE = 0, 3
PIVOT_RTOL = 1e-12


# ------------------------------------------------------------------------------------------- the three factors
def decimation_matrix(H, W, s):
    """(D [h w x H W], row map, column map)."""
    h, w = orc.downsampled_len(H, s), orc.downsampled_len(W, s)
    rmap, cmap = orc.nearest_map(H, h).astype(np.int64), orc.nearest_map(W, w).astype(np.int64)
    cols = (rmap[:, None] * W + cmap[None, :]).ravel()
    return sp.csr_matrix((np.ones(h * w), (np.arange(h * w), cols)), shape=(h * w, H * W)), rmap, cmap


def blur_matrix(taps, H, W):
    """B [H W x H W]: the correlation with `taps`, zero border."""
    taps = np.asarray(taps, dtype=np.float64)
    b = taps.shape[0]
    assert taps.shape == (b, b) and b % 2 == 1
    hb = (b - 1) // 2
    R, Cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rows, cols, vals = [], [], []
    for a in range(b):
        for e in range(b):
            rr_, cc = R + a - hb, Cc + e - hb
            ok = (rr_ >= 0) & (rr_ < H) & (cc >= 0) & (cc < W)
            rows.append((R * W + Cc)[ok])
            cols.append((rr_ * W + cc)[ok])
            vals.append(np.full(int(ok.sum()), taps[a, e]))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W))


def blur_transpose_matrix(taps, H, W, form="flip"):
    """The correlation matrix of the kernel an adjoint would use: "flip" = flipped in both axes (equals blur_matrix(taps).T),
    "matrix_transpose" = taps.T (the reference's kernel.t(): the adjoint only for a kernel symmetric under both flips)."""
    taps = np.asarray(taps, dtype=np.float64)
    return blur_matrix(taps[::-1, ::-1] if form == "flip" else taps.T, H, W)


def shift_warp_matrix(W, H, dx, dy):
    """M [H W x H W] of MotionModule's warp by (dx, dy), from the checker's warpAffine tables."""
    X, Y = orc.warp_tables(W, H, float(dx), float(dy))
    X, Y = X.astype(np.int64), Y.astype(np.int64)
    sc, fx = X >> 5, (X & 31).astype(np.float32)
    sr, fy = Y >> 5, (Y & 31).astype(np.float32)
    tx1 = fx * np.float32(1.0 / 32)
    tx0 = np.float32(1) - tx1
    ty1 = fy * np.float32(1.0 / 32)
    ty0 = np.float32(1) - ty1
    q = np.arange(H * W).reshape(H, W)
    rows, cols, vals = [], [], []
    for d_r, d_c, wy, wx in ((0, 0, ty0, tx0), (0, 1, ty0, tx1), (1, 0, ty1, tx0), (1, 1, ty1, tx1)):
        wgt = (wy[:, None] * wx[None, :]).astype(np.float64)  # float32 products, as BilinearTab_f holds them
        pr, pc = (sr + d_r)[:, None] + 0 * q, (sc + d_c)[None, :] + 0 * q
        ok = (pr >= 0) & (pr < H) & (pc >= 0) & (pc < W) & (wgt != 0)
        rows.append(q[ok])
        cols.append((pr * W + pc)[ok])
        vals.append(wgt[ok])
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W))


def affine_warp_matrix(M, W, H):
    rows, cols, w = ar.warp_triplets(M, W, H)
    return sp.csr_matrix((w, (rows, cols)), shape=(H * W, H * W))


def warp_matrix(motion, k, W, H):
    """motion: None, ("shifts", [K][2]) or ("affine", [K][2][3])."""
    if motion is None:
        return sp.identity(H * W, format="csr")
    kind, val = motion
    val = np.asarray(val, dtype=np.float64)
    return shift_warp_matrix(W, H, val[k][0], val[k][1]) if kind == "shifts" else affine_warp_matrix(val[k], W, H)


# ------------------------------------------------------------------------------------------- the model
class BlurKernelModel(orc.ImageModel):
    """A_k = D B M_k with a free-form B, as sparse matrices; apply / apply_transpose as orc.ImageModel has them."""

    def __init__(self, scale, K, H, W, taps, motion=None, adjoint="exact"):
        super().__init__(scale, None, 0, 0.0, num_frames=K)
        self.H, self.W, self.K = H, W, K
        self.taps = np.asarray(taps, dtype=np.float64)
        self.motion = motion
        self.D, self.rmap, self.cmap = decimation_matrix(H, W, scale)
        self.B = blur_matrix(self.taps, H, W)
        self.Mk = [warp_matrix(motion, k, W, H) for k in range(K)]
        self.A = [(self.D @ self.B @ M).tocsr() for M in self.Mk]
        if adjoint == "exact":
            self.At = [A.T.tocsr() for A in self.A]
        else:  # the reference's form of the blur's transpose, for the test that tells the two apart
            Bt = blur_transpose_matrix(self.taps, H, W, "matrix_transpose")
            self.At = [(M.T @ Bt @ self.D.T).tocsr() for M in self.Mk]
        self.h, self.w = len(self.rmap), len(self.cmap)

    def apply(self, hr, k):
        x = np.ascontiguousarray(hr, dtype=np.float64)
        return np.stack([(self.A[k] @ x[c].ravel()).reshape(self.h, self.w) for c in range(x.shape[0])])

    def apply_transpose(self, lr, k):
        u = np.ascontiguousarray(lr, dtype=np.float64)
        return np.stack([(self.At[k] @ u[c].ravel()).reshape(self.H, self.W) for c in range(u.shape[0])])

    def data_term(self, y, w, x, want_grad=True, cost_rows=None):
        return rr.weighted_data_term(self, y, w, x, want_grad, cost_rows)


# ------------------------------------------------------------------------------------------- the fit
def fit_columns(x, motion, k, ksize, s):
    """S [C h w x ksize^2]: column t = (a, e) holds (M_k x)(R0 + a - hb, C0 + e - hb) per (channel, LR pixel), 0 outside."""
    x = np.asarray(x, dtype=np.float64)
    C, H, W = x.shape
    _, rmap, cmap = decimation_matrix(H, W, s)
    M = warp_matrix(motion, k, W, H)
    hb = (ksize - 1) // 2
    z = np.zeros((C, H + 2 * hb, W + 2 * hb))
    for c in range(C):
        z[c, hb:hb + H, hb:hb + W] = (M @ x[c].ravel()).reshape(H, W)
    cols = []
    for a in range(ksize):
        for e in range(ksize):
            cols.append(z[:, (rmap + a)[:, None], (cmap + e)[None, :]].reshape(-1))
    return np.stack(cols, axis=1)


def gram(x, y, w, motion, ksize, s, order="natural"):
    """Full (n + 1) x (n + 1) Gram of [s_0 ... s_{n-1}, y] under w over every frame; y, w [K][C][h][w] (w None = ones).
    order: the order the observations enter the sums in ("natural", "reversed", "transposed": the sensitivity probe)."""
    y = np.asarray(y, dtype=np.float64)
    K, C, h, wd = y.shape
    n = ksize * ksize
    G = np.zeros((n + 1, n + 1))
    frames = range(K) if order != "reversed" else range(K - 1, -1, -1)
    for k in frames:
        S = np.concatenate([fit_columns(x, motion, k, ksize, s), y[k].reshape(-1, 1)], axis=1)
        wk = np.ones(S.shape[0]) if w is None else np.asarray(w[k], dtype=np.float64).reshape(-1)
        if order == "reversed":
            S, wk = S[::-1], wk[::-1]
        elif order == "transposed":
            perm = np.arange(C * h * wd).reshape(C, h, wd).transpose(0, 2, 1).ravel()
            S, wk = S[perm], wk[perm]
        G += S.T @ (wk[:, None] * S)
    return G


def pack(G):
    """The upper triangle, row-major: the layout of normal_equations_out."""
    return G[np.triu_indices(G.shape[0])]


def unpack(sums, n):
    G = np.zeros((n + 1, n + 1))
    G[np.triu_indices(n + 1)] = sums
    return G + np.triu(G, 1).T


def resize_kernel(taps, ksize):
    """The kernel zero-padded or centre-cropped to ksize."""
    taps = np.asarray(taps, dtype=np.float64)
    b = taps.shape[0]
    out = np.zeros((ksize, ksize))
    if ksize >= b:
        o = (ksize - b) // 2
        out[o:o + b, o:o + b] = taps
    else:
        o = (b - ksize) // 2
        out = taps[o:o + ksize, o:o + ksize].copy()
    return out


def energy(G, h):
    v = np.concatenate([np.asarray(h, dtype=np.float64).ravel(), [-1.0]])
    return float(v @ G @ v)


def solve_taps(G, current, sum_to_one=True, ridge=0.0):
    """(taps [ksize][ksize], quality [5] = E at `current`, E at the fit, smallest / largest Cholesky pivot, status)."""
    n = G.shape[0] - 1
    ksize = int(round(np.sqrt(n)))
    hcur = resize_kernel(current, ksize).ravel()
    e0 = energy(G, hcur)
    mu = ridge * np.trace(G[:n, :n]) / n
    A = G[:n, :n] + mu * np.eye(n)
    rhs = G[:n, n] + mu * hcur
    # the pivots of A = L L^T, and the library's no-texture test
    Lc, piv = np.zeros((n, n)), []
    for j in range(n):
        p = A[j, j] - np.dot(Lc[j, :j], Lc[j, :j])
        if not (A[j, j] > 0.0 and p > PIVOT_RTOL * A[j, j]):
            return hcur.reshape(ksize, ksize), np.array([e0, e0, 0.0, 0.0, STATUS_NO_TEXTURE])
        piv.append(p)
        Lc[j, j] = np.sqrt(p)
        for i in range(j + 1, n):
            Lc[i, j] = (A[i, j] - np.dot(Lc[i, :j], Lc[j, :j])) / Lc[j, j]
    if sum_to_one:
        Kkt = np.zeros((n + 1, n + 1))
        Kkt[:n, :n] = A
        Kkt[:n, n] = Kkt[n, :n] = 1.0
        h = np.linalg.solve(Kkt, np.concatenate([rhs, [1.0]]))[:n]
    else:
        h = np.linalg.solve(A, rhs)
    return h.reshape(ksize, ksize), np.array([e0, energy(G, h), min(piv), max(piv), STATUS_OK])


def fit_blur(x, y, w, motion, ksize, s, current, sum_to_one=True, ridge=0.0, order="natural"):
    G = gram(x, y, w, motion, ksize, s, order)
    taps, q = solve_taps(G, current, sum_to_one, ridge)
    return taps, q, pack(G)


# ------------------------------------------------------------------------------------------- kernels and inputs
def gaussian_taps(ksize, sigma):
    return orc.gaussian_kernel(ksize, sigma)[1] if (ksize > 0 and sigma > 0) else np.ones((1, 1))


def anisotropic_psf(ksize=5, sigma_u=1.5, sigma_v=0.7, angle=0.5):
    """A Gaussian with standard deviations (sigma_u, sigma_v) along axes rotated by `angle` radians, normalised to sum 1."""
    hb = (ksize - 1) // 2
    yy, xx = np.meshgrid(np.arange(-hb, hb + 1, dtype=np.float64), np.arange(-hb, hb + 1, dtype=np.float64), indexing="ij")
    u = np.cos(angle) * xx + np.sin(angle) * yy
    v = -np.sin(angle) * xx + np.cos(angle) * yy
    k = np.exp(-0.5 * ((u / sigma_u) ** 2 + (v / sigma_v) ** 2))
    return k / k.sum()


def streak_psf(ksize=5):
    """A one-sided horizontal motion streak: the centre and the taps to its right, decaying; nothing like symmetric."""
    k = np.zeros((ksize, ksize))
    hb = (ksize - 1) // 2
    k[hb, hb:] = 0.5 ** np.arange(ksize - hb)
    return k / k.sum()


def second_scene(C, H, W):
    """Another ground truth on the table's geometry: bars, a ramp and a disc elsewhere."""
    v, u = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    base = 0.45 + 0.2 * np.sign(np.sin(2 * np.pi * 5 * (u + 0.3 * v))) * (v > 0.5) + 0.3 * u * (v <= 0.5) \
        + 0.25 * ((u - .3) ** 2 + (v - .35) ** 2 < .02)
    return np.stack([np.clip(base * (0.7 + 0.3 * c / max(1, C - 1)), 0, 1) for c in range(C)])


def table_inputs():
    """The robust table's geometry (96 x 128 HR, scale 2, 6 frames, noise sigma 0.01, BTV(2, 0.5) lambda 0.005) with the
    sub-pixel shifts of the affine table and the rotated anisotropic 5 x 5 PSF as the true blur.  Two scenes: the
    calibration pair (the prototype ground truth and its frames) and a second scene to solve."""
    C, H, W, s, K = 1, 96, 128, 2, 6
    shifts = ar.TABLE_SHIFTS
    motion = ("shifts", shifts)
    psf = anisotropic_psf()
    truth = BlurKernelModel(s, K, H, W, psf, motion)
    out = dict(C=C, H=H, W=W, s=s, K=K, shifts=shifts, motion=motion, psf=psf, guess=(3, 1.0), reg=(orc.REG_BTV, 0.005, 2, 0.5),
               truth=truth, scenes={})
    for name, gt, seed in (("calibration", rr.prototype_ground_truth(C, H, W), 7), ("second", second_scene(C, H, W), 11)):
        clean = np.stack([truth.apply(gt, k) for k in range(K)])
        y = clean + 0.01 * np.random.default_rng(seed).standard_normal(clean.shape)
        out["scenes"][name] = (gt, clean, y)
    return out
