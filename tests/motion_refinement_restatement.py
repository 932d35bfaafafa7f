"""numpy restatement of the joint motion refinement (include/srmap.h: srmap_refine_motion) -- the checker of
tests/test_motion_refinement_cpu.py and tests/test_gpu_motion_refinement.py, written from the definition, not from the kernel.

With an HR estimate x [C][H][W], frame k's matrix F_k (affine_restatement's convention) is re-fitted through the forward model:

  energy     E(G) = sum_c sum_u w(c,u) r^2,  r = (D B M(G) x)(c,u) - y(c,u),  G = F^-1 (affine_restatement.inverse_map)
  sample     s = G(q) for every HR-grid pixel q (affine_restatement.source_coords: a x + (b y + t), each operation rounded);
             four taps v00 v01 v10 v11 (taps outside the image are 0), fx, fy the fractions:
             value = (1-fy)((1-fx) v00 + fx v01) + fy((1-fx) v10 + fx v11)
             gx    = (1-fy)(v01 - v00) + fy(v11 - v10)         d value / d s_x, exact inside a cell
             gy    = (1-fx)(v10 - v00) + fx(v11 - v01)         d value / d s_y
  increment  G <- G + dL (q - c0) + dt, c0 = ((W-1)/2, (H-1)/2), parameters (da, db, dtx, dc, dd, dty):
             J = D B of the six HR-grid images gx (qx-c0x), gx (qy-c0y), gx, gy (qx-c0x), gy (qy-c0y), gy
  sums       H = sum w J J^T (21 entries, upper triangle row-major), g = sum w J r (6), E: 28 numbers
  LM         (H + lambda diag H) d = -g by affine_registration_restatement.cholesky_solve (dof 2: indices (2, 5)); E' < E accepts.

D B is stated here with explicit taps (zero border, then every s-th pixel) so that an f32 problem's f32-rounded taps can be
given; with the oracle's Gaussian taps it IS the oracle's D B (tests/test_motion_refinement_cpu.py checks that).
"""
import os
import sys

import numpy as np

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import affine_registration_restatement as rg  # noqa: E402

SUMS = 28
MIN_DAMPING, MAX_DAMPING = 1e-9, 1e6
STATUS_CONVERGED, STATUS_ITERATIONS, STATUS_DAMPING, STATUS_NO_TEXTURE = 0, 1, 2, 3


def blur_taps(blur_ksize, blur_sigma, f32=False):
    """The b x b taps of B ([[1]] without a blur); f32: rounded as an f32 problem stores them."""
    k2 = orc.gaussian_kernel(blur_ksize, blur_sigma)[1] if (blur_ksize > 0 and blur_sigma > 0) else np.ones((1, 1))
    return k2.astype(np.float32).astype(np.float64) if f32 else k2


def blur_decimate(planes, taps, s):
    """D B of HR-grid planes [n][H][W] -> [n][H // s][W // s]: filter2D with a zero border, taps in row-major order, then
    the pixels (s i, s j)."""
    n, H, W = planes.shape
    b = taps.shape[0]
    hb = (b - 1) // 2
    h, w = H // s, W // s
    P = np.zeros((n, H + 2 * hb, W + 2 * hb))
    P[:, hb:hb + H, hb:hb + W] = planes
    out = np.zeros((n, h, w))
    for a in range(b):
        for e in range(b):
            out += taps[a, e] * P[:, a:a + s * h:s, e:e + s * w:s]
    return out


def sample_with_derivatives(x, G):
    """(value, gx, gy), each [C][H][W], of the four-tap sample of x at s = G(q) for every HR-grid pixel q."""
    C, H, W = x.shape
    qy, qx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    sx, sy = ar.source_coords(np.asarray(G, dtype=np.float64).reshape(2, 3), qx, qy)
    with np.errstate(invalid="ignore"):
        inside = (sx > -1.0) & (sx < W) & (sy > -1.0) & (sy < H)
    sx, sy = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    P = np.zeros((C, H + 2, W + 2))  # one pixel of zero border: tap (r, c) sits at P[r + 1, c + 1]
    P[:, 1:-1, 1:-1] = x
    v00, v01 = P[:, y0 + 1, x0 + 1], P[:, y0 + 1, x0 + 2]
    v10, v11 = P[:, y0 + 2, x0 + 1], P[:, y0 + 2, x0 + 2]
    m = inside.astype(np.float64)
    val = m * ((1 - fy) * ((1 - fx) * v00 + fx * v01) + fy * ((1 - fx) * v10 + fx * v11))
    gx = m * ((1 - fy) * (v01 - v00) + fy * (v11 - v10))
    gy = m * ((1 - fx) * (v10 - v00) + fx * (v11 - v01))
    return val, gx, gy, (sx, sy, inside)


def model_and_jacobian(x, G, taps, s):
    """(D B M(G) x [C][h][w], J [6][C][h][w])."""
    C, H, W = x.shape
    val, gx, gy, _ = sample_with_derivatives(x, G)
    qy, qx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, v = qx - (W - 1) / 2.0, qy - (H - 1) / 2.0
    planes = np.concatenate([val, gx * u, gx * v, gx, gy * u, gy * v, gy])
    out = blur_decimate(planes, taps, s)
    return out[:C], out[C:].reshape(6, C, out.shape[1], out.shape[2])


def _total(a, order):
    """Sum of [C][h][w], the planes in order, each by rg._total's orders."""
    return float(sum(rg._total(a[c], order) for c in range(a.shape[0])))


def refine_sums(x, y, w, G, taps, s, order="rows"):
    """The 28 sums of one pass of one frame: y, w [C][h][w] (w None = ones)."""
    m, J = model_and_jacobian(np.asarray(x, dtype=np.float64), G, taps, s)
    r = m - y
    wv = np.ones_like(r) if w is None else w
    S = np.zeros(SUMS)
    q = 0
    for a in range(6):
        wj = wv * J[a]
        for e in range(a, 6):
            S[q] = _total(wj * J[e], order)
            q += 1
        S[21 + a] = _total(wj * r, order)
    S[27] = _total((wv * r) * r, order)
    return S


def unpack(S):
    H = np.zeros((6, 6))
    q = 0
    for a in range(6):
        for e in range(a, 6):
            H[a, e] = H[e, a] = S[q]
            q += 1
    return H, S[21:27].copy(), float(S[27])


def lm_step(S, lam, dof):
    """d [6] of (H + lambda diag H) d = -g over the dof's parameters, or None (no texture)."""
    H, g, _ = unpack(S)
    idx = [2, 5] if dof == 2 else list(range(6))
    A = H[np.ix_(idx, idx)].copy()
    for i in range(len(idx)):
        A[i, i] = A[i, i] + lam * A[i, i]
    sol = rg.cholesky_solve(A, -g[idx])
    if sol is None:
        return None
    d = np.zeros(6)
    d[idx] = sol
    return d


def increment(G, d, W, H):
    c0x, c0y = (W - 1) / 2.0, (H - 1) / 2.0
    G = np.asarray(G, dtype=np.float64).reshape(2, 3)
    return np.array([[G[0, 0] + d[0], G[0, 1] + d[1], G[0, 2] + (d[2] - (d[0] * c0x + d[1] * c0y))],
                     [G[1, 0] + d[3], G[1, 1] + d[4], G[1, 2] + (d[5] - (d[3] * c0x + d[4] * c0y))]])


def refine_frame(x, y, w, F0, taps, s, dof=6, max_iterations=30, step_tolerance=1e-4, initial_damping=1e-3, order="rows"):
    """(F, quality [4] = E at the start, E at the result, passes, status, sums [28] at F, decisions) of one frame;
    decisions: one (accepted, E_trial, E_current) per trial pass."""
    x = np.asarray(x, dtype=np.float64)
    _, Hh, Ww = x.shape
    F = np.array(F0, dtype=np.float64).reshape(2, 3)
    G = ar.inverse_map(F)
    S = refine_sums(x, y, w, G, taps, s, order)
    e0, passes, lam, status, decisions = S[27], 1, initial_damping, None, []
    while status is None:
        # the next trial; rejections that need no pass are taken here
        if passes - 1 >= max_iterations:
            status = STATUS_ITERATIONS
            break
        d = lm_step(S, lam, dof)
        if d is None:
            status = STATUS_NO_TEXTURE
            break
        Gt = increment(G, d, Ww, Hh)
        with np.errstate(all="ignore"):
            Ft = ar.inverse_map(Gt)
        if dof == 2:
            Ft[:, :2] = F[:, :2]
        if not (np.all(np.isfinite(Gt)) and np.all(np.isfinite(Ft)) and ar.deviation(Ft) <= ar.MAX_DEVIATION):
            lam *= 10.0
            if lam > MAX_DAMPING:
                status = STATUS_DAMPING
            continue
        St = refine_sums(x, y, w, Gt, taps, s, order)
        passes += 1
        accepted = bool(St[27] < S[27])
        decisions.append((accepted, float(St[27]), float(S[27])))
        if accepted:
            step = rg.corner_displacement(F, Ft, Ww, Hh)
            G, F, S = Gt, Ft, St
            lam = max(lam / 10.0, MIN_DAMPING)
            if step < step_tolerance:
                status = STATUS_CONVERGED
        else:
            lam *= 10.0
            if lam > MAX_DAMPING:
                status = STATUS_DAMPING
    return F, np.array([e0, S[27], passes, status]), S, decisions


def refine_motion(x, y, w, F0, taps, s, with_decisions=False, **kw):
    """All frames: y, w [K][C][h][w] (w None = ones), F0 [K][2][3].  Frame 0 is the gauge: (cost, cost, 0, 0).
    Returns (matrices [K][2][3], quality [K][4], sums [K][28]) (+ the decisions per frame)."""
    K = y.shape[0]
    F0 = np.asarray(F0, dtype=np.float64).reshape(K, 2, 3)
    mats, quality, sums, dec = F0.copy(), np.zeros((K, 4)), np.zeros((K, SUMS)), [[] for _ in range(K)]
    for k in range(K):
        wk = None if w is None else w[k]
        if k == 0:
            sums[0] = refine_sums(np.asarray(x, dtype=np.float64), y[0], wk, ar.inverse_map(F0[0]), taps, s, kw.get("order", "rows"))
            quality[0] = [sums[0, 27], sums[0, 27], 0, 0]
            continue
        mats[k], quality[k], sums[k], dec[k] = refine_frame(x, y[k], wk, F0[k], taps, s, **kw)
    return (mats, quality, sums, dec) if with_decisions else (mats, quality, sums)


def min_margin(decisions):
    """Smallest relative cost margin |E' - E| / E over the accept / reject decisions of refine_motion (inf if none)."""
    m = [abs(et - ec) / ec for frame in decisions for _, et, ec in frame if ec > 0]
    return min(m) if m else float("inf")
