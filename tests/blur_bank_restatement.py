"""numpy / scipy.sparse restatement of the blur-kernel bank and of its per-entry calibration fit (include/srmap.h:
srmap_problem_set_blur_bank, srmap_fit_blur_bank) -- the checker of tests/test_blur_bank_cpu.py and
tests/test_gpu_blur_bank.py, written from the definition on top of blur_kernel_restatement (D, B, M_k of a translation or
an affine matrix), flow_restatement (M_k of a displacement field) and robust_restatement (the weighted data term, the solve).

  forward    A_{k,c} = D B_{k,c} M_k as explicit sparse matrices, B_{k,c} the literal correlation with entry (k, c) of the
             bank: entry k (per frame), c (per channel) or k * C + c (per frame and channel);
  adjoint    the literal transposes A_{k,c}^T (scipy's .T);
  fit        per entry the Gram S.T @ (w * S) of [s_0 ... s_{n-1}, y] over the entry's observations -- frames, then channels,
             in index order -- and blur_kernel_restatement's KKT solve; gram_sensitivity() reports what a second
             evaluation with the observations permuted changes: the restatement's own summation-order sensitivity.
"""
import os
import sys

import numpy as np

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import blur_kernel_restatement as bk  # noqa: E402
import flow_restatement as fr  # noqa: E402
import robust_restatement as rr  # noqa: E402

PER_FRAME, PER_CHANNEL, PER_FRAME_CHANNEL = 1, 2, 3
MODES = {"frame": PER_FRAME, "channel": PER_CHANNEL, "frame_channel": PER_FRAME_CHANNEL}


def entries(mode, K, C):
    return {PER_FRAME: K, PER_CHANNEL: C, PER_FRAME_CHANNEL: K * C}[mode]


def entry_of(mode, C, k, c):
    return {PER_FRAME: k, PER_CHANNEL: c, PER_FRAME_CHANNEL: k * C + c}[mode]


def members(mode, K, C, e):
    """The (frame, channel) pairs of entry e, frames then channels in index order."""
    return [(k, c) for k in range(K) for c in range(C) if entry_of(mode, C, k, c) == e]


def flat_bank(bank, mode, K, C):
    """The bank as [entries][b][b] (a per-(frame, channel) bank may come as [K][C][b][b])."""
    bank = np.asarray(bank, dtype=np.float64)
    b = bank.shape[-1]
    out = bank.reshape(-1, b, b)
    assert out.shape[0] == entries(mode, K, C) and bank.shape[-2] == b and b % 2 == 1, bank.shape
    return out


def warp_matrix(motion, k, W, H):
    """motion: None, ("shifts", [K][2]), ("affine", [K][2][3]) or ("flow", [K][2][H][W] as the library stores it)."""
    if motion is not None and motion[0] == "flow":
        return fr.warp_matrix(np.asarray(motion[1], dtype=np.float64)[k], W, H)
    return bk.warp_matrix(motion, k, W, H)


# ------------------------------------------------------------------------------------------- the model
class BlurBankModel(orc.ImageModel):
    """A_{k,c} = D B_{k,c} M_k; apply / apply_transpose over the problem's C channels as orc.ImageModel has them."""

    def __init__(self, scale, K, C, H, W, bank, mode, motion=None):
        super().__init__(scale, None, 0, 0.0, num_frames=K)
        self.H, self.W, self.K, self.C, self.mode = H, W, K, C, mode
        self.bank = flat_bank(bank, mode, K, C)
        self.motion = motion
        self.D, self.rmap, self.cmap = bk.decimation_matrix(H, W, scale)
        self.h, self.w = len(self.rmap), len(self.cmap)
        self.B = [bk.blur_matrix(t, H, W) for t in self.bank]
        self.Mk = [warp_matrix(motion, k, W, H) for k in range(K)]
        self.A = [[(self.D @ self.B[entry_of(mode, C, k, c)] @ self.Mk[k]).tocsr() for c in range(C)] for k in range(K)]
        self.At = [[A.T.tocsr() for A in row] for row in self.A]

    def apply(self, hr, k):
        x = np.ascontiguousarray(hr, dtype=np.float64)
        assert x.shape[0] == self.C
        return np.stack([(self.A[k][c] @ x[c].ravel()).reshape(self.h, self.w) for c in range(self.C)])

    def apply_transpose(self, lr, k):
        u = np.ascontiguousarray(lr, dtype=np.float64)
        assert u.shape[0] == self.C
        return np.stack([(self.At[k][c] @ u[c].ravel()).reshape(self.H, self.W) for c in range(self.C)])

    def data_term(self, y, w, x, want_grad=True, cost_rows=None):
        return rr.weighted_data_term(self, y, w, x, want_grad, cost_rows)


# ------------------------------------------------------------------------------------------- the fit
def bank_gram(x, y, w, motion, ksize, s, mode, order="natural"):
    """[entries][n + 1][n + 1]: per entry the Gram of [s_0 ... s_{n-1}, y] under w over the entry's observations; y, w
    [K][C][h][w] (w None = ones).  order "permuted": members and observations reversed (the sensitivity probe)."""
    y = np.asarray(y, dtype=np.float64)
    K, C, h, wd = y.shape
    n = ksize * ksize
    cols = [bk.fit_columns(x, motion, k, ksize, s).reshape(C, h * wd, n) for k in range(K)]
    out = np.zeros((entries(mode, K, C), n + 1, n + 1))
    for e in range(out.shape[0]):
        mem = members(mode, K, C, e)
        for k, c in (mem if order == "natural" else mem[::-1]):
            S = np.concatenate([cols[k][c], y[k, c].reshape(-1, 1)], axis=1)
            wk = np.ones(S.shape[0]) if w is None else np.asarray(w[k][c], dtype=np.float64).reshape(-1)
            if order != "natural":
                S, wk = S[::-1], wk[::-1]
            out[e] += S.T @ (wk[:, None] * S)
    return out


def gram_sensitivity(x, y, w, motion, ksize, s, mode):
    """(Grams in the natural order, per entry the largest change of the G / b / y.y block under the permuted order)."""
    n = ksize * ksize
    G, P = bank_gram(x, y, w, motion, ksize, s, mode), bank_gram(x, y, w, motion, ksize, s, mode, "permuted")
    blocks = ((slice(0, n), slice(0, n)), (slice(0, n), slice(n, n + 1)), (slice(n, n + 1), slice(n, n + 1)))
    return G, np.array([[np.max(np.abs(G[e][sl] - P[e][sl])) for sl in blocks] for e in range(G.shape[0])])


def current_entries(current, mode, K, C):
    """The kernel in force per entry of `mode`: current is one kernel [b][b], or (mode_in_force, bank)."""
    if isinstance(current, tuple):
        cm, cb = current
        cb = flat_bank(cb, cm, K, C)
        rep = {PER_FRAME: lambda e: (e, 0), PER_CHANNEL: lambda e: (0, e), PER_FRAME_CHANNEL: lambda e: divmod(e, C)}[mode]
        return [cb[entry_of(cm, C, *rep(e))] for e in range(entries(mode, K, C))]
    return [np.asarray(current, dtype=np.float64)] * entries(mode, K, C)


def fit_bank(x, y, w, motion, ksize, s, mode, current, sum_to_one=True, ridge=0.0, order="natural"):
    """(taps [entries][ksize][ksize], quality [entries][5], packed sums [entries][(n + 1)(n + 2) / 2])."""
    K, C = np.asarray(y).shape[:2]
    G = bank_gram(x, y, w, motion, ksize, s, mode, order)
    cur = current_entries(current, mode, K, C)
    fits = [bk.solve_taps(G[e], cur[e], sum_to_one, ridge) for e in range(G.shape[0])]
    return np.stack([f[0] for f in fits]), np.stack([f[1] for f in fits]), np.stack([bk.pack(g) for g in G])


# ------------------------------------------------------------------------------------------- kernels and inputs
def pad(taps, ksize):
    return bk.resize_kernel(taps, ksize)


def streak(angle_deg, taps=5, ksize=5):
    """A centred motion streak of `taps` taps along 0, 45 or 90 degrees inside ksize x ksize, normalised to sum 1."""
    k = np.zeros((ksize, ksize))
    hb, r = (ksize - 1) // 2, (taps - 1) // 2
    dy, dx = {0: (0, 1), 45: (-1, 1), 90: (1, 0)}[angle_deg]
    for t in range(-r, r + 1):
        k[hb + t * dy, hb + t * dx] = 1.0
    return k / k.sum()


def table_bank():
    """The per-frame bank of the table: frames 0, 2, 4 the 3 x 3 Gaussian sigma 1 (zero-padded to 5 x 5), frames 1, 3, 5
    five-tap streaks at 0, 45 and 90 degrees."""
    g = pad(bk.gaussian_taps(3, 1.0), 5)
    return np.stack([g, streak(0), g, streak(45), g, streak(90)])


def table_inputs():
    """The robust table's input (96 x 128 HR, scale 2, 6 frames with the affine table's sub-pixel shifts, noise sigma 0.01,
    BTV(2, 0.5) lambda 0.005), the frames generated under table_bank().  Two scenes: the calibration pair and a second
    scene to solve."""
    C, H, W, s, K = 1, 96, 128, 2, 6
    shifts = ar.TABLE_SHIFTS
    motion = ("shifts", shifts)
    bank = table_bank()
    truth = BlurBankModel(s, K, C, H, W, bank, PER_FRAME, motion)
    out = dict(C=C, H=H, W=W, s=s, K=K, shifts=shifts, motion=motion, bank=bank, mode=PER_FRAME, guess=(3, 1.0),
               reg=(orc.REG_BTV, 0.005, 2, 0.5), truth=truth, scenes={})
    for name, gt, seed in (("calibration", rr.prototype_ground_truth(C, H, W), 7), ("second", bk.second_scene(C, H, W), 11)):
        clean = np.stack([truth.apply(gt, k) for k in range(K)])
        y = clean + 0.01 * np.random.default_rng(seed).standard_normal(clean.shape)
        out["scenes"][name] = (gt, clean, y)
    return out


SOLVE_CAPS = (5, 20)  # IRLS rounds, CG iterations per round: DESIGN.md 3.9's caps


def solve_scene(table, scene, bank=None, taps=None):
    """(PSNR, (rounds, iterations, evaluations)) of the capped L2 solve of a scene under a per-frame bank or one kernel."""
    gt, _, y = table["scenes"][scene]
    if bank is not None:
        model = BlurBankModel(table["s"], table["K"], table["C"], table["H"], table["W"], bank, PER_FRAME, table["motion"])
    else:
        model = bk.BlurKernelModel(table["s"], table["K"], table["H"], table["W"], taps, table["motion"])
    o = orc.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = SOLVE_CAPS
    x, rep, _ = rr.irls_solve(model, y, rr.bilinear(y[0], table["s"]), reg=table["reg"], composed=True, options=o)
    return orc.psnr(gt, x), (rep.irls_rounds, rep.cg_iterations, rep.nfev)
