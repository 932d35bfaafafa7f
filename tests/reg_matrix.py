"""The covering matrix of the direct regulariser kernels (csrc/kernels_reg_direct.hip): every values, IRLS-weights and
gradient variant at the edges of its dispatch rule.  Shared by tests/test_gpu_reg_kernels.py (HIP against the oracle)
and tests/test_reg_matrix_cpu.py (the rule mirror reaches every cell; the bars of tests/error_bars.py catch planted bugs).

The mirror restates the three launchers:
  launch_btv_values4 / launch_reg_values / launch_reg_weights (values and weights, `values_kernel`):
    BTV, R = 3, W % 4 == 0, H >= 16            k_btv_values_strip<T, 3, 4>: strips of 4 rows, 4 columns per thread
    BTV, R in 1..3, W % 4 == 0, otherwise      k_btv_values4<T, R>
    anything else                              k_reg_values<T>
  launch_reg_gradient_direct (`grad_kernel`; eval passes no values for TV kinds, srmap_reg_values_and_gradient does):
    TV3D, no values, C >= 2, W % 4 == 0        k_tv3d_march<T>, channels in chunks of `march_chunk`
    TV / TV3D, no values, otherwise            k_tv_onepass<T, D3>: 256 columns x 4 rows per block; its unmasked path
                                               needs W % 4 == 0 and an interior row
    BTV, or values supplied                    k_reg_gradient_direct<T>
Kinds follow srmap.h: 0 TV, 1 TV3D, 2 BTV.
"""
import numpy as np

TV, TV3D, BTV = 0, 1, 2
STRIP_ROWS = 4  # kBtvStripRows


def cdiv(a, b):
    return -(-a // b)


def values_kernel(kind, R, C, H, W):
    """The kernel that computes regulariser values (and IRLS weights) for this geometry."""
    if kind == BTV and 1 <= R <= 3 and W % 4 == 0:
        if R == 3 and H >= 4 * STRIP_ROWS:
            return "strip"
        return "values4_R%d" % R
    return "reg_values"


def march_chunk(C, H, W):
    """k_tv3d_march's channels per thread: halve while the grid would have fewer than 4096 blocks."""
    per_plane = cdiv(W, 256) * cdiv(H, 4)
    chunk = C
    while chunk > 16 and per_plane * cdiv(C, chunk) < 4096:
        chunk = cdiv(chunk, 2)
    return chunk


def march_chunks(C, H, W):
    """[(first channel, length)] of every chunk."""
    ch = march_chunk(C, H, W)
    return [(c, min(ch, C - c)) for c in range(0, C, ch)]


def grad_kernel(kind, C, H, W, with_values):
    if kind != BTV and not with_values:
        if kind == TV3D and C >= 2 and W % 4 == 0:
            return "march"
        return "onepass3d" if kind == TV3D else "onepass2d"
    return "reg_gradient_direct"


def onepass_paths(H, W):
    """The k_tv_onepass paths the rows of this geometry take: 'fast' (W % 4 == 0, rows 1 .. H-2), 'masked' (the rest)."""
    fast_rows = max(0, H - 2) if W % 4 == 0 else 0
    return ({"fast"} if fast_rows else set()) | ({"masked"} if fast_rows < H else set())


# ---- values / IRLS-weights cells: (kind, R, decay, C, H, W) ----
# strip: H = 16..19 and one taller H per residue mod 4 (the last strip whole, or 1-3 rows: the masked path);
# W / 4 in {1, 3, 16, 63, 64, 65} cells: a wave of only row-final cells, rows of 3 or 16 cells (every wave mixes row-final
# and interior cells), 63 / 64 / 65 cells (a wave ends at, just before or just after a row's end)
STRIP = [(BTV, 3, d, C, H, W) for d, C, H, W in (
    (0.5, 1, 16, 4), (1.0, 1, 17, 12), (0.5, 2, 18, 64), (1.0, 1, 19, 252),
    (0.5, 1, 36, 256), (1.0, 1, 41, 260), (0.5, 1, 46, 12), (1.0, 2, 51, 64),
    (0.5, 1, 23, 260), (1.0, 1, 20, 4))]
# values4: R = 1, 2 on both sides of H = 16, R = 3 below it
VALUES4 = [(BTV, R, d, C, H, W) for R, d, C, H, W in (
    (1, 0.5, 1, 15, 8), (1, 1.0, 2, 17, 260), (1, 0.5, 1, 1, 4),
    (2, 1.0, 1, 3, 12), (2, 0.5, 1, 16, 256), (2, 0.5, 2, 19, 4),
    (3, 0.5, 1, 15, 4), (3, 1.0, 1, 15, 256), (3, 0.5, 2, 7, 260), (3, 0.5, 1, 1, 12))]
# k_reg_values: W % 4 in {1, 2, 3} for BTV R = 1..3, BTV R = 4 (any W), TV, TV3D
REG_VALUES = [(BTV, 1, 0.5, 1, 9, 5), (BTV, 2, 1.0, 2, 17, 6), (BTV, 3, 0.5, 1, 19, 7), (BTV, 3, 1.0, 1, 16, 257),
              (BTV, 4, 0.5, 1, 18, 8), (BTV, 4, 1.0, 2, 5, 255),
              (TV, 0, 0.0, 1, 5, 9), (TV, 0, 0.0, 2, 16, 256),
              (TV3D, 0, 0.0, 3, 6, 12), (TV3D, 0, 0.0, 1, 4, 7)]
VALUE_CELLS = STRIP + VALUES4 + REG_VALUES

# ---- gradient cells under eval (no values for TV kinds): (kind, R, decay, C, H, W) ----
# march: C = 2, 3, 4, 17, 40, 50 on small planes (chunk and last-chunk lengths 0, 1 and 2 mod 3), C = 20 on a plane of
# 4096 row blocks (no halving); H mod 4 in {0..3}; W in {4, 252, 256, 260}
MARCH = [(TV3D, 0, 0.0, C, H, W) for C, H, W in (
    (2, 5, 4), (3, 6, 252), (4, 7, 256), (17, 8, 260), (40, 9, 4), (50, 10, 252), (17, 4, 256), (20, 16384, 4))]
# onepass: TV / TV3D masked (W % 4 != 0, or border rows), the fast path (W % 4 == 0; TV3D with C = 1), H = 1..5,
# W in {1, 255, 257} and the 256-column block edge
ONEPASS = [(TV, 0, 0.0, C, H, W) for C, H, W in (
    (1, 1, 1), (2, 2, 255), (1, 3, 257), (2, 4, 1), (1, 5, 255), (1, 5, 256), (2, 7, 260), (1, 6, 512))] + \
    [(TV3D, 0, 0.0, C, H, W) for C, H, W in (
        (3, 2, 257), (2, 5, 255), (4, 3, 1), (2, 1, 9), (1, 5, 256), (1, 8, 260))]
# k_reg_gradient_direct: BTV R = 1..4 at ragged W / H (the values go through every values kernel on the way)
BTV_GRAD = [(BTV, R, d, C, H, W) for R, d, C, H, W in (
    (1, 0.5, 1, 5, 5), (1, 1.0, 2, 3, 257), (2, 0.5, 1, 17, 13), (2, 1.0, 2, 2, 255),
    (3, 0.5, 1, 16, 17), (3, 1.0, 1, 19, 6), (3, 0.5, 2, 18, 260), (4, 0.5, 2, 5, 257), (4, 1.0, 1, 18, 7),
    (4, 0.5, 1, 1, 1))]
GRAD_CELLS = MARCH + ONEPASS + BTV_GRAD


def cell_id(cell):
    kind, R, d, C, H, W = cell
    name = {TV: "tv", TV3D: "tv3d", BTV: "btv%d" % R}[kind]
    return "%s-d%g-C%dH%dW%d" % (name, d, C, H, W)


def weights_input(rng, C, H, W):
    """An x to build IRLS weights from, in 4 x 4 patches: flat (r = 0, the clamp), steps of 2^-16 or 2^-17 on a random
    base (r on both sides of 1e-5), or k/64 noise.  Every value is a multiple of 2^-17 in [0, 1 + 2^-16]: exact in f32,
    with exact differences."""
    hp, wp = cdiv(H, 4), cdiv(W, 4)
    kind = rng.integers(0, 4, size=(C, hp, wp)).repeat(4, 1).repeat(4, 2)[:, :H, :W]
    base = (rng.integers(0, 65, size=(C, hp, wp)) / 64.0).repeat(4, 1).repeat(4, 2)[:, :H, :W]
    bit = rng.integers(0, 2, size=(C, H, W))
    fine = np.where(kind == 1, bit * 2.0 ** -16, np.where(kind == 2, bit * 2.0 ** -17, 0.0))
    return np.where(kind == 3, rng.integers(0, 65, size=(C, H, W)) / 64.0, base + fine)
