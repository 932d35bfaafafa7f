"""The covering matrix of the tile path (csrc/kernels_ztile.hip, the sequence eval_ztile of csrc/eval.hip): every instance of k_eval_z at the
ragged right / bottom edges it has to handle.  Shared by tests/test_gpu_tile_edges.py (HIP against the oracle) and
tests/test_error_bars_cpu.py (the bars of tests/error_bars.py catch plausible kernel bugs on the same geometries).

A tile is 64 LR cells (64 S HR columns) by 8 HR rows (ztile_dev.hpp ZCfg).  Per (S, regulariser leg) four geometries:
  w mod 64 in {0, 1, 2, 63} LR cells (W mod 64 S in {0, S, 2 S, 64 S - S} HR pixels), 1 and 2 column tiles;
  H mod 8 in {0, 1, R, 7}, rounded to the residues a multiple of S can have (S = 2: even, S = 4: {0, 4});
  one geometry without motion reach (E = 0, the fewest rows the plan accepts: 1 row tile at S = 2), three with shifts of
  every one of the S^2 phases, both signs and +-E in both axes (E = S), one of them with two channels (obs_c0 offsets).
"""
import numpy as np

LEGS = {  # name: (kind, range) -- kind 0 TV, 2 BTV; None: no in-kernel regulariser
    "none": None, "tv": (0, 0), "btv1": (2, 1), "btv2": (2, 2), "btv3": (2, 3)}
SCALES = (2, 3, 4)
BLURS = (1, 3)


def leg_reach(leg):
    """How far the leg's pass 1 reaches down (ZCfg WIN): the H mod 8 residue that puts the bottom tile inside it."""
    spec = LEGS[leg]
    return 2 if spec is None else (1 if spec[0] == 0 else spec[1])


def rows_with_residue(S, t, hmin, used=()):
    """Smallest h >= hmin whose H = h S has H mod 8 closest to t (circularly) among the residues a multiple of S has and
    `used` does not hold yet (all of them once none is left); on a tie the residue further into the tile for t <= 4,
    nearer its start above (t = 1 -> 2, t = 7 -> 6 at S = 2)."""
    have = sorted({(h * S) % 8 for h in range(8)})
    have = [r for r in have if r not in used] or have
    best = min(have, key=lambda r: (min((r - t) % 8, (t - r) % 8), (r - t) % 8 if t <= 4 else (t - r) % 8))
    h = hmin
    while (h * S) % 8 != best:
        h += 1
    return h


def phase_shifts(S, E, rng):
    """Integer shifts covering every (dx mod S, dy mod S) phase with both signs, plus (E, -E), (-E, E), (E, E), (0, 0)."""
    out = [[0, 0], [E, -E], [-E, E], [E, E], [-E, -E]]
    for a in range(S):
        for b in range(S):
            dx = a if rng.random() < 0.5 else a - S
            dy = b if rng.random() < 0.5 else b - S
            out.append([int(dx), int(dy)])
    return out


def geometries(S, leg):
    """[(W, H, C, shifts, decay)] for one (S, leg)."""
    rng = np.random.default_rng(31 * S + list(LEGS).index(leg))
    reach = leg_reach(leg)
    E = S
    hmin = (4 * E + 2 * S) // S + 1          # H > 4E + 2S (the integer plan's border frame)
    out = []
    # E = 0: only the (0, 0) phase; the shortest image the plan takes (H > 2S)
    h0 = (2 * S) // S + 1
    out.append((64 * S, rows_with_residue(S, 0, h0) * S, 1, [[0, 0], [0, 0]], 0.5))
    for w, t, C, decay in ((65, 1, 1, 0.625), (66, reach, 2, 0.5), (63, 7, 1, 0.625)):
        h = rows_with_residue(S, t, hmin, {g[1] % 8 for g in out})
        out.append((w * S, h * S, C, phase_shifts(S, E, rng), decay))
    return out


def matrix():
    """[(S, B, leg, index, geometry)] over every (S, B, leg) instance of the tile kernel (dtype is a separate axis)."""
    return [(S, B, leg, i, geo) for S in SCALES for B in BLURS for leg in LEGS for i, geo in enumerate(geometries(S, leg))]


def geo_id(S, B, leg, i, geo):
    W, H, C = geo[:3]
    return "S%d-B%d-%s-g%d-W%dH%dC%d" % (S, B, leg, i, W, H, C)


def regs_of(leg, decay):
    """[(kind, lam, R, decay)] of the leg, lambda = 2^-6."""
    spec = LEGS[leg]
    if spec is None:
        return []
    kind, R = spec
    return [(kind, 2.0 ** -6, R, decay if kind == 2 else 0.0)]
