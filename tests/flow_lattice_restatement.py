"""numpy restatement of the displacement field on a control lattice (include/srmap.h: srmap_problem_set_flow_lattice;
LatticeField of csrc/sample_dev.hpp), written from the header's statement of the rule, and the lattices the GPU tests use.

A lattice has `step` HR pixels between nodes and lw x lh nodes per component; node (i, j) sits at HR pixel (i step, j step).
u at the HR pixel (x, y) is the bilinear interpolant of the nodes at (x, y) / step clamped to the lattice, in double, in the
order of flow_registration_restatement.resample (sub = 0, div = step, gain = 1), rounded once to the problem's dtype.  From
u on the model is flow_restatement's: a lattice problem IS the dense-flow problem of expand(nodes).

No GPU and no library: tests/test_flow_lattice_cpu.py checks this file; tests/test_gpu_flow_lattice.py the kernels against it."""
import numpy as np

import flow_registration_restatement as fq
import flow_restatement as fr

MAX_STEP = 1024


class LatticeError(ValueError):
    """What the entry point answers SRMAP_EINVAL for before it looks at a node."""


def check_domain(step, lw, lh, W, H):
    if not 1 <= step <= MAX_STEP:
        raise LatticeError("step")
    if lw < 2 or lh < 2:
        raise LatticeError("nodes")
    if (lw - 1) * step >= W + step or (lh - 1) * step >= H + step:
        raise LatticeError("reach")


def expand(nodes, step, H, W, dtype=np.float64):
    """[...][H][W] doubles from nodes [...][lh][lw]: the field the kernels interpolate, rounded once to dtype."""
    n = np.asarray(nodes, dtype=np.float64)
    lh, lw = n.shape[-2:]
    check_domain(step, lw, lh, W, H)
    lead = n.shape[:-2]
    planes = n.reshape((-1, lh, lw))
    out = fq.resample(planes, H, W, 0.0, float(step), 1.0)
    return fr.stored(out.reshape(lead + (H, W)), dtype)


def nodes_from_registration(u, scale):
    """The lattice of an input-level estimate u [...][h][w] (LR pixels): nodes = scale * u at step = scale, lw = w, lh = h."""
    return float(scale) * np.asarray(u, dtype=np.float64)


def covering_size(W, H, step):
    """(lw, lh) of the smallest lattice whose last node is at or beyond the last pixel."""
    return -(-(W - 1) // step) + 1 if W > 1 else 2, -(-(H - 1) // step) + 1 if H > 1 else 2


def node_difference_sum(nodes, step):
    """(largest node difference along x + along y) / step of one frame's nodes [2][lh][lw]: what quality[3i+2] of
    srmap_problem_register_flow_lattice reports, and -- for a lattice that covers the image -- max_neighbour_sum of the
    expanded field to rounding (a bilinear interpolant's neighbour differences are convex combinations of its cells')."""
    n = np.asarray(nodes, dtype=np.float64)
    dx = np.max(np.abs(n[:, :, 1:] - n[:, :, :-1]))
    dy = np.max(np.abs(n[:, 1:, :] - n[:, :-1, :]))
    return float(dx + dy) / float(step)


# ------------------------------------------------------------------------------------------- the GPU tests' lattices
FORMS = ("registration", "covering", "two")


def lattice_size(form, step, h, w, scale):
    W, H = w * scale, h * scale
    if form == "registration":
        assert step == scale
        return w, h
    if form == "covering":
        lw, lh = covering_size(W, H, step)
        return max(lw, 2), max(lh, 2)
    return 2, 2


def random_nodes(rng, K, lw, lh, step, offsets, slope=0.16):
    """Nodes whose neighbour differences stay within slope * step per axis (dx + dy of the expanded field <= 2 slope <
    the documented 0.4) around a per-frame offset (ox, oy) in HR pixels."""
    out = np.empty((K, 2, lh, lw))
    for k in range(K):
        for c in range(2):
            out[k, c] = offsets[k][c] + 0.5 * slope * step * rng.uniform(-1.0, 1.0, (lh, lw))
    return out


# (LR h, LR w, scale, step, form, blur, channels, frames); blur: 0 / 3 = Gaussian size, "free" = the free-form 5 x 5,
# "bank" = a per-frame bank of 3 x 3 kernels.  Every LR size, scale, step (1, 2, 3, 4, 8, 64), form, blur, C and K of the
# issue's list appears; 70 x 129 spans many workgroups and its last cell at step 3 is ragged (257 = 85 * 3 + 2).
CASES = [
    (5, 7, 2, 2, "registration", 0, 1, 2),
    (5, 7, 4, 4, "registration", "free", 3, 5),
    (5, 7, 3, 64, "two", 3, 1, 2),
    (9, 13, 3, 3, "registration", 3, 1, 5),
    (9, 13, 2, 1, "covering", "bank", 3, 2),
    (9, 13, 4, 8, "covering", 0, 1, 2),
    (17, 23, 2, 4, "covering", "free", 1, 2),
    (17, 23, 3, 2, "two", "bank", 3, 5),
    (17, 23, 4, 4, "registration", 3, 1, 2),
    (70, 129, 2, 3, "covering", 3, 1, 2),
]


def case_offsets(K, W, H):
    """Per-frame (ox, oy): frame 0 none, sub-pixel and integer translations, and the last frame pushed a third of the
    image outside."""
    table = [(0.0, 0.0), (0.37, -0.61), (-2.0, 1.0), (1.25, 2.5), (0.0, 0.0)]
    out = [table[k % len(table)] for k in range(K)]
    out[K - 1] = (W / 3.0 + 0.3, -0.45)
    return out


def case_nodes(h, w, scale, step, form, K):
    W, H = w * scale, h * scale
    lw, lh = lattice_size(form, step, h, w, scale)
    rng = np.random.default_rng(7000 + 100 * h + 10 * scale + step)
    return random_nodes(rng, K, lw, lh, step, case_offsets(K, W, H))


# the refusals: name -> what flow_restatement.classify says of the expanded field of the frame the defect sits in, at
# the geometry (LR h, LR w, scale, step, frames) with the covering lattice
REFUSAL_GEOMETRY = (21, 33, 2, 4, 4)


def refusal_nodes(name, K, lw, lh, step, W, H):
    """A valid lattice with one defect in frame 1."""
    rng = np.random.default_rng(99)
    n = random_nodes(rng, K, lw, lh, step, [(0.0, 0.0)] * K)
    if name == "folded":
        # every pixel of the middle third samples one source column: nodes = (lo + 0.5) - node position there
        X = np.arange(lw, dtype=np.float64) * step
        lo, hi = W // 3, 2 * W // 3
        n[1, 0] = np.where((X >= lo) & (X < hi), (lo + 0.5) - X, 0.0)[None, :]
        n[1, 1] = 0.0
    elif name == "steep":
        # a node difference of 0.9 step per node along both axes: dx + dy = 1.8 of the expanded field
        n[1, 0] = -0.9 * step * (np.arange(lw)[None, :] + np.arange(lh)[:, None])
        n[1, 1] = -0.9 * step * (np.arange(lw)[None, :] + np.arange(lh)[:, None])
    elif name == "nan":
        n[1, 1, lh // 2, lw // 2] = np.nan
    elif name == "huge":
        n[1, 0, lh // 2, lw // 2] = 2.0 ** 20 + 4.0 * step
    else:
        raise KeyError(name)
    return n


REFUSALS = {"folded": "eunsupported", "steep": "eunsupported", "nan": "einval", "huge": "eunsupported"}
