"""CPU checks of the joint motion refinement (include/srmap.h: srmap_refine_motion) through its numpy
restatement, tests/motion_refinement_restatement.py: the Jacobian against central differences of the restated forward
model, the recovery contract, the translation-only form, the data weights, the README's table (registered matrices -> L2
solve -> 3 x (refinement, warm solve) -> cold solve) and the accept / reject margins of the GPU tests' whole-run inputs.
"""
import os
import re
import sys

import numpy as np
import pytest

import oracle as orc

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import affine_registration_restatement as rg  # noqa: E402
import motion_refinement_restatement as mr  # noqa: E402
import robust_restatement as rr  # noqa: E402
from test_affine_cpu import TABLE as MODEL_TABLE  # noqa: E402  the figures with the TRUE matrices
from test_affine_registration_cpu import TABLE as REGISTERED_TABLE, contract_cases  # noqa: E402
from test_gpu_registration import texture  # noqa: E402

NOISE_FREE_BAR = 0.05  # HR px: the project's registration bars (test_affine_registration_cpu.py)
NOISE_BAR = 0.1


def test_library_exports_and_header_declares_the_entry_points():
    import srmap
    with open(os.path.join(ROOT, "include", "srmap.h")) as f:
        header = f.read()
    for name in ("srmap_motion_refinement_options_default", "srmap_refine_motion", "srmap_refine_motion_device"):
        assert name in srmap.EXPORTED_SYMBOLS
        assert re.search(r"(int|void)\s+" + name + r"\s*\(", header)
        assert hasattr(srmap.load(), name)
    assert "srmap_motion_refinement_options;" in header and "3.8" in header


def displaced(rng, M, W, H, px):
    """M with a random change of all six entries whose corner displacement is exactly px."""
    d = np.hstack([rng.uniform(-1, 1, (2, 2)) / max(W, H), rng.uniform(-1, 1, (2, 1))])
    return M + d * (px / rg.corner_displacement(M + d, M, W, H))


def frames_of(x, mats, taps, s):
    return np.stack([mr.model_and_jacobian(x, ar.inverse_map(m), taps, s)[0] for m in mats])


# ------------------------------------------------------------------------------------------- the model and its Jacobian
@pytest.mark.parametrize("scale,blur,C", [(2, 0, 1), (2, 3, 3), (3, 3, 1), (3, 5, 3), (4, 0, 3), (4, 5, 1)])
def test_blur_and_decimation_are_the_oracles(scale, blur, C):
    rng = np.random.default_rng(scale * 10 + blur)
    H, W = 9 * scale, 11 * scale
    x = rng.random((C, H, W))
    taps = mr.blur_taps(blur, 1.0)
    db = orc.ImageModel(scale=scale, shifts=None, blur_ksize=blur, blur_sigma=1.0)
    assert np.max(np.abs(mr.blur_decimate(x, taps, scale) - db.apply(x, 0))) <= 1e-15
    M = ar.random_matrix(rng, 0.2)
    model = ar.AffineImageModel(scale, M[None], blur, 1.0)
    assert np.max(np.abs(mr.model_and_jacobian(x, ar.inverse_map(M), taps, scale)[0] - model.apply(x, 0))) <= 1e-14


# (scale, blur, C, seed): the seeds are chosen so that at most 1 % of the 192 LR pixels is excluded (a blur of 5 on a wide
# image puts 25 samples per pixel next to 2 h |q - c0| of cell border: blur 5 goes with the smaller scales)
JACOBIAN_CASES = [(2, 0, 1, 1), (2, 5, 3, 1), (3, 3, 1, 1), (3, 5, 3, 2), (4, 0, 3, 1), (4, 3, 1, 1)]


@pytest.mark.parametrize("at_bound", [False, True])
@pytest.mark.parametrize("scale,blur,C,seed", JACOBIAN_CASES)
def test_jacobian_against_central_differences(scale, blur, C, seed, at_bound):
    """Inside a cell of the sampling grid the model is quadratic in the parameters, so a central difference is exact up to
    rounding: every LR pixel none of whose sample coordinates crosses an integer between -h and +h agrees to 1e-8 max |J|,
    and those pixels are at least 99 % of all, per parameter."""
    h = 1e-5
    rng = np.random.default_rng(seed)
    Hh, Ww = 12 * scale, 16 * scale
    x = rng.random((C, Hh, Ww))
    taps = mr.blur_taps(blur, 1.0)
    M = ar.random_matrix(rng, 0.25 if at_bound else 0.2, shift=2.0, at_bound=at_bound)
    G = ar.inverse_map(M)
    _, J = mr.model_and_jacobian(x, G, taps, scale)
    cells0 = [np.floor(c) for c in mr.sample_with_derivatives(x, G)[3][:2]]
    ones = np.ones_like(taps)
    for i in range(6):
        d = np.zeros(6)
        d[i] = h
        Gp, Gm = mr.increment(G, d, Ww, Hh), mr.increment(G, -d, Ww, Hh)
        mp, mm = mr.model_and_jacobian(x, Gp, taps, scale)[0], mr.model_and_jacobian(x, Gm, taps, scale)[0]
        crossed = np.zeros((Hh, Ww), dtype=bool)
        for Gq in (Gp, Gm):
            sx, sy, _ = mr.sample_with_derivatives(x, Gq)[3]
            crossed |= (np.floor(sx) != cells0[0]) | (np.floor(sy) != cells0[1])
        excluded = mr.blur_decimate(crossed[None].astype(np.float64), ones, scale)[0] > 0
        share = np.mean(excluded)
        err = np.max(np.abs((mp - mm) / (2 * h) - J[i])[:, ~excluded])
        print("scale %d blur %d C %d %s parameter %d: excluded %.2f %%, max |difference - J| %.2e, max |J| %.2e"
              % (scale, blur, C, "bound" if at_bound else "random", i, 100 * share, err, np.max(np.abs(J[i]))))
        assert share <= 0.01
        assert err <= 1e-8 * np.max(np.abs(J))


# ------------------------------------------------------------------------------------------- recovery
@pytest.fixture(scope="module")
def T():
    return ar.table_inputs()


@pytest.mark.parametrize("noise", [0.0, 0.01])
def test_recovery_contract(T, noise):
    """x = the table's ground truth; frames made by the model at known matrices (rotations to 7 degrees, scale 0.97-1.02,
    shear, shifts); the start is the truth displaced by up to 1 HR px at the corners."""
    x, s, W, H = T["gt"], T["s"], T["W"], T["H"]
    taps = mr.blur_taps(*T["blur"])
    names = ["gauge"] + [n for n, _ in contract_cases(W, H)]
    truth = np.stack([ar.translation(0, 0)] + [m for _, m in contract_cases(W, H)])
    y = frames_of(x, truth, taps, s)
    if noise:
        y = y + noise * np.random.default_rng(3).standard_normal(y.shape)
    rng = np.random.default_rng(11)
    start = np.stack([truth[0]] + [displaced(rng, truth[k], W, H, 1.0 if k % 2 else rng.uniform(0.3, 1.0)) for k in range(1, len(truth))])
    got, q, _ = mr.refine_motion(x, y, None, start, taps, s)
    assert np.array_equal(got[0], truth[0]) and list(q[0, 2:]) == [0, 0] and q[0, 0] == q[0, 1]
    worst = 0.0
    for k in range(1, len(truth)):
        e0, e1 = rg.corner_displacement(start[k], truth[k], W, H), rg.corner_displacement(got[k], truth[k], W, H)
        print("noise %.2f %-12s corner error %.3f -> %.4f HR px, cost %.4e -> %.4e, passes %d, status %d"
              % (noise, names[k], e0, e1, q[k, 0], q[k, 1], q[k, 2], q[k, 3]))
        worst = max(worst, e1)
        assert q[k, 1] <= q[k, 0]
    assert worst <= (NOISE_BAR if noise else NOISE_FREE_BAR)


@pytest.mark.parametrize("noise", [0.0, 0.01])
def test_translation_only(T, noise):
    """dof = 2 on pure translations: the shifts to the same bars, L bit-identical."""
    x, s, W, H = T["gt"], T["s"], T["W"], T["H"]
    taps = mr.blur_taps(*T["blur"])
    truth = np.stack([ar.translation(*sh) for sh in T["shifts"]])
    y = frames_of(x, truth, taps, s)
    if noise:
        y = y + noise * np.random.default_rng(4).standard_normal(y.shape)
    rng = np.random.default_rng(12)
    start = truth.copy()
    for k in range(1, len(truth)):
        v = rng.standard_normal(2)
        start[k, :, 2] += v / np.hypot(*v) * (1.0 if k % 2 else 0.6)
    got, q, _ = mr.refine_motion(x, y, None, start, taps, s, dof=2)
    errs = [rg.corner_displacement(got[k], truth[k], W, H) for k in range(1, len(truth))]
    print("noise %.2f dof 2: corner errors %s HR px, passes %s, status %s" % (noise, np.round(errs, 4), q[1:, 2], q[1:, 3]))
    assert np.array_equal(got[:, :, :2], truth[:, :, :2])
    assert max(errs) <= (NOISE_BAR if noise else NOISE_FREE_BAR)


# ------------------------------------------------------------------------------------------- weights
def test_a_zero_weight_frame_keeps_its_matrix(T):
    x, s = T["gt"], T["s"]
    taps = mr.blur_taps(*T["blur"])
    truth, _, y = T["inputs"]["0.5deg"]
    start = truth.copy()
    start[1:, :, 2] += 0.3
    w = np.ones_like(y)
    w[2] = 0.0
    got, q, S = mr.refine_motion(x, y, w, start, taps, s)
    assert np.array_equal(got[2], start[2]) and list(q[2]) == [0.0, 0.0, 1.0, mr.STATUS_NO_TEXTURE] and not S[2].any()
    assert all(q[k, 3] == mr.STATUS_CONVERGED and not np.array_equal(got[k], start[k]) for k in (1, 3, 4, 5))


ROBUST_PINNED = {"unweighted": 0.309, "huber": 0.106}  # corner error of the corrupted frame, HR px, from this restatement's run


def test_huber_weights_make_the_refinement_robust(T):
    """3 % salt-and-pepper in frame 3 of the 0.5-degree input: matrices registered from the frames, a Huber solve, then
    frame 3 refined at that solve's x with its final weights and without weights."""
    s, W, H = T["s"], T["W"], T["H"]
    taps = mr.blur_taps(*T["blur"])
    truth, _, y = T["inputs"]["0.5deg"]
    rng = np.random.default_rng(21)
    y = y.copy()
    hit = rng.random(y[3].shape) < 0.03
    y[3] = np.where(hit, rng.integers(0, 2, y[3].shape).astype(float), y[3])
    est = rg.register_affine(y[:, 0], hr_scale=s)
    x, _, w = rr.irls_solve(ar.AffineImageModel(s, est, *T["blur"]), y, rr.bilinear(y[0], s), reg=T["reg"], loss="huber", delta=T["delta"])
    errs = {}
    for label, wk in (("unweighted", None), ("huber", w[3])):
        F, q, _, _ = mr.refine_frame(x, y[3], wk, est[3], taps, s)
        errs[label] = rg.corner_displacement(F, truth[3], W, H)
        print("%-10s corner error of frame 3: %.4f -> %.4f HR px (cost %.4e -> %.4e, passes %d, status %d)"
              % (label, rg.corner_displacement(est[3], truth[3], W, H), errs[label], q[0], q[1], q[2], q[3]))
    assert errs["huber"] < errs["unweighted"]
    for label in errs:
        assert abs(errs[label] - ROBUST_PINNED[label]) <= 0.005, label


# ------------------------------------------------------------------------------------------- the table
# PSNR in dB and (IRLS rounds, iterations, evaluations) of each solve, and the largest corner error of frames 1...5 in HR
# px after each refinement, from this restatement's own run.
TABLE = {
    "0.5deg": {"unrefined": (37.623, (7, 121, 183)), "round1": (37.825, (6, 103, 216)), "round2": (37.925, (6, 95, 203)),
               "round3": (38.049, (7, 131, 191)), "cold": (38.017, (7, 105, 163)), "corner": (0.185, 0.096, 0.077)},
    "2deg": {"unrefined": (37.605, (7, 118, 176)), "round1": (37.917, (7, 116, 177)), "round2": (37.951, (7, 113, 180)),
             "round3": (37.952, (6, 93, 142)), "cold": (38.022, (7, 125, 187)), "corner": (0.303, 0.138, 0.084)},
}
COLD_OVER_UNREFINED = 0.25   # dB
WITHIN_TRUE_MATRICES = 0.15  # dB
CORNER_AFTER_ROUND_3 = 0.1   # HR px


def joint_rows(T, name, x0=None, cold=True):
    """Registered matrices -> L2 solve -> 3 x (refine frames 1...5, warm solve) [-> cold L2 solve with the final matrices]:
    (rows {label: (psnr, counts)}, corner errors per round, qualities per round, final matrices)."""
    truth, _, y = T["inputs"][name]
    s = T["s"]
    taps = mr.blur_taps(*T["blur"])

    def solve(mats, start):
        x, rep, _ = rr.irls_solve(ar.AffineImageModel(s, mats, *T["blur"]), y, start, reg=T["reg"], composed=True)
        return x, (orc.psnr(T["gt"], x), (rep.irls_rounds, rep.cg_iterations, rep.nfev))

    first = rr.bilinear(y[0], s) if x0 is None else x0
    mats = rg.register_affine(y[:, 0], hr_scale=s)
    rows, corners, quals = {}, [], []
    x, rows["unrefined"] = solve(mats, first)
    for r in (1, 2, 3):
        mats, q, _ = mr.refine_motion(x, y, None, mats, taps, s)
        x, rows["round%d" % r] = solve(mats, x)
        corners.append(max(rg.corner_displacement(mats[k], truth[k], T["W"], T["H"]) for k in range(1, T["K"])))
        quals.append(q)
    if cold:
        _, rows["cold"] = solve(mats, first)
    return rows, corners, quals, mats


@pytest.fixture(scope="module")
def table(T):
    return {name: joint_rows(T, name) for name in T["inputs"]}


@pytest.mark.parametrize("name", ["0.5deg", "2deg"])
def test_table_figures(T, table, name):
    rows, corners, quals, _ = table[name]
    for label in ("unrefined", "round1", "round2", "round3", "cold"):
        print("%s %-10s %.3f dB (%d/%d/%d)" % ((name, label, rows[label][0]) + rows[label][1]))
    print("%s largest corner error after each refinement (HR px): %s; passes per frame and round: %s"
          % (name, np.round(corners, 3), [q[1:, 2].astype(int).tolist() for q in quals]))
    assert rows["unrefined"][1] == REGISTERED_TABLE[name]["estimated_l2"][1]  # the same start as the registration's row
    for label in ("unrefined", "round1", "round2", "round3", "cold"):
        assert rows[label][1] == TABLE[name][label][1], label
        assert abs(rows[label][0] - TABLE[name][label][0]) <= 0.05, label
    assert np.max(np.abs(np.array(corners) - TABLE[name]["corner"])) <= 0.005


@pytest.mark.parametrize("name", ["0.5deg", "2deg"])
def test_refinement_recovers_the_registration_loss(table, name):
    rows, corners, quals, _ = table[name]
    true = MODEL_TABLE[name]["affine_l2"][0]
    print("%s: unrefined %.3f dB, cold solve with the refined matrices %.3f dB, true matrices %.2f dB"
          % (name, rows["unrefined"][0], rows["cold"][0], true))
    assert rows["cold"][0] - rows["unrefined"][0] >= COLD_OVER_UNREFINED
    assert true - rows["cold"][0] <= WITHIN_TRUE_MATRICES
    assert corners[2] <= CORNER_AFTER_ROUND_3
    for q in quals:
        assert np.all(q[:, 1] <= q[:, 0])  # E_k never increases across a refinement call


# The restatement's own movement of the round-3 PSNR when x0 is perturbed by 1e-14 relative (joint_rows with that x0):
# 2.8e-11 dB and 1.1e-11 dB on the two inputs.  The GPU end-to-end test's bar is max(0.01 dB, ten times this).
ROUND_3_SENSITIVITY = 3e-11


# ------------------------------------------------------------------------------------------- the GPU tests' whole runs
WHOLE_RUN_OPTIONS = dict(max_iterations=30, step_tolerance=1e-2, initial_damping=1e-3)


def whole_run_input(lr_shape, dof=6):
    """(x, y, weights or None, start, truth, scale, blur) of a whole-run case of tests/test_gpu_motion_refinement.py: textured
    x, 4 frames made by the model plus sigma 0.01 noise, the start 0.5 HR px off at the corners."""
    h, w = lr_shape
    s, blur, C, K = 2, (3, 1.0), 2 if h < 40 else 1, 4
    H, W = h * s, w * s
    rng = np.random.default_rng(h * 100 + w + dof)
    x = np.stack([texture(rng, H, W) for _ in range(C)])
    if dof == 2:
        truth = np.stack([ar.translation(0, 0), ar.translation(1.25, -.5), ar.translation(-.75, .4), ar.translation(.3, 2.2)])
    else:
        truth = np.stack([ar.translation(0, 0), ar.rotation_about_centre(1.5, (1.25, .75), W, H),
                          ar.rotation_about_centre(-3, (-.5, 1.5), W, H, 1.01), ar.rotation_about_centre(0.4, (2.25, -1), W, H, 0.99)])
    taps = mr.blur_taps(*blur)
    y = frames_of(x, truth, taps, s) + 0.01 * rng.standard_normal((K, C, h, w))
    start = truth.copy()
    for k in range(1, K):
        if dof == 2:
            start[k, :, 2] += np.array([0.3, -0.4])
        else:
            start[k] = displaced(rng, truth[k], W, H, 0.5)
    wts = 0.25 + rng.random(y.shape) if h < 40 else None
    return x, y, wts, start, truth, s, blur


WHOLE_RUNS = [((24, 32), 6), ((48, 64), 6), ((24, 32), 2)]


@pytest.mark.parametrize("lr_shape,dof", WHOLE_RUNS)
def test_whole_run_inputs_have_clear_decisions(lr_shape, dof):
    """Every accept / reject decision of the restatement on the GPU tests' whole-run inputs has a relative cost margin of at
    least 1e-9: summation order cannot flip one."""
    x, y, wts, start, truth, s, blur = whole_run_input(lr_shape, dof)
    got, q, _, dec = mr.refine_motion(x, y, wts, start, mr.blur_taps(*blur), s, with_decisions=True, dof=dof, **WHOLE_RUN_OPTIONS)
    margin = mr.min_margin(dec)
    errs = [rg.corner_displacement(got[k], truth[k], x.shape[2], x.shape[1]) for k in range(1, len(got))]
    print("LR %s dof %d: smallest margin %.2e, passes %s, status %s, decisions %s, corner errors %s"
          % (lr_shape, dof, margin, q[1:, 2], q[1:, 3], ["".join("A" if a else "r" for a, _, _ in d) for d in dec[1:]], np.round(errs, 3)))
    assert margin >= 1e-9
    assert np.all(q[1:, 2] >= 3)  # there is a trajectory to compare
