"""CPU checks of the affine registration (include/srmap.h: srmap_register_affine) through its numpy restatement,
tests/affine_registration_restatement.py: the recovery contract on bilinear-warped texture, the central-window seed, the
pyramid transfer rules, and the README's figures (matrices estimated from the LR frames alone, then the affine solve).
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
import robust_restatement as rr  # noqa: E402
from test_affine_cpu import TABLE as MODEL_TABLE  # noqa: E402  the figures with the TRUE matrices / shifts
from test_gpu_registration import texture  # noqa: E402

NOISE_FREE_BAR = 0.05  # px: the project's bar for bilinear-warped content (test_gpu_registration.py)
NOISE_BAR = 0.1        # px: its bar under sigma = 0.01 noise


def warped(img, M):
    H, W = img.shape
    return ar.warp_forward(ar.warp_triplets(M, W, H), img[None])[0]


def contract_cases(W, H):
    """(name, true matrix): rotations / scales about the image centre plus a shift, and one general matrix with shear."""
    shear = np.array([[1.03, 0.04, 0.0], [-0.02, 0.97, 0.0]])
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    shear[:, 2] = c - shear[:, :2] @ c + np.array([2.0, -1.5])
    return [("identity", ar.translation(0, 0)),
            ("0.5deg", ar.rotation_about_centre(0.5, (1.25, .75), W, H)),
            ("2deg", ar.rotation_about_centre(2, (-3, 2), W, H)),
            ("-5deg_s1.02", ar.rotation_about_centre(-5, (4.5, -2.25), W, H, 1.02)),
            ("7deg", ar.rotation_about_centre(7, (0, 0), W, H)),
            ("3deg_s0.97", ar.rotation_about_centre(3, (10, -7), W, H, 0.97)),
            ("shear", shear)]


def contract_stack(H, W, noise=0.0):
    """(stack [8][H][W], true matrices): frame 0 the texture, frames 1..7 the cases."""
    img = texture(np.random.default_rng(H + W), H, W)
    mats = [m for _, m in contract_cases(W, H)]
    stack = np.stack([img] + [warped(img, m) for m in mats])
    if noise:
        stack = stack + noise * np.random.default_rng(1).standard_normal(stack.shape)
    return stack, np.stack([ar.translation(0, 0)] + mats)


def test_library_exports_and_header_declares_the_entry_point():
    import srmap
    assert "srmap_register_affine" in srmap.EXPORTED_SYMBOLS
    assert "srmap_affine_registration_options_default" in srmap.EXPORTED_SYMBOLS
    with open(os.path.join(ROOT, "include", "srmap.h")) as f:
        header = f.read()
    assert re.search(r"int\s+srmap_register_affine\s*\(", header)
    assert "srmap_affine_registration_options" in header
    assert "caller's job" not in header


@pytest.mark.parametrize("size", [(96, 128), (131, 157)])
@pytest.mark.parametrize("noise", [0.0, 0.01])
def test_recovery_contract(size, noise):
    H, W = size
    stack, truth = contract_stack(H, W, noise)
    got, q = rg.register_affine(stack, with_quality=True)
    assert np.array_equal(got[0], rg.identity())
    worst = 0.0
    for k, (name, _) in enumerate(contract_cases(W, H), start=1):
        err = rg.corner_displacement(got[k], truth[k], W, H)
        print("%3d x %3d noise %.2f %-12s corner error %.4f px  quality %s" % (H, W, noise, name, err, np.round(q[k], 4)))
        worst = max(worst, err)
    assert worst <= (NOISE_BAR if noise else NOISE_FREE_BAR)


def test_central_window_seed_under_rotation():
    """240 x 320, 7 degrees about the centre, zero shift: the overlap-window search answers a far-away shift here (the zero
    wedges of the rotated frame); the fixed central window must seed (0, 0) at the coarsest level."""
    H, W = 240, 320
    img = texture(np.random.default_rng(H + W), H, W)
    M = ar.rotation_about_centre(7, (0, 0), W, H)
    frame = warped(img, M)
    L = rg.num_levels(W, H)
    assert L == 3
    seed, sep = rg.coarse_seed(rg.pyramid(img, L)[-1], rg.pyramid(frame, L)[-1])
    print("seed", seed, "separation %.3f" % sep)
    assert max(abs(seed[0]), abs(seed[1])) <= 1
    F, _, its = rg.register_pair(img, frame)
    err = rg.corner_displacement(F, M, W, H)
    print("corner error %.4f px, iterations %s" % (err, its))
    assert err <= NOISE_FREE_BAR


def test_pyramid_levels_and_transfer_rules():
    assert [rg.num_levels(w, h) for w, h in ((8, 8), (63, 200), (64, 64), (127, 500), (128, 128), (1024, 1024))] == [1, 1, 2, 2, 3, 6]
    assert rg.num_levels(1024, 1024, 1) == 1 and rg.num_levels(1024, 1024, 3) == 3 and rg.num_levels(1 << 20, 1 << 20) == 12
    assert rg.down2(np.arange(35.0).reshape(5, 7)).shape == (2, 3)
    rng = np.random.default_rng(0)
    for _ in range(20):
        M = ar.random_matrix(rng, 0.2, shift=20.0)
        assert np.max(np.abs(rg.to_finer(rg.to_coarser(M)) - M)) <= 1e-13
        assert np.max(np.abs(rg.to_coarser(rg.to_finer(M)) - M)) <= 1e-13
        # the rule IS "fine p = 2 u + 1/2": mapping a coarse point and lifting it equals lifting it and mapping it
        u = rng.uniform(0, 50, (16, 2))
        assert np.max(np.abs((2 * rg.apply_map(M, u) + 0.5) - rg.apply_map(rg.to_finer(M), 2 * u + 0.5))) <= 1e-11
        # F o W^-1 on sample points: (F o W^-1)(W(p)) = F(p)
        delta = rng.uniform(-0.02, 0.02, 6) * np.array([1, 1, 50, 1, 1, 50])
        Wm = rg.increment_matrix(delta, 128, 96)
        c = np.array([(128 - 1) / 2.0, (96 - 1) / 2.0])
        D, d = np.array([[delta[0], delta[1]], [delta[3], delta[4]]]), np.array([delta[2], delta[5]])
        assert np.max(np.abs(rg.apply_map(Wm, u) - (u + (u - c) @ D.T + d))) <= 1e-11
        assert np.max(np.abs(rg.apply_map(rg.compose_with_inverse(M, Wm), rg.apply_map(Wm, u)) - rg.apply_map(M, u))) <= 1e-10


def test_sums_do_not_sample_outside_and_flat_frames_keep_their_matrix():
    """A pixel whose taps leave the frame is left out (n shrinks with the shift); no texture is a Cholesky failure, not an
    error; too small an overlap and a step that leaves the model's domain are errors."""
    img = texture(np.random.default_rng(2), 40, 48)
    n0 = rg.gn_sums(img, img, ar.translation(0, 0))[3]
    n5 = rg.gn_sums(img, img, ar.translation(5.5, 0))[3]
    assert n0 == 38 * 46 and n5 == 38 * (46 - 5)
    flat = np.full((2, 64, 64), 0.5)
    got, q = rg.register_affine(flat, with_quality=True)
    assert np.all(np.isfinite(got)) and np.array_equal(got[1][:, :2], np.eye(2))
    with pytest.raises(rg.RegistrationError):
        rg.register_affine(np.stack([img, img]), init=np.stack([ar.translation(0, 0), ar.translation(40, 0)]))
    with pytest.raises(rg.RegistrationError):
        rg.register_affine(np.zeros((2, 4, 4)))


# ---- the figures of the README: matrices estimated from the LR frames alone (hr_scale = 2), then the affine solve.
# PSNR in dB and (IRLS rounds, iterations, evaluations), taken from this restatement's own run ----
TABLE = {
    "0.5deg": {"estimated_l2": (37.624, (7, 121, 183)), "estimated_huber": (37.640, (7, 117, 177))},
    "2deg": {"estimated_l2": (37.605, (7, 118, 176)), "estimated_huber": (37.732, (7, 128, 189))},
}
MARGIN_OVER_TRANSLATION = {"0.5deg": 1.0, "2deg": 10.0}  # dB over the translation-only L2 with the TRUE shifts
WITHIN_TRUE_MATRICES = 0.75                               # dB below the affine L2 with the TRUE matrices


def solve_with_estimate(T, name):
    """Register the LR frames of one table input and solve with the estimated matrices: (matrices, row)."""
    _, _, y = T["inputs"][name]
    est = rg.register_affine(y[:, 0], hr_scale=T["s"])
    model = ar.AffineImageModel(T["s"], est, *T["blur"])
    x0 = rr.bilinear(y[0], T["s"])
    row = {}
    for label, loss in (("estimated_l2", "l2"), ("estimated_huber", "huber")):
        x, rep, _ = rr.irls_solve(model, y, x0, reg=T["reg"], loss=loss, delta=T["delta"] if loss == "huber" else None,
                                  composed=True)
        row[label] = (orc.psnr(T["gt"], x), (rep.irls_rounds, rep.cg_iterations, rep.nfev))
    return est, row


@pytest.fixture(scope="module")
def table():
    T = ar.table_inputs()
    return T, {name: solve_with_estimate(T, name) for name in T["inputs"]}


@pytest.mark.parametrize("name", ["0.5deg", "2deg"])
def test_table_figures(table, name):
    T, rows = table
    est, row = rows[name]
    truth = T["inputs"][name][0]
    errs = [rg.corner_displacement(est[k], truth[k], T["W"], T["H"]) for k in range(1, T["K"])]
    print("%s: corner error of the estimate per frame (HR px): %s" % (name, np.round(errs, 3)))
    for label in ("estimated_l2", "estimated_huber"):
        print("  %-16s %.2f dB (%d/%d/%d)" % ((label, row[label][0]) + row[label][1]))
    for label in ("estimated_l2", "estimated_huber"):
        assert row[label][1] == TABLE[name][label][1], label
        assert abs(row[label][0] - TABLE[name][label][0]) <= 0.05, label


@pytest.mark.parametrize("name", ["0.5deg", "2deg"])
def test_estimated_matrices_close_the_loop(table, name):
    _, rows = table
    got = rows[name][1]["estimated_l2"][0]
    trans, true = MODEL_TABLE[name]["trans_l2"][0], MODEL_TABLE[name]["affine_l2"][0]
    print("%s: estimated-affine L2 %.2f dB, translation-only L2 (true shifts) %.2f dB, true matrices %.2f dB" % (name, got, trans, true))
    assert got - trans >= MARGIN_OVER_TRANSLATION[name]
    assert true - got <= WITHIN_TRUE_MATRICES
