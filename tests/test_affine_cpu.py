"""CPU checks of the affine motion model's CHECKER (tests/affine_restatement.py) and of the library's new boundary: the
triplet warp and its literal transpose (adjoint identity, finite differences), the gather form the kernel uses against the
triplet transpose, the pure-translation anchor against the reference-pinned translational model, the figures the README
quotes, and the new symbol."""
import os
import re
import sys

import numpy as np
import pytest

import oracle as orc

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import robust_restatement as rr  # noqa: E402

# shifts that are multiples of 1/32 px and no rounding ties, plus integer shifts
ANCHOR_SHIFTS = [(1.25, .75), (-.40625, 2.15625), (3, -2), (0, 0), (1, 0), (-2, 3)]


def test_library_exports_and_header_declares_the_affine_entry_point():
    import __graft_entry__ as ge
    ge.build_lib()
    import srmap
    lib = srmap.load()
    name = "srmap_problem_set_affine_motion"
    text = open(os.path.join(ROOT, "include", "srmap.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*srmap_problem\s*\*\s*p\s*,\s*const\s+double\s*\*\s*affine_2x3\s*\)" % name, code)
    assert hasattr(lib, name)
    assert name in srmap.EXPORTED_SYMBOLS
    assert callable(getattr(srmap.Problem, "set_affine_motion", None))
    at = text.index("int %s(" % name)
    comment = text[text.rindex("/*", 0, at):at]
    assert "no reference counterpart" in comment.lower()
    assert "motion_module.cpp:18-51" in comment


def _bound_matrices(seed, n):
    rng = np.random.default_rng(seed)
    mats = [ar.random_matrix(rng, ar.MAX_DEVIATION, at_bound=True) for _ in range(n)]
    for M in mats:
        assert ar.MAX_DEVIATION - 1e-12 <= ar.deviation(M) <= ar.MAX_DEVIATION
    return mats


@pytest.mark.parametrize("scale,blur", [(2, 3), (3, 0), (4, 5)])
def test_adjoint_identity_at_the_domain_bound(scale, blur):
    rng = np.random.default_rng(10 * scale + blur)
    mats = _bound_matrices(scale, 6)
    C, h, w = 2, 11, 13
    model = ar.AffineImageModel(scale, mats, blur, 1.0 if blur else 0.0)
    for k in range(len(mats)):
        u = rng.standard_normal((C, h * scale, w * scale))
        v = rng.standard_normal((C, h, w))
        lhs = np.sum(model.apply(u, k) * v)
        rhs = np.sum(u * model.apply_transpose(v, k))
        rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
        print("scale %d blur %d frame %d: <Au,v> %.15g <u,A^Tv> %.15g rel %.2e" % (scale, blur, k, lhs, rhs, rel))
        assert rel <= 1e-13


def test_gradient_matches_finite_differences():
    rng = np.random.default_rng(5)
    s, C, h, w = 2, 1, 9, 10
    mats = [ar.translation(0, 0)] + _bound_matrices(11, 3)
    model = ar.AffineImageModel(s, mats, 3, 1.0)
    y = rng.random((len(mats), C, h, w))
    wts = 2.0 * rng.random(y.shape)
    wts[2] = 0.0
    x = rng.random((C, h * s, w * s))
    for wt in (None, wts):
        _, g = rr.weighted_data_term(model, y, wt, x)
        eps, worst = 1e-6, 0.0
        for idx in rng.choice(x.size, 40, replace=False):
            d = np.zeros(x.size)
            d[idx] = eps
            fp, _ = rr.weighted_data_term(model, y, wt, x + d.reshape(x.shape), want_grad=False)
            fm, _ = rr.weighted_data_term(model, y, wt, x - d.reshape(x.shape), want_grad=False)
            worst = max(worst, abs((fp - fm) / (2 * eps) - g.ravel()[idx]))
        print("worst central-difference deviation %.3e" % worst)
        assert worst <= 1e-6  # the cost is quadratic: the central difference is exact up to rounding (~1e-16 * f / eps)


def test_gather_form_equals_the_triplet_transpose_with_at_most_nine_candidates():
    rng = np.random.default_rng(3)
    W, H = 37, 29
    mats = _bound_matrices(7, 6) + [ar.rotation_about_centre(7.0, (1.3, -2.6), W, H), ar.translation(.3, -.7),
                                    ar.translation(0, 0), ar.translation(2, -1)]
    for M in mats:
        u = rng.standard_normal((2, H, W))
        trip = ar.warp_triplets(M, W, H)
        ref = ar.warp_transpose(trip, u)
        got, counts = ar.gather_adjoint(M, u, return_counts=True)
        per_pixel = np.bincount(trip[1][trip[2] != 0], minlength=W * H)  # pixels q whose footprint holds p
        err = np.max(np.abs(got - ref))
        print("deviation %.3f: gather vs transpose %.2e, candidates per pixel <= %d (gather walked %d)" % (
            ar.deviation(M), err, per_pixel.max(), counts.max()))
        assert err <= 1e-14
        assert per_pixel.max() <= 9
        assert np.array_equal(counts.ravel(), per_pixel)  # the 3 x 3 box missed none and invented none


@pytest.mark.parametrize("scale,blur", [(2, 3), (3, 0)])
def test_pure_translation_anchor_against_the_translational_model(scale, blur):
    """Exact-coordinate bilinear warping equals warpAffine's 1/32-px quantised one on shifts that are multiples of 1/32 px
    off the rounding ties (measured difference: 0.0), forward and transpose."""
    rng = np.random.default_rng(scale)
    C, h, w = 2, 12, 15
    sig = 1.0 if blur else 0.0
    ref = orc.ImageModel(scale=scale, shifts=ANCHOR_SHIFTS, blur_ksize=blur, blur_sigma=sig)
    model = ar.AffineImageModel(scale, [ar.translation(dx, dy) for dx, dy in ANCHOR_SHIFTS], blur, sig)
    x = rng.random((C, h * scale, w * scale))
    v = rng.random((C, h, w))
    for k, sh in enumerate(ANCHOR_SHIFTS):
        ef = np.max(np.abs(model.apply(x, k) - ref.apply(x, k)))
        et = np.max(np.abs(model.apply_transpose(v, k) - ref.apply_transpose(v, k)))
        eg = np.max(np.abs(model.apply_transpose_gather(v, k) - ref.apply_transpose(v, k)))
        print("shift %s: forward %.2e transpose %.2e gather form %.2e" % (sh, ef, et, eg))
        assert ef <= 1e-14 and et <= 1e-14 and eg <= 1e-14


# ---- the figures of the README: PSNR in dB and (IRLS rounds, iterations, evaluations) ----
TABLE = {
    "0.5deg": {"bilinear": 32.53, "trans_l2": (36.01, (7, 113, 177)), "trans_huber": (36.31, (7, 116, 174)),
               "affine_l2": (38.08, (7, 112, 167)), "affine_huber": (38.09, (7, 105, 160))},
    "2deg": {"bilinear": 32.53, "trans_l2": (25.58, (7, 81, 133)), "trans_huber": (29.39, (7, 147, 207)),
             "affine_l2": (37.95, (6, 104, 159)), "affine_huber": (38.10, (7, 111, 167))},
}
MARGIN = {"0.5deg": 1.5, "2deg": 10.0}  # affine L2 over translation-only L2 (measured 2.07 and 12.4 dB)


@pytest.fixture(scope="module")
def table():
    T = ar.table_inputs()
    out = {}
    for name, (_, model, y) in T["inputs"].items():
        x0 = rr.bilinear(y[0], T["s"])
        row = {"bilinear": orc.psnr(T["gt"], x0)}
        for label, mdl, loss in (("trans_l2", T["translation_model"], "l2"), ("trans_huber", T["translation_model"], "huber"),
                                 ("affine_l2", model, "l2"), ("affine_huber", model, "huber")):
            x, rep, _ = rr.irls_solve(mdl, y, x0, reg=T["reg"], loss=loss, delta=T["delta"] if loss == "huber" else None,
                                      composed=True)
            row[label] = (orc.psnr(T["gt"], x), (rep.irls_rounds, rep.cg_iterations, rep.nfev))
        out[name] = row
    return out


@pytest.mark.parametrize("name", ["0.5deg", "2deg"])
def test_table_figures(table, name):
    row = table[name]
    print("%s: bilinear %.2f dB" % (name, row["bilinear"]))
    for label in ("trans_l2", "trans_huber", "affine_l2", "affine_huber"):
        print("  %-12s %.2f dB (%d/%d/%d)" % ((label, row[label][0]) + row[label][1]))
    assert abs(row["bilinear"] - TABLE[name]["bilinear"]) <= 0.05
    for label in ("trans_l2", "trans_huber", "affine_l2", "affine_huber"):
        # the reference's ALGLIB and the restated mincg walk the same trajectory on these inputs (both were measured)
        assert row[label][1] == TABLE[name][label][1], label
        assert abs(row[label][0] - TABLE[name][label][0]) <= 0.05, label


@pytest.mark.parametrize("name", ["0.5deg", "2deg"])
def test_affine_beats_translation_only(table, name):
    row = table[name]
    gain = row["affine_l2"][0] - row["trans_l2"][0]
    print("%s: affine L2 %.2f dB, translation-only L2 %.2f dB, gain %.2f dB" % (name, row["affine_l2"][0], row["trans_l2"][0], gain))
    assert gain >= MARGIN[name]
