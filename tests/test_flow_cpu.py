"""CPU checks of the displacement-field motion model's CHECKER (tests/flow_restatement.py) and of the library's new
boundary: the adjoint identity of the sparse model, the integer-shift and affine anchors against the two existing
restatements, completeness of the seed-and-window rule (the gather form against the literal transpose, acceptance of the
GPU matrix's fields, refusal of a fold), the pinned table, and the new symbols."""
import os
import re
import sys

import numpy as np
import pytest

import oracle as orc

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import blur_kernel_restatement as bk  # noqa: E402
import flow_restatement as fr  # noqa: E402
import robust_restatement as rr  # noqa: E402


def matrix_fields(rng, H, W):
    """The fields of the GPU parity matrix (tests/test_gpu_flow.py), one frame each, by name."""
    far = fr.from_shifts([[-0.37 * W, 0.21 * H]], H, W)[0] + fr.smooth_random(rng, H, W, 0.3)
    bound = ar.random_matrix(rng, ar.MAX_DEVIATION, at_bound=True)
    return {
        "zero": np.zeros((2, H, W)),
        "integer": fr.from_shifts([[2, -1]], H, W)[0],
        "subpixel": fr.from_shifts([[-1.3, 0.45]], H, W)[0],
        "affine_bound": fr.from_affine([bound], H, W)[0],
        "sinusoid_bound": fr.at_bound(fr.sinusoid(H, W, 1.0, 17.0, offset=(-20.3, 7.6))),
        "smooth_random": fr.smooth_random(rng, H, W, 1.2),
        "third_outside": far,
    }


def test_library_exports_and_header_declares_the_flow_entry_points():
    import __graft_entry__ as ge
    ge.build_lib()
    import srmap
    lib = srmap.load()
    text = open(os.path.join(ROOT, "include", "srmap.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+srmap_problem_set_flow\s*\(\s*srmap_problem\s*\*\s*p\s*,\s*const\s+double\s*\*\s*flow_host\s*\)", code)
    assert re.search(r"\bint\s+srmap_problem_set_flow_device\s*\(\s*srmap_problem\s*\*\s*p\s*,\s*const\s+void\s*\*\s*flow_dev\s*,"
                     r"\s*void\s*\*\s*hip_stream\s*\)", code)
    for name in ("srmap_problem_set_flow", "srmap_problem_set_flow_device", "srmap_problem_get_flow"):
        assert hasattr(lib, name)
        assert name in srmap.EXPORTED_SYMBOLS
    for name in ("set_flow", "flow"):
        assert callable(getattr(srmap.Problem, name, None))
    at = text.index("int srmap_problem_set_flow(")
    comment = text[text.rindex("/*", 0, at):at]
    assert "no reference counterpart" in comment.lower()
    for word in ("SRMAP_EUNSUPPORTED", "SRMAP_EINVAL", "2^20", "exact transpose", "K*2*H*W"):
        assert word in comment, word
    # the module helpers state the two correspondences of the definition
    H, W = 9, 11
    shifts = [[1.25, -0.5], [0, 2]]
    assert np.array_equal(srmap.flow_from_shifts(shifts, H, W), fr.from_shifts(shifts, H, W))
    mats = [ar.rotation_about_centre(3.0, (0.5, -1.0), W, H, 1.02), ar.translation(1.5, 0.25)]
    assert np.max(np.abs(srmap.flow_from_affine(mats, H, W) - fr.from_affine(mats, H, W))) <= 16 * np.spacing(float(max(H, W)))


@pytest.mark.parametrize("scale,blur", [(1, 0), (2, 3), (3, 5), (4, 0)])
def test_adjoint_identity(scale, blur):
    """<A x, r> = <x, A^T r> to 1e-12 relative, over every field of the GPU matrix (Gaussian and free-form blur)."""
    rng = np.random.default_rng(10 * scale + blur)
    h, w, C = 9, 13, 2
    H, W = h * scale, w * scale
    fields = np.stack(list(matrix_fields(rng, H, W).values()))
    for taps in (bk.gaussian_taps(blur, 1.0), bk.streak_psf(5)):
        model = fr.FlowModel(scale, fields, taps)
        for k in range(len(fields)):
            u = rng.standard_normal((C, H, W))
            v = rng.standard_normal((C, h, w))
            Au, Atv = model.apply(u, k), model.apply_transpose(v, k)
            lhs, rhs = np.sum(Au * v), np.sum(u * Atv)
            rel = abs(lhs - rhs) / max(np.sqrt(np.sum(Au * Au) * np.sum(v * v)), 1e-300)
            assert rel <= 1e-12, (k, rel)


def test_integer_shift_flow_is_the_oracles_shifted_model():
    """u = (-dx, -dy) for integer (dx, dy): the SAME warp matrix as MotionModule's, entry for entry, and the same model."""
    rng = np.random.default_rng(3)
    s, h, w, C = 2, 10, 12, 2
    H, W = h * s, w * s
    shifts = [[0, 0], [1, 1], [-2, 3], [3, -1], [0, -4]]
    fields = fr.from_shifts(shifts, H, W)
    for k, (dx, dy) in enumerate(shifts):
        d = fr.warp_matrix(fields[k], W, H) - bk.shift_warp_matrix(W, H, dx, dy)
        assert d.nnz == 0 or np.max(np.abs(d.data)) == 0.0, k
    model = fr.gaussian_model(s, fields, 3, 1.0)
    ref = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=3, blur_sigma=1.0)
    x, v = rng.random((C, H, W)), rng.random((C, h, w))
    for k in range(len(shifts)):
        assert np.max(np.abs(model.apply(x, k) - ref.apply(x, k))) <= 1e-14
        assert np.max(np.abs(model.apply_transpose(v, k) - ref.apply_transpose(v, k))) <= 1e-14


def test_affine_flow_against_the_affine_restatement():
    """u(q) = F^-1(q) - q: s is rebuilt as q + (s - q), two roundings of at most half an ulp of the coordinate each, so an
    entry of the warp matrix moves by at most 4 ulps of the largest coordinate (two axes, two roundings)."""
    rng = np.random.default_rng(5)
    H, W = 96, 128
    mats = [ar.random_matrix(rng, ar.MAX_DEVIATION, at_bound=True), ar.rotation_about_centre(7.0, (1.3, -0.6), W, H, 1.02),
            ar.rotation_about_centre(2.0, (0.25, -1), W, H)]
    fields = fr.from_affine(mats, H, W)
    worst = 0.0
    for k, M in enumerate(mats):
        d = fr.warp_matrix(fields[k], W, H) - bk.affine_warp_matrix(M, W, H)
        worst = max(worst, float(np.max(np.abs(d.data))) if d.nnz else 0.0)
    bar = 4 * np.spacing(float(max(H, W)))
    print("largest difference of a matrix entry between the two formulations: %.2e (bar %.2e)" % (worst, bar))
    assert worst <= bar


def test_seed_and_window_rule_is_complete_on_the_matrix_fields():
    """Every field of the GPU matrix is accepted, and the gather form then IS the literal transpose; the table's fields,
    the issue's sinusoid on a (-20.3, 7.6) px offset and a 7-degree rotation with 2 % of scale likewise."""
    for H, W in ((10, 14), (27, 39), (140, 258)):
        rng = np.random.default_rng(H)
        for name, f in matrix_fields(rng, H, W).items():
            for dtype in (np.float64, np.float32):
                fs = fr.stored(f, dtype)
                assert fr.classify(fs, W, H) == "ok", (name, H, W, dtype)
        f = matrix_fields(rng, H, W)
        assert abs(sum(fr.neighbour_differences(f["sinusoid_bound"])) - fr.NEIGHBOUR_BOUND) <= 1e-9
        outside = np.mean((np.arange(W)[None, :] + f["third_outside"][0] >= W) | (np.arange(H)[:, None] + f["third_outside"][1] < 0))
        assert outside >= 0.3, outside
    H, W = 27, 39
    rng = np.random.default_rng(1)
    v = rng.standard_normal((2, H, W))
    for name, f in matrix_fields(rng, H, W).items():
        lit = np.stack([(fr.warp_matrix(f, W, H).T @ v[c].ravel()).reshape(H, W) for c in range(2)])
        assert np.max(np.abs(fr.gather_adjoint(f, v) - lit)) <= 1e-13, name
    H, W = 96, 128
    extra = {"table": fr.table_fields(H, W, ar.TABLE_SHIFTS),
             "sinusoid": fr.at_bound(fr.sinusoid(H, W, 1.0, 40.0, offset=(-20.3, 7.6)), 0.245)[None],
             "rotation": fr.from_affine([ar.rotation_about_centre(7.0, (0, 0), W, H, 1.02)], H, W)}
    for name, fields in extra.items():
        for f in fields:
            assert fr.classify(f, W, H) == "ok", name
            print("%s: largest seed distance %d" % (name, fr.max_seed_distance(f, W, H)))


def test_a_folded_field_a_nan_and_an_oversize_displacement_are_refused():
    H, W = 24, 36
    assert fr.classify(fr.folded(H, W), W, H) == "eunsupported"
    assert fr.window_violations(fr.folded(H, W), W, H) > 0
    f = np.zeros((2, H, W))
    f[1, 3, 4] = np.nan
    assert fr.classify(f, W, H) == "einval"
    f[1, 3, 4] = 2.0 ** 20 + 1
    assert fr.classify(f, W, H) == "eunsupported"
    f[1, 3, 4] = 2.0 ** 20  # a single far pixel samples outside the image: no pair, nothing to miss
    assert fr.classify(f, W, H) == "ok"
    # a shear beyond the window: neighbour differences of 0.9 px along x
    qx = np.arange(W, dtype=np.float64)[None, :] + np.zeros((H, 1))
    assert fr.classify(np.stack([-0.9 * qx, np.zeros((H, W))]), W, H) == "eunsupported"


@pytest.fixture(scope="module")
def table():
    return fr.table_inputs()


def _solve(T, model, y, **kw):
    x, rep, _ = rr.irls_solve(model, y, rr.bilinear(y[0], T["s"]), reg=T["reg"], composed=True, **kw)
    return orc.psnr(T["gt"], x), (rep.irls_rounds, rep.cg_iterations, rep.nfev)


def test_the_pinned_table(table):
    """Re-derives fr.TABLE.  The counts and the last digits are pinned for the reference's ALGLIB (oracle/_ref); with the
    oracle's own mincg the PSNR conditions below still hold and the pins are compared at 0.05 dB."""
    T = table
    dx, dy = fr.neighbour_differences(T["fields"])
    assert abs(max(dx, dy) - 0.147) <= 1e-3
    got = {"bilinear": (orc.psnr(T["gt"], rr.bilinear(T["y"][0], T["s"])), None),
           "translation_l2": _solve(T, T["translation_model"], T["y"]),
           "translation_huber": _solve(T, T["translation_model"], T["y"], loss="huber", delta=T["delta"]),
           "flow_l2": _solve(T, T["model"], T["y"]),
           "flow_huber": _solve(T, T["model"], T["y"], loss="huber", delta=T["delta"]),
           "flow_lbfgs": _solve(T, T["model"], T["y"], solver="lbfgs", m=5),
           "undeformed_l2": _solve(T, T["translation_model"], T["y_undeformed"])}
    for name, (ps, counts) in got.items():
        print("%-18s %.3f dB %s (pinned %.3f dB %s)" % (name, ps, counts, fr.TABLE[name][0], fr.TABLE[name][1]))
    alglib = orc.have_ref()
    for name, (ps, counts) in got.items():
        assert abs(ps - fr.TABLE[name][0]) <= (0.002 if alglib else 0.05), name
        if alglib:
            assert counts == fr.TABLE[name][1], name
    assert got["flow_l2"][0] >= got["translation_l2"][0] + 5.0
    assert abs(got["flow_l2"][0] - 38.03) <= 0.3 and abs(got["undeformed_l2"][0] - 38.03) <= 0.01
    assert got["translation_huber"][0] < got["flow_l2"][0]
