"""CPU checks of the robust data term's CHECKER (tests/robust_restatement.py) and of the library's new boundary: the
composed weighted data term against the oracle's own, the Python IRLS loop against the oracle's solve, the gradient
against finite differences, what the Huber loss buys on the two outlier inputs, and the six new symbols."""
import os
import re
import sys

import numpy as np
import pytest

import oracle as orc

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_restatement as rr  # noqa: E402

NEW_SYMBOLS = ["srmap_set_data_weights", "srmap_set_data_weights_device", "srmap_get_data_weights",
               "srmap_problem_set_data_loss", "srmap_update_data_weights_device"]
NEW_NAMES = NEW_SYMBOLS + ["srmap_data_loss"]  # the sixth: the loss enum


def test_library_exports_and_header_declares_the_robust_entry_points():
    import __graft_entry__ as ge
    ge.build_lib()
    import srmap
    lib = srmap.load()
    text = open(os.path.join(ROOT, "include", "srmap.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
        assert name in srmap.EXPORTED_SYMBOLS
    assert re.search(r"SRMAP_DATA_LOSS_L2\s*=\s*0\s*,\s*SRMAP_DATA_LOSS_HUBER\s*=\s*1\s*}\s*srmap_data_loss\s*;", code)
    assert (srmap.DATA_LOSS_L2, srmap.DATA_LOSS_HUBER) == (0, 1)
    # every new entry point says that the reference has nothing like it
    for name in NEW_SYMBOLS:
        at = text.index("int %s(" % name)
        comment = text[text.rindex("/*", 0, at):at]
        assert "no reference counterpart" in comment.lower(), name


@pytest.mark.parametrize("scale", [2, 3, 4])
@pytest.mark.parametrize("blur", [0, 3])
@pytest.mark.parametrize("subpixel", [False, True])
def test_composed_data_term_with_unit_weights_equals_the_oracle(scale, blur, subpixel):
    rng = np.random.default_rng(100 * scale + 10 * blur + subpixel)
    K, C, h, w = 5, 2, 11, 13
    H, W = h * scale, w * scale
    if subpixel:
        shifts = [[0, 0]] + [[float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2))] for _ in range(K - 1)]
    else:
        shifts = [[0, 0]] + [[int(rng.integers(-2, 3)), int(rng.integers(-2, 3))] for _ in range(K - 1)]
    model = orc.ImageModel(scale=scale, shifts=shifts, blur_ksize=blur, blur_sigma=1.0 if blur else 0.0)
    y = rng.random((K, C, h, w))
    x = rng.random((C, H, W))
    f_ref, g_ref = orc.Problem(model, y).data_term(x)
    for wts in (None, np.ones_like(y)):
        f, g = rr.weighted_data_term(model, y, wts, x)
        ef = abs(f - f_ref) / max(1.0, abs(f_ref))
        eg = np.max(np.abs(g - g_ref) / np.maximum(1.0, np.abs(g_ref)))
        print("scale %d blur %d subpixel %d: cost %.2e gradient %.2e" % (scale, blur, subpixel, ef, eg))
        assert ef <= 1e-12 and eg <= 1e-12


def test_weighted_gradient_matches_finite_differences():
    rng = np.random.default_rng(5)
    s, K, C, h, w = 2, 4, 1, 9, 10
    shifts = [[0, 0], [1.25, -0.5], [0, 1], [-0.75, 0.3]]
    model = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=3, blur_sigma=1.0)
    y = rng.random((K, C, h, w))
    wts = 2.0 * rng.random(y.shape)
    wts[2] = 0.0
    x = rng.random((C, h * s, w * s))
    _, g = rr.weighted_data_term(model, y, wts, x)
    eps = 1e-6
    worst = 0.0
    for idx in rng.choice(x.size, 40, replace=False):
        d = np.zeros(x.size)
        d[idx] = eps
        fp, _ = rr.weighted_data_term(model, y, wts, x + d.reshape(x.shape), want_grad=False)
        fm, _ = rr.weighted_data_term(model, y, wts, x - d.reshape(x.shape), want_grad=False)
        worst = max(worst, abs((fp - fm) / (2 * eps) - g.ravel()[idx]))
    print("worst central-difference deviation %.3e" % worst)
    assert worst <= 1e-6  # the cost is quadratic: the central difference is exact up to rounding (~1e-16 * f / eps)


def test_huber_weights():
    r = np.array([0.0, 0.01, -0.02, 0.02, 0.04, -0.08, 1.0])
    w = rr.huber_weights(r, 0.02)
    assert np.array_equal(w[:4], np.ones(4))
    assert np.allclose(w[4:], [0.5, 0.25, 0.02], rtol=1e-15)


@pytest.fixture(scope="module")
def proto():
    return rr.prototype_inputs()


@pytest.fixture(scope="module")
def l2_solves(proto):
    out = {}
    for name, y, _ in proto["inputs"]:
        x0 = rr.bilinear(y[0], proto["s"])
        out[name] = rr.irls_solve(proto["model"], y, x0, reg=proto["reg"])
    return out


@pytest.mark.parametrize("which", [0, 1, 2])
def test_l2_python_loop_equals_the_oracle_solve(proto, l2_solves, which):
    name, y, _ = proto["inputs"][which]
    x0 = rr.bilinear(y[0], proto["s"])
    p = orc.Problem(proto["model"], y)
    p.add_regularizer(*proto["reg"])
    x_ref, rep_ref = p.solve(x0, None, use_alglib=orc.have_ref())
    x, rep, _ = l2_solves[name]
    print("%s: rounds %d/%d iterations %d/%d evaluations %d/%d, PSNR %.3f dB, max |dx| %.2e" % (
        name, rep.irls_rounds, rep_ref.irls_rounds, rep.cg_iterations, rep_ref.cg_iterations, rep.nfev, rep_ref.nfev,
        orc.psnr(proto["gt"], x), np.max(np.abs(x - x_ref))))
    assert (rep.irls_rounds, rep.cg_iterations, rep.nfev) == (rep_ref.irls_rounds, rep_ref.cg_iterations, rep_ref.nfev)
    assert np.array_equal(x, x_ref)


@pytest.mark.parametrize("which", [1, 2])
def test_huber_beats_l2_by_10_db_on_the_outlier_inputs(proto, l2_solves, which):
    """Measured with the reference's ALGLIB as inner solver: 27.7 dB (salt-and-pepper) and 14.9 dB (misregistered
    frame); the bar leaves the smaller one a third of its size."""
    name, y, _ = proto["inputs"][which]
    x0 = rr.bilinear(y[0], proto["s"])
    x_l2 = l2_solves[name][0]
    x_h, rep, _ = rr.irls_solve(proto["model"], y, x0, reg=proto["reg"], loss="huber", delta=proto["delta"])
    p_l2, p_h = orc.psnr(proto["gt"], x_l2), orc.psnr(proto["gt"], x_h)
    print("%s: bilinear %.2f dB, L2 %.2f dB, Huber %.2f dB (%d rounds / %d iterations / %d evaluations)" % (
        name, orc.psnr(proto["gt"], x0), p_l2, p_h, rep.irls_rounds, rep.cg_iterations, rep.nfev))
    assert p_h >= p_l2 + 10.0
