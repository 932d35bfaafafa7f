"""The regularisers' two gradient modes on the CPU (tests/reg_exact_restatement.py): the restatement's reference mode
against the oracle, its exact mode against central differences of its own cost -- and the reference mode FAILING that
check --, the properties the modes differ by, and the solve table of tests/golden/reg_exact_table.json."""
import itertools
import json
import os

import numpy as np
import pytest

import oracle as orc
import reg_exact_restatement as rx
from conftest import GOLDEN

KINDS = [(rx.TV, 0, 0.0), (rx.TV3D, 0, 0.0)] + [(rx.BTV, R, 0.5 if R != 2 else 0.7) for R in (1, 2, 3, 4)]
FD_SHAPES = [(1, 3, 4), (1, 9, 11), (2, 6, 7)]


def _ids(k):
    return {rx.TV: "tv", rx.TV3D: "tv3d", rx.BTV: "btv"}[k[0]] + (str(k[1]) if k[0] == rx.BTV else "")


def _weights(rng, shape, weighted):
    return 0.5 + rng.random(shape) if weighted else np.ones(shape)


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("kind", KINDS, ids=_ids)
def test_reference_mode_is_the_oracle(kind, C, weighted):
    k, R, decay = kind
    rng = np.random.default_rng(11 + 7 * C + R)
    s, h, w, K = 2, 5, 6, 2
    H, W = h * s, w * s
    lam = 0.03
    x = rng.random((C, H, W))
    wts = _weights(rng, (C, H, W), weighted)
    model = orc.ImageModel(scale=s, shifts=[[0, 0], [1, 0]], blur_ksize=3, blur_sigma=1.0)
    ref = orc.Problem(model, rng.random((K, C, h, w)))
    ref.add_regularizer(k, lam, R, decay)
    ref.set_irls_weights(0, wts)
    f_ref, g_ref = ref.reg_term(0, x)
    vals, g = rx.gradient(k, x, lam * wts, rx.REFERENCE, R, decay)
    f = rx.cost(k, x, lam * wts, R, decay)
    assert np.max(np.abs(vals - orc.reg_values(k, x, R, decay))) <= 1e-12
    assert abs(f - f_ref) <= 1e-12 * max(1.0, abs(f_ref))
    assert np.max(np.abs(g - g_ref.reshape(g.shape))) <= 1e-12 * max(1.0, np.max(np.abs(g_ref)))


def _fd_case(kind, shape, weighted, seed):
    k, R, decay = kind
    rng = np.random.default_rng(seed)
    x = rx.separated_point(rng, shape)
    c = 0.02 * _weights(rng, shape, weighted)
    # the condition of the check: no tap difference within 1e-3 of a sign change (eps = 1e-6 moves none across zero)
    assert rx.min_tap_difference(k, x, R) >= 1e-3
    return x, c, rx.central_differences(k, x, c, R, decay, eps=1e-6)


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weights"])
@pytest.mark.parametrize("shape", FD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS, ids=_ids)
def test_exact_mode_is_the_gradient_of_the_cost(kind, shape, weighted):
    k, R, decay = kind
    x, c, fd = _fd_case(kind, shape, weighted, 100 + R + 10 * shape[1])
    _, g = rx.gradient(k, x, c, rx.EXACT, R, decay)
    err = np.max(np.abs(g - fd))
    print("kind %d R %d shape %s: |g - fd| = %.3e, max|g| = %.3e" % (k, R, shape, err, np.max(np.abs(g))))
    assert err <= 1e-7 * np.max(np.abs(g))


# one channel: 3-D TV is TV there, whose reference gradient is exact
FAIL_CASES = [(k, s) for k in KINDS if k[0] != rx.TV for s in FD_SHAPES if not (k[0] == rx.TV3D and s[0] == 1)]


@pytest.mark.parametrize("kind,shape", FAIL_CASES, ids=[_ids(k) + "-" + "x".join(map(str, s)) for k, s in FAIL_CASES])
def test_reference_mode_fails_the_same_check(kind, shape):
    """the finite-difference check discriminates: the reference's BTV and 3-D TV gradients are not the cost's"""
    k, R, decay = kind
    x, c, fd = _fd_case(kind, shape, True, 100 + R + 10 * shape[1])
    _, g = rx.gradient(k, x, c, rx.REFERENCE, R, decay)
    assert np.max(np.abs(g - fd)) > 1e-7 * np.max(np.abs(fd))
    assert np.max(np.abs(g - fd)) > 1e-2 * np.max(np.abs(fd))  # not by rounding: by a sizeable part of the gradient


def test_btv_range_1_reference_gradient_is_zero():
    rng = np.random.default_rng(3)
    x = rng.random((2, 7, 9))
    c = 0.02 * (0.5 + rng.random(x.shape))
    vals, g_ref = rx.gradient(rx.BTV, x, c, rx.REFERENCE, 1, 0.5)
    _, g_ex = rx.gradient(rx.BTV, x, c, rx.EXACT, 1, 0.5)
    assert np.max(vals) > 0 and rx.cost(rx.BTV, x, c, 1, 0.5) > 0  # the cost counts the regulariser ...
    assert np.all(g_ref == 0.0)                                      # ... and the reference's gradient ignores it
    assert np.max(np.abs(g_ex)) > 1e-3


def test_tv_modes_are_equal():
    rng = np.random.default_rng(4)
    x = rng.random((3, 8, 5))
    c = 0.02 * (0.5 + rng.random(x.shape))
    a, b = rx.gradient(rx.TV, x, c, rx.REFERENCE), rx.gradient(rx.TV, x, c, rx.EXACT)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_tv3d_modes_differ_by_the_z_self_term():
    rng = np.random.default_rng(5)
    x = rng.random((3, 6, 7))
    c = 0.02 * (0.5 + rng.random(x.shape))
    r, g_ref = rx.gradient(rx.TV3D, x, c, rx.REFERENCE)
    _, g_ex = rx.gradient(rx.TV3D, x, c, rx.EXACT)
    want = np.zeros_like(x)
    want[:-1] = -2.0 * c[:-1] * r[:-1] * np.sign(x[1:] - x[:-1])
    assert np.array_equal(g_ex, g_ref + want)  # exactly: one more term, added last
    assert np.any(want != 0.0) and np.array_equal(g_ex[-1], g_ref[-1])  # the last channel has no next one


@pytest.mark.parametrize("R", [1, 2, 3])
def test_corner_pixel_is_a_source_in_exact_mode_only(R):
    x = rx.corner_image((1, 6, 7))
    c = np.full(x.shape, 0.02)
    _, g_ref = rx.gradient(rx.BTV, x, c, rx.REFERENCE, R, 0.5)
    _, g_ex = rx.gradient(rx.BTV, x, c, rx.EXACT, R, 0.5)
    # only r[0,0] is non-zero; its taps (i, j) in [0, R]^2 are the neighbours it is a source for
    nb_ref = g_ref.copy(); nb_ref[0, 0, 0] = 0.0
    assert np.all(nb_ref == 0.0)
    for i, j in itertools.product(range(R + 1), repeat=2):
        if (i, j) != (0, 0):
            assert g_ex[0, i, j] < 0.0, (i, j)  # x[0,0] lies above them: the cost falls as they rise
    outside = g_ex.copy(); outside[0, :R + 1, :R + 1] = 0.0
    assert np.all(outside == 0.0)
    fd = rx.central_differences(rx.BTV, x + 0.0, c, R, 0.5)
    # the constant part of the image sits on sign changes; at the window of (0, 0) the differences are 0.4: compare there
    assert np.max(np.abs(g_ex - fd)[0, :R + 1, :R + 1]) <= 1e-7 * np.max(np.abs(g_ex))


# ---- the solve table ----
# What tests/golden/make_reg_exact_table.py measured (CG; dB gained by the exact gradient, evaluations exact / reference):
MEASURED_GAIN = {(1, 0.005): 12.77, (1, 0.02): 10.82, (2, 0.005): 1.40, (2, 0.02): 0.44}
MEASURED_EVAL_RATIO = {(2, 0.005): 133 / 204, (2, 0.02): 91 / 102}
MARGIN_DB = 0.25


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "reg_exact_table.json")) as f:
        t = json.load(f)
    assert [(r["range"], r["lambda"]) for r in t["rows"]] == rx.TABLE_ROWS
    return t


@pytest.fixture(scope="module")
def table_inputs():
    return rx.table_inputs()


@pytest.mark.parametrize("row", range(len(rx.TABLE_ROWS)), ids=["R%d-lambda%g" % rl for rl in rx.TABLE_ROWS])
def test_solve_table_row(table, table_inputs, row):
    """A row of the golden table re-solved by CG with both gradients: the PSNR within ten times what moving the
    observations by 1e-13 moved it (1e-6 dB at least), the counts where the generator found them stable; then what the
    generator measured, with 0.25 dB of margin: the gain at R 1 and R 2 and the evaluation ratio at R 2.  Nothing is
    asserted of the gain at R 3."""
    R, lam = rx.TABLE_ROWS[row]
    r = table["rows"][row]
    got = {}
    for name, mode in (("reference", rx.REFERENCE), ("exact", rx.EXACT)):
        want = r["cg_" + name]
        psnr, counts = rx.table_solve(table_inputs, R, lam, mode)
        print("R %d lambda %g %s: %.3f dB %s (table %.3f %s, stable %s)" % (R, lam, name, psnr, counts, want["psnr"], want["counts"], want["stable"]))
        assert abs(psnr - want["psnr"]) <= max(10.0 * want["psnr_moved_by"], 1e-6)
        if want["stable"]:
            assert counts == want["counts"]
        got[name] = (psnr, counts)
    gain = got["exact"][0] - got["reference"][0]
    if R in (1, 2):
        assert gain >= MEASURED_GAIN[(R, lam)] - MARGIN_DB > 0.0
    if R == 1:
        # the reference's gradient is zero: its solve fits the noise unregularised and ends BELOW the start
        assert got["reference"][0] < table["start_psnr"] - MARGIN_DB < got["exact"][0]
    if R == 2:
        assert r["cg_reference"]["stable"] and r["cg_exact"]["stable"]
        ratio = got["exact"][1][2] / got["reference"][1][2]
        assert ratio == MEASURED_EVAL_RATIO[(R, lam)] and ratio < 1.0


def test_solve_table_file_holds_results_only(table):
    assert sorted(table) == ["amplitude", "decay", "rows", "solver", "start_psnr"]
    for r in table["rows"]:
        for solver in ("cg", "lbfgs"):
            for name in ("reference", "exact"):
                assert sorted(r[solver + "_" + name]) == ["counts", "psnr", "psnr_moved_by", "stable"]
