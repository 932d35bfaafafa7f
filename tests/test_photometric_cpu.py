"""CPU checks of the photometric frame model's CHECKER (tests/photometric_restatement.py) and of the library's new boundary:
the fit recovers the parameters the frames were generated with (exactly without noise, within the noise's reach with it),
Huber weights make it outlier-robust, the statuses of the per-frame solve, idempotence, the normalisation's rounding, what
the model buys on the README's table input, and the new symbols."""
import os
import re
import sys

import numpy as np
import pytest

import oracle as orc

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import photometric_restatement as pr  # noqa: E402
import robust_restatement as rr  # noqa: E402

# README's table as measured with the reference's ALGLIB (and, bit-equal, the oracle's mincg): PSNR dB, (IRLS rounds, CG
# iterations, evaluations); "rounds": the four solves of solve_photometric(rounds=3) and the PSNR after the last
TABLE = {"ignored": (16.6177, (13, 80, 183)), "true": (38.0949, (7, 116, 178)), "x0_fit": (37.32, (7, 111, 163)),
         "rounds": (37.8369, [(7, 111, 163), (7, 120, 188), (7, 115, 179), (7, 101, 153)]), "cold": (37.89, (7, 116, 214)),
         # the same four solves with the six sums added in another order ("transposed"): the parameters move by ~1e-15 and
         # the LAST solve, run to the default thresholds, ends two iterations later -- the restatement's counts are not
         # unique there.  Capped at 5 IRLS rounds of 20 CG iterations (SOLVE_CAPS, as tests/test_blur_kernel_cpu.py's) they
         # are the same in every order: these are what the GPU end-to-end test must reproduce
         "rounds_other_order": (37.8389, [(7, 111, 163), (7, 120, 188), (7, 115, 179), (7, 103, 155)]),
         "rounds_capped": (37.8317, [(5, 98, 139), (5, 98, 145), (5, 95, 141), (5, 94, 137)])}
SOLVE_CAPS = (5, 20)

NEW_SYMBOLS = ["srmap_problem_set_photometric", "srmap_problem_get_photometric", "srmap_fit_photometric",
               "srmap_fit_photometric_device"]


def test_library_exports_and_header_declares_the_photometric_entry_points():
    import __graft_entry__ as ge
    ge.build_lib()
    import srmap
    lib = srmap.load()
    text = open(os.path.join(ROOT, "include", "srmap.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS + ["srmap_photometric_fit_options_default"]:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
        assert name in srmap.EXPORTED_SYMBOLS
    # the two blocks (the model, the fit) say that the reference has nothing like them
    for opening, name in (("/* Photometric frame model", "srmap_problem_set_photometric"),
                          ("/* Fit of the photometric parameters", "srmap_fit_photometric")):
        block = text[text.index(opening):text.index("int %s(" % name)]
        assert "no reference counterpart" in block.lower(), name
    # the header states the units of the cost
    assert "NOT the maximum-likelihood weighting" in text and "normalised residuals" in text
    fields = [f for f, _ in srmap.PhotometricFitOptions._fields_]
    assert fields == ["struct_size", "model", "gauge_frame", "min_gain", "max_gain", "apply"]


@pytest.fixture(scope="module")
def table():
    return pr.table_inputs()


def test_exact_recovery_without_noise(table):
    """x the ground truth, no noise: the parameters the frames were generated with (measured: gain 4e-15, bias 7e-16)."""
    T = table
    y = pr.apply_photometric(T["clean"], T["truth"])
    gb, q, _ = pr.fit(T["model"], T["gt"], y, gauge_frame=-1)
    eg, eb = np.max(np.abs(gb[:, 0] - T["truth"][:, 0])), np.max(np.abs(gb[:, 1] - T["truth"][:, 1]))
    print("no noise: gain error %.2e, bias error %.2e" % (eg, eb))
    assert np.all(q[:, 3] == pr.STATUS_OK)
    assert eg <= 1e-12 and eb <= 1e-12


def test_recovery_under_noise(table):
    """x the ground truth, noise sigma 0.01, 5 seeds (measured: gain <= 0.0052, bias <= 0.0019)."""
    T = table
    worst_g = worst_b = 0.0
    for seed in range(5):
        y = pr.apply_photometric(T["clean"], T["truth"]) + 0.01 * np.random.default_rng(seed).standard_normal(T["clean"].shape)
        gb, _, _ = pr.fit(T["model"], T["gt"], y, gauge_frame=-1)
        worst_g = max(worst_g, np.max(np.abs(gb[:, 0] - T["truth"][:, 0])))
        worst_b = max(worst_b, np.max(np.abs(gb[:, 1] - T["truth"][:, 1])))
    print("sigma 0.01, 5 seeds: gain error %.4f, bias error %.4f" % (worst_g, worst_b))
    assert worst_g <= 0.01 and worst_b <= 0.004


def test_huber_weights_make_the_fit_robust(table):
    """3 % salt-and-pepper in one frame (the robust table's own mask and values, seed 7), each of the frames 1..5 in turn, on
    noise-free frames -- noise sigma 0.01 alone moves a fit by up to 0.005 (test_recovery_under_noise), more than the bar here.
    The unweighted fit misses (measured: gain 0.007 ... 0.033, bias 0.007 ... 0.016); with the Huber weights (delta 0.02) of
    the normalised residual at that fit it is within 0.002 / 0.002 (measured <= 0.0009 / 0.0003)."""
    T = table
    rng = np.random.default_rng(7)
    rng.standard_normal(T["clean"].shape)  # the table's noise draw comes first
    mask = rng.random(T["clean"].shape) < 0.03
    vals = rng.integers(0, 2, T["clean"].shape).astype(float)
    s = pr.predictions(T["model"], T["gt"], T["K"])
    for k in range(1, T["K"]):
        y = pr.apply_photometric(T["clean"], T["truth"])
        y[k] = np.where(mask[k], vals[k], y[k])
        gb, _, _ = pr.fit(T["model"], T["gt"], y, gauge_frame=-1)
        miss = np.abs(gb[k] - T["truth"][k])
        gbw, _, _ = pr.fit(T["model"], T["gt"], y, w=rr.huber_weights(s - pr.normalise(y, gb), 0.02), gauge_frame=-1)
        hit = np.abs(gbw[k] - T["truth"][k])
        print("frame %d: unweighted gain / bias error %.4f / %.4f, Huber-weighted %.4f / %.4f" % (k, miss[0], miss[1], hit[0], hit[1]))
        assert hit[0] <= 0.002 and hit[1] <= 0.002
        assert miss[0] >= 0.005 and miss[1] >= 0.005
        others = np.delete(np.arange(T["K"]), k)  # a frame's answer is independent of the other frames
        assert np.max(np.abs(gbw[others] - T["truth"][others])) <= 1e-12


def test_gain_only_and_bias_only(table):
    T = table
    gains = np.stack([T["truth"][:, 0], np.zeros(T["K"])], axis=1)
    y = pr.apply_photometric(T["clean"], gains)
    gb, q, _ = pr.fit(T["model"], T["gt"], y, kind=pr.GAIN_ONLY, gauge_frame=-1)
    assert np.max(np.abs(gb - gains)) <= 1e-12 and np.all(q[:, 3] == 0)
    biases = np.stack([np.ones(T["K"]), T["truth"][:, 1]], axis=1)
    y = pr.apply_photometric(T["clean"], biases)
    gb, q, _ = pr.fit(T["model"], T["gt"], y, kind=pr.BIAS_ONLY, gauge_frame=-1)
    assert np.max(np.abs(gb - biases)) <= 1e-12 and np.all(q[:, 3] == 0)
    # the parameter that is not fitted keeps the value in force
    cur = np.tile([1.25, 0.5], (T["K"], 1))
    gb, _, _ = pr.fit(T["model"], T["gt"], y, current=cur, kind=pr.GAIN_ONLY, gauge_frame=-1)
    assert np.array_equal(gb[:, 1], cur[:, 1])
    gb, _, _ = pr.fit(T["model"], T["gt"], y, current=cur, kind=pr.BIAS_ONLY, gauge_frame=-1)
    assert np.array_equal(gb[:, 0], cur[:, 0])


def test_statuses_and_the_gauge(table):
    T = table
    y = pr.apply_photometric(T["clean"], T["truth"])
    w = np.ones_like(y)
    w[3] = 0.0  # a frame without weight
    cur = np.tile([1.5, 0.25], (T["K"], 1))
    gb, q, _ = pr.fit(T["model"], T["gt"], y, w=w, current=cur, gauge_frame=0)
    assert list(q[:, 3]) == [0, 0, 0, 3, 0, 0]
    assert np.array_equal(gb[3], cur[3]) and q[3, 2] == 0.0
    assert np.array_equal(gb[0], cur[0]) and q[0, 0] == q[0, 1]  # the gauge: unchanged, status 0
    # a constant HR image: s is flat, the determinant vanishes
    flat = np.full_like(T["gt"], 0.5)
    interior = np.zeros_like(y)
    interior[:, :, 2:-2, 2:-2] = 1.0  # away from the blur's zero border, where s is exactly constant
    gb, q, _ = pr.fit(T["model"], flat, y, w=interior, current=cur, gauge_frame=-1)
    assert np.all(q[:, 3] == 3) and np.array_equal(gb, cur)
    # a gain beyond the bounds
    gb, q, _ = pr.fit(T["model"], T["gt"], y, current=cur, gauge_frame=-1, max_gain=1.04)
    assert list(q[:, 3]) == [0, 2, 0, 2, 0, 0]
    assert np.array_equal(gb[1], cur[1]) and np.array_equal(gb[3], cur[3]) and q[1, 0] == q[1, 1]
    gb, q, _ = pr.fit(T["model"], T["gt"], y, gauge_frame=-1, min_gain=0.95)
    assert list(q[:, 3]) == [0, 0, 2, 0, 2, 0]


def test_the_fit_is_absolute(table):
    """The fit reads the raw frames: the parameters in force do not move it (they only set E at the start)."""
    T = table
    gb1, q1, S1 = pr.fit(T["model"], T["gt"], T["y"], gauge_frame=-1)
    gb2, q2, S2 = pr.fit(T["model"], T["gt"], T["y"], current=gb1, gauge_frame=-1)
    assert np.array_equal(gb1, gb2) and np.array_equal(S1, S2)
    assert np.array_equal(q2[:, 0], q2[:, 1])  # already at the minimum
    assert np.all(q1[:, 1] <= q1[:, 0])


def test_energy_from_the_sums_is_the_weighted_residual(table):
    T = table
    rng = np.random.default_rng(1)
    w = rng.random(T["y"].shape)
    S = pr.sums(T["model"], T["gt"], T["y"], w)
    s = pr.predictions(T["model"], T["gt"], T["K"])
    for k, (a, b) in enumerate(T["truth"]):
        direct = np.sum(w[k] * (a * s[k] + b - T["y"][k]) ** 2)
        assert abs(pr.energy(S[k], a, b) - direct) <= 1e-12 * S[k, 5]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_normalise_rounds_once(dtype):
    rng = np.random.default_rng(2)
    y = rng.random((3, 2, 5, 7))
    gb = np.array([[1.0, 0.0], [1.08, 0.03], [0.9, -0.02]])
    yn = pr.normalise(y, gb, dtype)
    assert yn.dtype == dtype
    assert np.array_equal(yn[0], y[0].astype(dtype))  # (1, 0) changes nothing
    stored = y.astype(dtype).astype(np.float64)
    for k in range(3):
        assert np.array_equal(yn[k], ((stored[k] - gb[k, 1]) / gb[k, 0]).astype(dtype))


def test_table_what_the_photometric_model_buys(table):
    """README's table, with the reference's ALGLIB as the inner solver where oracle/_ref is built.  Measured: bilinear
    32.53 dB; ignored 16.62 dB (13 / 80 / 183); true parameters 38.09 dB (7 / 116 / 178); fitted from the bilinear x0 alone
    37.32 dB (7 / 111 / 163); after 3 x (fit, warm solve) 37.84 dB; cold solve with those parameters 37.89 dB (7 / 116 / 214);
    largest gain error per fit 0.0240, 0.0183, 0.0134, 0.0095."""
    T = table
    m, y, gt, reg = T["model"], T["y"], T["gt"], T["reg"]
    x0 = rr.bilinear(y[0], T["s"])

    def solve(frames, start=x0):
        x, rep, _ = rr.irls_solve(m, frames, start, reg=reg)
        return orc.psnr(gt, x), (rep.irls_rounds, rep.cg_iterations, rep.nfev)

    ignored, true = solve(y), solve(pr.normalise(y, T["truth"]))
    x, reports, fits = pr.solve_photometric(m, y, x0, reg=reg, rounds=3)
    first = (orc.psnr(gt, rr.irls_solve(m, pr.normalise(y, fits[0][0]), x0, reg=reg)[0]),
             (reports[0].irls_rounds, reports[0].cg_iterations, reports[0].nfev))
    cold = solve(pr.normalise(y, fits[-1][0]))
    gain_err = [float(np.max(np.abs(gb[:, 0] - T["truth"][:, 0]))) for gb, _ in fits]
    print("bilinear %.2f dB; ignored %.2f dB %s; true %.2f dB %s; x0 fit %.2f dB %s; after 3 rounds %.2f dB; cold %.2f dB %s; "
          "gain errors %s" % (orc.psnr(gt, x0), ignored[0], ignored[1], true[0], true[1], first[0], first[1], orc.psnr(gt, x),
                              cold[0], cold[1], np.round(gain_err, 4)))
    counts = [(r.irls_rounds, r.cg_iterations, r.nfev) for r in reports]
    assert counts == TABLE["rounds"][1] and abs(orc.psnr(gt, x) - TABLE["rounds"][0]) <= 0.005
    for name, got in (("ignored", ignored), ("true", true), ("x0_fit", first), ("cold", cold)):
        assert got[1] == TABLE[name][1] and abs(got[0] - TABLE[name][0]) <= 0.006, name
    assert ignored[0] <= true[0] - 15.0
    assert first[0] >= true[0] - 1.0
    assert cold[0] >= true[0] - 0.3
    assert all(b <= a for a, b in zip(gain_err, gain_err[1:]))


def test_capped_solves_keep_their_counts_under_another_summation_order(table):
    """What the GPU end-to-end test pins.  The GPU adds the six sums in its own order, so its parameters differ from the
    restatement's in the last bits; run to the default thresholds that already moves the fourth solve's counts (shown here
    with the restatement's own "transposed" order), capped at SOLVE_CAPS it does not."""
    T = table
    m, y, gt, reg = T["model"], T["y"], T["gt"], T["reg"]
    x0 = rr.bilinear(y[0], T["s"])
    o = orc.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = SOLVE_CAPS
    for order in ("natural", "transposed"):
        x, reports, _ = pr.solve_photometric(m, y, x0, reg=reg, rounds=3, options=o, order=order)
        counts = [(r.irls_rounds, r.cg_iterations, r.nfev) for r in reports]
        print("capped, %s order: %.4f dB %s" % (order, orc.psnr(gt, x), counts))
        assert counts == TABLE["rounds_capped"][1] and abs(orc.psnr(gt, x) - TABLE["rounds_capped"][0]) <= 0.005
    x, reports, _ = pr.solve_photometric(m, y, x0, reg=reg, rounds=3, order="transposed")
    counts = [(r.irls_rounds, r.cg_iterations, r.nfev) for r in reports]
    print("default thresholds, transposed order: %.4f dB %s" % (orc.psnr(gt, x), counts))
    assert counts == TABLE["rounds_other_order"][1] != TABLE["rounds"][1]
    assert abs(orc.psnr(gt, x) - TABLE["rounds_other_order"][0]) <= 0.005 and abs(orc.psnr(gt, x) - TABLE["rounds"][0]) <= 0.01
