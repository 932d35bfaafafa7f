"""The residual scale without a GPU (include/srmap.h: srmap_residual_scale, srmap_problem_set_huber_scale):
the digit passes of csrc/select_host.hpp -- restated in numpy (tests/residual_scale_restatement.py) and run in plain C++
(tests/cpp/residual_scale_test.cpp) -- against np.partition, bit for bit; the Lipschitz property the GPU bars rest on; and
the automatic Huber delta's figures on the README's inputs."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle as orc
from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import residual_scale_restatement as rs  # noqa: E402
import robust_restatement as rr  # noqa: E402

NEW_SYMBOLS = ("srmap_problem_set_huber_scale", "srmap_problem_get_huber_delta", "srmap_residual_scale",
               "srmap_residual_scale_device")


def test_library_exports_and_header_declares_the_entry_points():
    import __graft_entry__ as ge
    ge.build_lib()
    import srmap
    lib = srmap.load()
    text = open(os.path.join(ROOT, "include", "srmap.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in srmap.EXPORTED_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "SRMAP_HUBER_DELTA_FIXED = 0, SRMAP_HUBER_DELTA_MAD = 1" in text
    assert (srmap.HUBER_DELTA_FIXED, srmap.HUBER_DELTA_MAD) == (0, 1)


def _bits(v):
    v = np.asarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _cases(dtype):
    """[(name, values, mask or None)]: every pattern at an even and an odd size, n = 1, 2, 3, and masks that leave 0, 1,
    some and all elements."""
    out = []
    for n in (64, 257):
        rng = np.random.default_rng(n)
        for name, v in rs.patterns(dtype, n, rng).items():
            out.append(("%s n=%d" % (name, n), v, None))
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 4, 5):
        out.append(("n=%d" % n, rng.standard_normal(n).astype(dtype), None))
        out.append(("n=%d equal" % n, np.full(n, -2.5, dtype=dtype), None))
    v = rng.standard_normal(101).astype(dtype)
    one = np.zeros(101)
    one[17] = 1.0
    for name, m in (("mask none", np.zeros(101)), ("mask one", one), ("mask random", (rng.random(101) < 0.5).astype(float)),
                    ("mask all", np.ones(101)), ("mask of weights", rng.random(101) * (rng.random(101) < 0.7))):
        out.append((name, v, m))
    out.append(("NaNs above +inf", np.array([np.nan, np.inf, 1.0, np.nan, np.nan], dtype=dtype), None))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_digit_passes_equal_partition(dtype):
    for name, v, m in _cases(dtype):
        want, n = rs.lower_median(v, m)
        got, n2 = rs.radix_lower_median(v, m)
        assert n == n2 == (v.size if m is None else int(np.sum(m > 0))), name
        assert _bits(got) == _bits(want), (name, got, want)
        if n and not np.any(np.isnan(v)):  # an element of the input, of rank (n - 1) // 2, never an average
            a = np.sort(rs.counted(v, m))
            assert want == a[(n - 1) // 2] and want in a, name
        if n == 0:
            assert want == 0
    # more than half zeros: exactly 0
    z = np.zeros(11, dtype=dtype)
    z[:5] = [1, -2, 3, -4, 5]
    assert rs.radix_lower_median(z) == (0, 11) and rs.radix_lower_median(z[:10])[0] == 0
    assert rs.radix_lower_median(np.array([3, 1], dtype=dtype))[0] == 1  # the LOWER median of two


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cpp_passes_equal_nth_element_and_partition(dtype):
    """tests/cpp/residual_scale_test.cpp runs select_host.hpp's passes; it exits non-zero itself when they disagree with
    std::nth_element.  Its key, count, scale and delta against numpy, bit for bit."""
    import __graft_entry__ as ge
    exe = ge.build_residual_scale_test()
    assert exe and os.path.exists(exe)
    cases = _cases(dtype)
    lines = []
    for name, v, m in cases:
        mm = np.ones(v.size) if m is None else m
        lines.append("%s %d %s" % ("f32" if dtype == np.float32 else "f64", v.size,
                                   " ".join("%x %d" % (int(b), int(k > 0)) for b, k in zip(_bits(v), mm))))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-300:], out.stderr[-300:])
    rows = out.stdout.strip().split("\n")
    assert len(rows) == len(cases)
    for (name, v, m), row in zip(cases, rows):
        key, n, scale, delta = row.split()
        want, nw = rs.lower_median(v, m)
        assert int(n) == nw, name
        assert int(key, 16) == (int(_bits(np.abs(want))) if nw else 0), name
        ws = rs.MAD_TO_SIGMA * float(want)
        assert float.fromhex(scale) == ws or (np.isnan(ws) and np.isnan(float.fromhex(scale))), name
        assert float.fromhex(delta) == rs.mad_delta(ws, 1.345, 1e-4), name


def test_order_statistic_is_1_lipschitz():
    """|median(|r + e|) - median(|r|)| <= max |e|: every order statistic moves by at most the largest perturbation.  The
    GPU bars on a general x rest on this: the scale inherits the residuals' own parity bar, times 1.4826."""
    rng = np.random.default_rng(0)
    for n in (1, 2, 7, 100, 1001):
        for eps in (1e-12, 1e-6, 1e-2, 1.0):
            r = rng.standard_normal(n)
            mask = (rng.random(n) < 0.7).astype(float) if n > 2 else None
            for e in (eps * (2 * rng.random(n) - 1), np.full(n, eps), eps * np.sign(rng.standard_normal(n))):
                moved = r + e
                a, b = rs.lower_median(r, mask)[0], rs.lower_median(moved, mask)[0]
                assert abs(float(a) - float(b)) <= np.max(np.abs(moved - r)) * (1 + 1e-15), (n, eps)  # the perturbation as rounded


def test_scales_of_a_stack():
    rng = np.random.default_rng(5)
    r = rng.standard_normal((4, 2, 5, 7))
    mask = (rng.random(r.shape) < 0.6).astype(float)
    mask[2] = 0.0
    s, c = rs.residual_scales(r, mask)
    s2, c2 = rs.residual_scales(r, mask, median=rs.radix_lower_median)
    assert np.array_equal(s, s2) and np.array_equal(c, c2)
    assert s[3] == 0.0 and c[3] == 0.0 and c[0] == mask.sum() and s[0] > 0
    assert s[1] == 1.4826 * np.sort(np.abs(r[0][mask[0] > 0]))[(int(c[1]) - 1) // 2]


# ---------------------------------------------------------------------------------------------- the table
# PSNR in dB of the fixed delta 0.02 and of the MAD rule (tuning 1.345, floor 1e-4), with the inner solver this checkout
# has (the reference's ALGLIB where oracle/_ref is built, else the oracle's mincg).  MIN_GAIN: half of the gains of the
# prototype that proposed the rule (0.43 / 1.47 / 0.72 / 1.87 dB); the gains measured here are 0.43 / 1.42 / 0.77 / 1.88 dB
MIN_GAIN = {"noise": 0.2, "salt_pepper": 0.7, "misregistered": 0.35, "salt_pepper sigma 0.003": 0.9}


@pytest.fixture(scope="module")
def proto():
    P = rr.prototype_inputs()
    P["inputs"] = [(n, y) for n, y, _ in P["inputs"]] + [("salt_pepper sigma 0.003", rs.seed11_input(0.003)),
                                                         ("salt_pepper sigma 0.03", rs.seed11_input(0.03))]
    return P


@pytest.fixture(scope="module")
def solves(proto):
    out = {}
    for name, y in proto["inputs"]:
        x0 = rr.bilinear(y[0], proto["s"])
        xf, rf, _ = rr.irls_solve(proto["model"], y, x0, reg=proto["reg"], loss="huber", delta=proto["delta"])
        xm, rm, _, deltas, frames = rs.irls_solve_mad(proto["model"], y, x0, proto["reg"])
        out[name] = dict(fixed=orc.psnr(proto["gt"], xf), mad=orc.psnr(proto["gt"], xm), rep_fixed=rf, rep_mad=rm, deltas=deltas,
                         frames=frames)
        print("%-26s fixed %.3f dB (%d / %d / %d) | MAD %.3f dB (%d / %d / %d) | delta %.4f -> %.4f | frames %s" % (
            name, out[name]["fixed"], rf.irls_rounds, rf.cg_iterations, rf.nfev, out[name]["mad"], rm.irls_rounds,
            rm.cg_iterations, rm.nfev, deltas[0], deltas[-1], " ".join("%.4f" % f for f in frames)))
    return out


@pytest.mark.parametrize("name", sorted(MIN_GAIN))
def test_mad_delta_gains_over_the_fixed_delta(solves, name):
    s = solves[name]
    assert s["mad"] - s["fixed"] >= MIN_GAIN[name], (name, s["mad"], s["fixed"])
    assert 1e-4 < s["deltas"][-1] < 0.05


def test_sigma_0_03_is_the_stated_limit(solves):
    """Noise 0.03 with lambda 0.005: the regulariser is too weak for this noise, the MAD rule LOSES 2 dB against delta 0.02
    and the IRLS loop runs 18 of its 20 rounds (24.758 dB).  A limit to be stated, not hidden (README, "Residual scale")."""
    s = solves["salt_pepper sigma 0.03"]
    assert s["rep_mad"].irls_rounds == 18
    assert abs(s["fixed"] - 26.748) <= 0.002 and abs(s["mad"] - 24.758) <= 0.002


# as measured, with the reference's ALGLIB and with the oracle's mincg alike (the two give the same figures to every digit
# shown): PSNR fixed, PSNR MAD, (rounds, iterations, evaluations) of MAD
PINNED = {"noise": (38.105, 38.536, (7, 116, 196)), "salt_pepper": (35.830, 37.248, (15, 222, 394)),
          "misregistered": (36.231, 36.999, (13, 143, 243)), "salt_pepper sigma 0.003": (36.643, 38.519, (9, 265, 378))}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_figures(solves, name):
    s, (fixed, mad, counts) = solves[name], PINNED[name]
    assert abs(s["fixed"] - fixed) <= 0.002 and abs(s["mad"] - mad) <= 0.002
    assert (s["rep_mad"].irls_rounds, s["rep_mad"].cg_iterations, s["rep_mad"].nfev) == counts


def test_per_frame_scales_flag_the_misregistered_frame_and_must_not_drive_delta(proto, solves):
    s = solves["misregistered"]
    others = np.delete(s["frames"], 4)
    assert s["frames"][4] >= 2.0 * np.median(others), s["frames"]
    name, y = proto["inputs"][2]
    x0 = rr.bilinear(y[0], proto["s"])
    xp, rp, _, _, _ = rs.irls_solve_mad(proto["model"], y, x0, proto["reg"], per_frame=True)
    per_frame = orc.psnr(proto["gt"], xp)
    print("misregistered: one scale %.3f dB, a delta per frame %.3f dB" % (s["mad"], per_frame))
    assert per_frame <= s["mad"] - 5.0
