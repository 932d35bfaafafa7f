"""csrc/model_tables.hpp, the host arithmetic of problem creation (tests/cpp/model_tables_test.cpp), CPU only, against the
oracle's restatement of the same OpenCV parameter arithmetic (oracle.warp_tables / nearest_map / gaussian_kernel).

The integer tables must be equal.  The Gaussian taps must be equal as doubles: both sides restate one expression in the
same order, the oracle's exp is the C library's and so is the header's, and neither build contracts a * b + c.  What the
header derives from the tables (the tap record of make_warp, the maps_regular predicate) is compared with the same
derivation made here from the ORACLE's tables."""
import os
import subprocess

import numpy as np
import pytest

import oracle as orc

SIZES = (1, 2, 7, 32, 33)
SCALES = (1, 2, 3)
SHIFTS = (0.0, 0.5, -0.5, 1.0 / 64, 1.0 / 64 + 1e-13, -3.96875, 15999.5)
# dy within rounding of a 1/32-px quantisation tie (-15.5 / 1024 + 1e-16, found by scanning the oracle's y table over
# (n + 1/2) / 1024 +- 1e-16 ... 1e-13): row 0 lands on one side of the tie, every later row on the other
TIE_DY = -0.0151367187499999
GAUSS_SIZES = (1, 3, 5, 9)
GAUSS_SIGMAS = (0.5, 1.0, 2.5)


def _run(lines):
    import __graft_entry__ as ge
    exe = ge.build_model_tables_test()
    assert exe and os.path.exists(exe)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stdout[-500:], out.stderr[-500:])
    rows = out.stdout.rstrip("\n").split("\n")
    assert len(rows) == len(lines)
    return [r.split() for r in rows]


def _bits(values):
    return np.asarray(values, dtype=np.float64).view(np.int64)


def _warp_cases():
    cases = [(W, H, dx, dy) for W in SIZES for H in SIZES for dx in SHIFTS for dy in SHIFTS if (dx == SHIFTS[0] or dy == dx or W == H)]
    return cases + [(W, H, dx, TIE_DY) for W in SIZES for H in SIZES for dx in (0.0, 0.25)]


def test_warp_tables_equal_the_oracle():
    cases = _warp_cases()
    rows = _run(["wt %d %d %s %s" % (W, H, float(dx).hex(), float(dy).hex()) for W, H, dx, dy in cases])
    for (W, H, dx, dy), row in zip(cases, rows):
        X, Y = orc.warp_tables(W, H, dx, dy)
        got = np.array([int(t) for t in row])
        assert np.array_equal(got[:W], X) and np.array_equal(got[W:], Y), (W, H, dx, dy)


def _taps_from_tables(X, Y):
    """What make_warp derives, from the oracle's tables: (ox, oy, ntaps, fx, w[4] as the float32 BilinearTab_f products,
    y table or [])."""
    H = len(Y)
    fx, fy = int(X[0]) & 31, int(Y[0]) & 31
    tx1 = np.float32(fx) * np.float32(1.0 / 32)
    ty1 = np.float32(fy) * np.float32(1.0 / 32)
    tx0, ty0 = np.float32(1) - tx1, np.float32(1) - ty1
    w = [ty0 * tx0, ty0 * tx1, ty1 * tx0, ty1 * tx1]
    assert all(isinstance(v, np.float32) for v in w)
    uniform = np.array_equal(Y, Y[0] + 32 * np.arange(H))
    ntaps = 1 if (fx == 0 and fy == 0 and uniform) else 4
    return int(X[0]) >> 5, int(Y[0]) >> 5, ntaps, fx, [float(v) for v in w], ([] if uniform else [int(v) for v in Y])


def test_make_warp_equals_the_derivation_from_the_oracle_tables():
    cases = _warp_cases()
    rows = _run(["mw %d %d %s %s" % (W, H, float(dx).hex(), float(dy).hex()) for W, H, dx, dy in cases])
    for (W, H, dx, dy), row in zip(cases, rows):
        X, Y = orc.warp_tables(W, H, dx, dy)
        ox, oy, ntaps, fx, w, ytab = _taps_from_tables(X, Y)
        assert np.array_equal(X, X[0] + 32 * np.arange(W))  # a pure translation: the x table is uniform
        assert [int(t) for t in row[:5]] == [0, ox, oy, ntaps, fx], (W, H, dx, dy)
        assert np.array_equal(_bits([float.fromhex(t) for t in row[5:9]]), _bits(w)), (W, H, dx, dy)
        assert int(row[9]) == len(ytab) and [int(t) for t in row[10:]] == ytab, (W, H, dx, dy)


def test_the_quantisation_tie_gives_both_sides_the_same_non_uniform_y_table():
    for H in SIZES[1:]:
        X, Y = orc.warp_tables(7, H, 0.25, TIE_DY)
        assert not np.array_equal(Y, Y[0] + 32 * np.arange(H)), H
        row = _run(["mw 7 %d %s %s" % (H, (0.25).hex(), TIE_DY.hex())])[0]
        assert int(row[0]) == 0 and int(row[3]) == 4 and int(row[9]) == H
        assert np.array_equal(np.array([int(t) for t in row[10:]]), Y), H


def test_make_warp_refuses_a_shift_of_16000():
    rows = _run(["mw 7 7 %s 0" % (16000.0).hex(), "mw 7 7 0 %s" % (-16000.0).hex(), "mw 7 7 nan 0", "mw 7 7 %s %s" % ((15999.5).hex(), (-15999.5).hex())])
    assert [int(r[0]) for r in rows] == [1, 1, 1, 0]


def _size_cases():
    return [(n, s) for n in SIZES for s in SCALES if orc.downsampled_len(n, s) >= 1]


def test_nearest_map_equals_the_oracle():
    assert (7, 2) in _size_cases() and (32, 3) in _size_cases()  # sizes that are no multiple of the scale
    cases = []
    for n, s in _size_cases():
        m = orc.downsampled_len(n, s)
        cases += [(n, m), (m, n), (m * s, m), (m, m * s)]  # decimation, the NN upsampling, and both on the transpose's size
    rows = _run(["nm %d %d" % c for c in cases])
    for (src, dst), row in zip(cases, rows):
        assert np.array_equal(np.array([int(t) for t in row]), orc.nearest_map(src, dst)), (src, dst)


def test_maps_regular_equals_the_derivation_from_the_oracle_maps():
    cases = [(W, H, s) for W, s in _size_cases() for H in SIZES if orc.downsampled_len(H, s) >= 1]
    rows = _run(["mr %d %d %d" % c for c in cases])
    seen = set()
    for (W, H, s), row in zip(cases, rows):
        w, h = orc.downsampled_len(W, s), orc.downsampled_len(H, s)
        want = (W == w * s and H == h * s
                and np.array_equal(orc.nearest_map(W, w), s * np.arange(w)) and np.array_equal(orc.nearest_map(H, h), s * np.arange(h))
                and np.array_equal(orc.nearest_map(w, W), np.arange(W) // s) and np.array_equal(orc.nearest_map(h, H), np.arange(H) // s))
        assert int(row[0]) == int(want), (W, H, s)
        seen.add(bool(want))
    assert seen == {True, False}


@pytest.mark.parametrize("sigma", GAUSS_SIGMAS)
def test_gaussian_kernel_equals_the_oracle_bit_for_bit(sigma):
    rows = _run(["gk %d %s" % (b, float(sigma).hex()) for b in GAUSS_SIZES])
    for b, row in zip(GAUSS_SIZES, rows):
        got = np.array([float.fromhex(t) for t in row])
        k1, k2 = orc.gaussian_kernel(b, sigma)
        assert np.array_equal(_bits(got[:b]), _bits(k1)) and np.array_equal(_bits(got[b:]), _bits(k2.ravel())), (b, sigma)
