"""The translational registration on the GPU (include/srmap.h: srmap_register_translational_ex; k_ssd_candidates and
k_lk_sums of csrc/registration.hip, k_down2_stack of csrc/motion_fit.hip) against its numpy restatement
(tests/registration_restatement.py) on the restatement's case table: widths under one wave and around one thread stride,
every row-chunk count from 1 to the cap of 64 with its empty trailing chunks, the `> 64` level rule, odd sizes, the "too
small to refine" exit, the clamp.  tests/test_registration_cpu.py shows that no decision of a case (argmin, stop, texture
test, clamp, margin) is within rounding of its threshold, so the two runs take the same path and differ by rounding only.

Bars.  Frames that are exact integer translations: shift and RMS are EQUAL (the true shift's error is exactly 0 in both,
tx = ty = 0 samples exactly); so is the separation where the shift is a whole number of pixels of the coarsest level as
well -- elsewhere the coarsest best is a sum of non-zero squares and the separation gets the bar of the other frames.
Every other frame: |shift - restatement| <= max(100 x the restatement's own summation-order sensitivity of that frame,
1e-10 px) -- the floor tests/test_gpu_affine_registration.py uses for sums of the same kind --, separation and RMS within
max(100 x their sensitivity, 1e-12).  Every figure is printed ("PARITY ...") and logged through parity_log.note.

The host facade (registration::TranslationalRegistrationWithQuality against the C call, bit for bit, at 33 x 47 with the
table's shifts) is TestRegistrationWithQuality of tests/cpp/facade_test.cpp, run by tests/test_gpu_facade.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_log  # noqa: E402
import registration_restatement as tr  # noqa: E402

pytestmark = pytest.mark.gpu

SHIFT_FLOOR, QUALITY_FLOOR = 1e-10, 1e-12


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


def compare(name, stack, exact, got, q):
    """Hold every frame of one GPU run to the restatement; prints one line per frame."""
    ref, rq, trace = tr.restated(name)["rows"]
    s_shift, s_sep, s_rms = tr.sensitivity(name)
    H, W = stack.shape[1:]
    assert got.shape == ref.shape and q.shape == rq.shape
    assert np.array_equal(got[0], [0.0, 0.0]) and np.array_equal(q[0], [1.0, 0.0])
    for k in range(1, len(ref)):
        T = trace[k]
        d_shift = float(np.max(np.abs(got[k] - ref[k])))
        d_sep, d_rms = abs(q[k, 0] - rq[k, 0]), abs(q[k, 1] - rq[k, 1])
        b_shift = max(100 * s_shift[k], SHIFT_FLOOR)
        b_sep, b_rms = max(100 * s_sep[k], QUALITY_FLOOR), max(100 * s_rms[k], QUALITY_FLOOR)
        print("PARITY %3d x %3d %-14s frame %d restated (%+.6f, %+.6f) passes %2d: GPU - restatement shift %.2e px (sensitivity "
              "%.1e, bar %.1e), separation %.2e (%.1e, %.1e), rms %.2e (%.1e, %.1e)%s"
              % (H, W, name, k, ref[k, 0], ref[k, 1], len(T["passes"]), d_shift, s_shift[k], b_shift, d_sep, s_sep[k], b_sep,
                 d_rms, s_rms[k], b_rms, "  [exact]" if exact[k] else ""))
        parity_log.note(d_shift, "%s frame %d shift" % (name, k))
        parity_log.note(d_sep, "%s frame %d separation" % (name, k))
        parity_log.note(d_rms, "%s frame %d rms" % (name, k))
        if exact[k]:
            assert np.array_equal(got[k], ref[k]), (name, k, got[k], ref[k])
            assert q[k, 1] == rq[k, 1], (name, k, q[k], rq[k])
            if T["levels"][0]["best"] == 0.0:
                assert q[k, 0] == rq[k, 0], (name, k, q[k], rq[k])
        else:
            assert d_shift <= b_shift, (name, k, got[k], ref[k])
            sx, sy = T["integer"]
            assert abs(got[k, 0] - sx) <= 1.0 and abs(got[k, 1] - sy) <= 1.0  # the same integer part: inside its clamp
        if not T["passes"]:
            assert q[k, 1] == -1.0  # too small to refine
        assert d_sep <= b_sep, (name, k, q[k], rq[k])
        assert d_rms <= b_rms, (name, k, q[k], rq[k])


@pytest.mark.parametrize("name", tr.case_ids())
def test_table_case_matches_the_restatement(ctx, name):
    c = tr.case(name)
    got, q = ctx.register_translational(c["stack"], with_quality=True)
    compare(name, c["stack"], c["exact"], got, q)
    assert np.array_equal(ctx.register_translational(c["stack"]), got)  # the plain call: the same shifts, bit for bit


def test_minimum_size_keeps_the_integer_shift_without_a_pass(ctx):
    c = tr.case("8x8")
    got, q = ctx.register_translational(c["stack"], with_quality=True)
    assert np.array_equal(got[2:6], c["shifts"][2:6]) and list(q[2:6, 1]) == [-1.0] * 4 and list(q[2:6, 0]) == [1.0] * 4
    assert np.array_equal(got[1], [0.0, 0.0]) and q[1, 1] == 0.0


def test_flat_periodic_and_clamped_pairs_equal_the_restatement(ctx):
    no = np.zeros(2, dtype=bool)
    # flat: every candidate ties at 0, the first wins, (-R0, -R0); no texture; separation 0
    st = tr.special("flat")
    got, q = ctx.register_translational(st, with_quality=True)
    compare("flat", st, no, got, q)
    assert np.array_equal(got[1], [-16.0, -16.0]) and list(q[1]) == [0.0, 0.0]
    # periodic: candidates a period apart tie at exactly 0, the first wins: ambiguous, and reported as such
    st = tr.special("periodic")
    got, q = ctx.register_translational(st, with_quality=True)
    compare("periodic", st, no, got, q)
    assert np.array_equal(got[1], tr.restated("periodic")["rows"][0][1]) and q[1, 0] == 0.0 and q[1, 0] < 0.2 and q[1, 1] == 0.0
    # clamp: every pass is clamped on both axes, the pass limit ends the run: the answer is the integer answer -+ 1 exactly
    st = tr.special("clamp")
    got, q = ctx.register_translational(st, with_quality=True)
    compare("clamp", st, no, got, q)
    assert np.array_equal(got[1], tr.restated("clamp")["rows"][0][1])


def test_five_frames_repeat_permute_and_prefix_bit_for_bit(ctx):
    st = tr.special("five")
    got, q = ctx.register_translational(st, with_quality=True)
    compare("five", st, np.array([False, False, True, False, False]), got, q)
    again, q2 = ctx.register_translational(st, with_quality=True)
    assert np.array_equal(again, got) and np.array_equal(q2, q)
    perm = list(tr.FIVE_PERMUTATION)  # frame 0 stays
    gp, qp = ctx.register_translational(st[perm], with_quality=True)
    assert np.array_equal(gp, got[perm]) and np.array_equal(qp, q[perm])
    for n in range(1, 5):
        gn, qn = ctx.register_translational(st[:n], with_quality=True)
        assert np.array_equal(gn, got[:n]) and np.array_equal(qn, q[:n])
        assert np.array_equal(ctx.register_translational(st[:n]), got[:n])


# ------------------------------------------------------------------------------------------- error paths
SENTINEL = 7.0


def _raw(sr, ctx, n, W, H, images, want_shifts=True, want_quality=True, plain=False):
    """(status, shifts buffer, quality buffer) of the C call itself; the buffers start as SENTINEL."""
    lib = sr.load()
    dp = C.POINTER(C.c_double)
    cap = max(n, 1) + 1
    out, q = np.full((cap, 2), SENTINEL), np.full((cap, 2), SENTINEL)
    pi = None if images is None else np.ascontiguousarray(images, dtype=np.float64).ctypes.data_as(dp)
    po = out.ctypes.data_as(dp) if want_shifts else None
    if plain:
        return lib.srmap_register_translational(ctx._h, n, W, H, pi, po), out, q
    return lib.srmap_register_translational_ex(ctx._h, n, W, H, pi, po, q.ctypes.data_as(dp) if want_quality else None), out, q


def test_refusals_and_what_they_leave_untouched(sr, ctx):
    st = np.array(tr.case("12x16")["stack"][:3])
    untouched = np.full((4, 2), SENTINEL)
    for plain in (False, True):
        for st_n, images, shifts in ((-1, st, True), (3, st, False), (3, None, True)):
            rc, out, q = _raw(sr, ctx, st_n, 16, 12, images, want_shifts=shifts, plain=plain)
            assert rc == sr.EINVAL and np.array_equal(out, untouched[:len(out)]) and np.array_equal(q, untouched[:len(q)])
    for bad in (np.zeros((2, 7, 40)), np.zeros((2, 40, 7))):
        with pytest.raises(sr.SrmapError) as e:
            ctx.register_translational(bad)
        assert e.value.status == sr.EINVAL and "at least 8 x 8" in str(e.value)
        rc, out, q = _raw(sr, ctx, 2, bad.shape[2], bad.shape[1], bad)
        assert rc == sr.EINVAL and np.all(out == SENTINEL) and np.all(q == SENTINEL)
    # n = 0 writes nothing; n = 1 writes (0, 0) and (1, 0), and nothing behind them
    rc, out, q = _raw(sr, ctx, 0, 16, 12, st)
    assert rc == sr.OK and np.all(out == SENTINEL) and np.all(q == SENTINEL)
    rc, out, q = _raw(sr, ctx, 1, 16, 12, st)
    assert rc == sr.OK and list(out[0]) == [0.0, 0.0] and list(q[0]) == [1.0, 0.0] and np.all(out[1:] == SENTINEL) and np.all(q[1:] == SENTINEL)
    rc, out, _ = _raw(sr, ctx, 1, 16, 12, st, want_quality=False)
    assert rc == sr.OK and list(out[0]) == [0.0, 0.0]


def test_finite_pixels_whose_products_overflow_are_refused(sr, ctx):
    """The restatement's "overflow" pair: every pixel finite, the step NaN (tests/test_registration_cpu.py).  The call
    refuses before a NaN shift becomes the next pass's margin and sample offsets; the frames before it are answered."""
    st = tr.special("overflow")
    with pytest.raises(sr.SrmapError) as e:
        ctx.register_translational(st, with_quality=True)
    assert e.value.status == sr.EINVAL and "Could not determine motion shift between images." in str(e.value)
    rc, out, q = _raw(sr, ctx, 2, 47, 33, st)
    assert rc == sr.EINVAL and list(out[0]) == [0.0, 0.0] and np.all(out[1:] == SENTINEL)
    got = ctx.register_translational(tr.case("33x47")["stack"][:2])  # the context still works
    assert np.array_equal(got, tr.restated("33x47")["rows"][0][:2])


@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("frame", [0, 2])
def test_a_non_finite_frame_is_refused_by_both_estimators(sr, ctx, frame, value):
    """A non-finite pixel in frame 0 made every mean squared difference NaN, which fails every comparison: both calls
    answered SRMAP_OK with the corner of the search.  In a later frame the refinement's step became NaN and the next pass
    took its margin and its sample offsets from it.  Now: SRMAP_EINVAL before any GPU work, the frame's number in the
    message, as srmap_register_flow answers; nothing written."""
    st = np.array(tr.case("33x47")["stack"][:3])
    st[frame, 11, 13] = value
    for call, word in ((ctx.register_translational, "registration: image %d is not finite"),
                       (lambda s: ctx.register_translational(s, with_quality=True), "registration: image %d is not finite"),
                       (ctx.register_affine, "affine registration: image %d is not finite")):
        with pytest.raises(sr.SrmapError) as e:
            call(st)
        assert e.value.status == sr.EINVAL and (word % frame) in str(e.value), str(e.value)
    rc, out, q = _raw(sr, ctx, 3, 47, 33, st)
    assert rc == sr.EINVAL and np.all(out == SENTINEL) and np.all(q == SENTINEL)
    with pytest.raises(tr.RegistrationError):
        tr.register_translational(st)
    # and the same call on the finite stack still answers
    ok = np.array(tr.case("33x47")["stack"][:3])
    assert np.array_equal(ctx.register_translational(ok), ctx.register_translational(tr.case("33x47")["stack"])[:3])
