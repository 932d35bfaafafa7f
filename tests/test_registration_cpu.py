"""The restatement of the translational registration (tests/registration_restatement.py), CPU only: the conditions that
make its case table a fair yardstick for the GPU (tests/test_gpu_registration_parity.py), and its own contract.

Conditions.  The GPU and the restatement differ at the rounding level (summation order, fused multiply-adds).  A case is
in the table only if no DECISION of the run is that close to its threshold, in all three summation orders: the argmin of
every level, the stop of the refinement, the texture test, the clamp, the margin.  A case that breaks one is replaced.

Bars of the contract are pinned from what the restatement measures on this table (the figures are in the messages)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_registration_restatement as rg  # noqa: E402
import registration_restatement as tr  # noqa: E402
from test_affine_map_cpu import _call  # noqa: E402

ALL = tr.case_ids() + list(tr.SPECIAL)
CLEAN = [n for n in tr.case_ids() if not n.endswith("noise")]


# ------------------------------------------------------------------------------------------- the table's conditions
def near(v, target, rtol=1e-3):
    return target * (1 - rtol) <= v <= target * (1 + rtol)


@pytest.mark.parametrize("name", ALL)
def test_no_decision_of_a_case_is_within_rounding_of_its_threshold(name):
    runs = tr.restated(name)
    n = len(runs["rows"][0])
    figures = dict(argmin=np.inf, stop=np.inf, clamp=np.inf, margin=np.inf)
    for k in range(1, n):
        base = runs["rows"][2][k]
        for order in tr.ORDERS:
            T = runs[order][2][k]
            where = "%s frame %d order %s" % (name, k, order)
            assert T["integer"] == base["integer"] and len(T["passes"]) == len(base["passes"]), where
            for lv in T["levels"]:
                if lv["best"] == 0.0:
                    continue
                gap = (lv["second"] - lv["best"]) / lv["second"]
                figures["argmin"] = min(figures["argmin"], gap)
                assert gap >= 1e-6, (where, lv["size"], gap)
            sx, sy = T["integer"]
            for p in T["passes"]:
                assert not near(abs(p["det_ratio"]), tr.TEXTURE_RTOL), (where, p["det_ratio"])
                arg = p["margin_arg"]
                if arg != round(arg):
                    figures["margin"] = min(figures["margin"], abs(arg - round(arg)))
                    assert abs(arg - round(arg)) > 1e-9, (where, arg)
                if p["u"] is None:
                    continue
                step = max(abs(p["u"][0]), abs(p["u"][1]))
                if step > 0.0:
                    figures["stop"] = min(figures["stop"], max(step / tr.STOP, tr.STOP / step))
                assert not near(step, tr.STOP), (where, step)
                for v, s in zip(p["unclamped"], (sx, sy)):
                    d = min(abs(v - (s - 1.0)), abs(v - (s + 1.0)))
                    figures["clamp"] = min(figures["clamp"], d)
                    assert d > 1e-9, (where, p["unclamped"])
    print("%s: smallest argmin gap %.2e, step nearest to the stop a factor %.3f away, nearest to the clamp %.2e px, "
          "margin argument nearest to an integer %.2e" % (name, figures["argmin"], figures["stop"], figures["clamp"], figures["margin"]))


def test_the_clamp_case_clamps_in_every_pass_and_ends_at_the_pass_limit():
    sh, q, trace = tr.restated("clamp")["rows"]
    T = trace[1]
    sx, sy = T["integer"]
    R = tr.coarsest_radius(47, 33)
    assert (abs(sx), abs(sy)) == (R, R)
    assert len(T["passes"]) == tr.MAX_PASSES and all(p["clamped"] for p in T["passes"])
    assert abs(sh[1, 0] - sx) == 1.0 and abs(sh[1, 1] - sy) == 1.0
    assert all(abs(p["unclamped"][0] - sx) > 1.0 and abs(p["unclamped"][1] - sy) > 1.0 for p in T["passes"])  # both axes


# ------------------------------------------------------------------------------------------- the structure the table names
def test_level_rule_radius_and_chunks_are_what_the_table_says():
    assert tr.level_sizes(64, 64) == [(64, 64)] and tr.coarsest_radius(64, 64) == 16
    assert tr.level_sizes(65, 65) == [(65, 65), (32, 32)] and tr.coarsest_radius(65, 65) == 8
    assert tr.level_sizes(129, 70) == [(129, 70), (64, 35)] and tr.coarsest_radius(129, 70) == 8
    assert tr.level_sizes(257, 130) == [(257, 130), (128, 65), (64, 32)] and tr.coarsest_radius(257, 130) == 8
    assert tr.coarsest_radius(8, 8) == 4 and tr.coarsest_radius(255, 31) == 7 and tr.coarsest_radius(16, 1030) == 4
    assert [tr.largest_shift(W, H) for H, W, _ in tr.SIZES] == [4, 4, 4, 4, 8, 16, 16, 16, 32, 7, 8, 8, 4, 4]
    assert len(tr.level_sizes(1 << 20, 1 << 20)) == tr.MAX_LEVELS
    assert [len(tr.row_chunks(h)) for h in (8, 16, 31, 32, 33, 47, 48, 1023, 1024, 1030)] == [1, 1, 1, 2, 2, 2, 3, 63, 64, 64]
    ch = tr.row_chunks(1030)
    assert ch[0] == (0, 17) and ch[60] == (1020, 1030) and [r1 - r0 for r0, r1 in ch[61:]] == [1030 - 61 * 17, 1030 - 62 * 17, 1030 - 63 * 17]
    assert all(r1 <= r0 for r0, r1 in ch[61:])  # three empty trailing chunks
    for h in (8, 9, 17, 33, 65, 130, 1030):
        rows = [r for r0, r1 in tr.row_chunks(h) for r in range(r0, r1)]
        assert rows == list(range(h))  # every row once


@pytest.mark.parametrize("name", ["8x8", "9x11", "33x47", "65x65", "130x257", "33x257", "1030x16", "16x600"])
def test_overlap_counts_and_the_quarter_rule(name):
    """Every candidate of every level counts (w - |ux|)(h - |uy|) pixels, and is left out exactly below 0.25 w h."""
    _, _, trace = tr.restated(name)["rows"]
    left_out = at_the_quarter = 0
    for T in trace[1:]:
        for lv in T["levels"]:
            h, w = lv["size"]
            R, (cx, cy) = lv["R"], lv["centre"]
            u = np.arange(-R, R + 1)
            want = np.maximum(0, h - np.abs(cy + u))[:, None] * np.maximum(0, w - np.abs(cx + u))[None, :]
            assert np.array_equal(lv["counts"], want), (name, lv["size"], lv["centre"])
            assert np.array_equal(lv["msd"] < 0, want < 0.25 * w * h)
            left_out += int(np.count_nonzero(lv["msd"] < 0))
            at_the_quarter += int(np.count_nonzero(want == 0.25 * w * h))
    # R0 <= max(4, side / 4) on sides >= 8 keeps at least half of each side: the rule leaves no candidate of these tables
    # out, and 8 x 8 has the corners of its search exactly AT the quarter, which stay in (the largest-shift case is one)
    assert left_out == 0 and (at_the_quarter > 0) == (name == "8x8")


# ------------------------------------------------------------------------------------------- the contract
def pass_runs(H, W, d):
    """Whether a refinement pass fits at the integer shift d."""
    margin = int(max(abs(d[0]), abs(d[1]))) + 2
    return min(H, W) - 2 * margin >= 4


@pytest.mark.parametrize("name", CLEAN)
def test_integer_shifts_are_recovered_exactly(name):
    """True integer shifts: the shift exactly; RMS exactly 0, or -1 where no pass fits; separation exactly 1 where the
    shift is a whole number of pixels of the coarsest level too (there the best candidate's error is exactly 0), a clear
    minimum (> 0.5; smallest measured 0.672) where it is not."""
    c = tr.case(name)
    sh, q, trace = tr.restated(name)["rows"]
    coarse = 2 ** (len(tr.level_sizes(c["W"], c["H"])) - 1)
    for k in np.nonzero(c["exact"])[0][1:]:
        d = c["shifts"][k]
        assert np.array_equal(sh[k], d), (name, k, sh[k], d)
        assert q[k, 1] == (0.0 if pass_runs(c["H"], c["W"], d) else -1.0), (name, k, q[k])
        if d[0] % coarse == 0 and d[1] % coarse == 0:
            assert q[k, 0] == 1.0, (name, k, q[k])
        else:
            assert 0.5 < q[k, 0] < 1.0, (name, k, q[k])


def test_the_minimum_size_returns_the_integer_shift_without_a_pass():
    c = tr.case("8x8")
    sh, q, trace = tr.restated("8x8")["rows"]
    for k in range(1, len(sh)):
        moved = max(abs(sh[k, 0]), abs(sh[k, 1])) >= 1
        assert (len(trace[k]["passes"]) == 0) == moved
        if moved:
            assert q[k, 1] == -1.0 and np.array_equal(sh[k], trace[k]["integer"])
    assert np.array_equal(sh[2:6], c["shifts"][2:6]) and list(q[2:6, 1]) == [-1.0] * 4  # |d| >= 1: integer, RMS -1
    assert q[1, 1] == 0.0  # (0, 0): one pass fits (margin 2 leaves 4 x 4)
    # 12 x 16 is the first size of the table at which shifts of 1 and 2 get a pass
    assert list(tr.restated("9x11")["rows"][1][2:5, 1]) == [-1.0] * 3
    assert list(tr.restated("12x16")["rows"][1][2:5, 1]) == [0.0] * 3


# worst sub-pixel error per size: the bar (measured on this table: the figure in the comment)
SUBPIXEL_BARS = {"8x8": 1.5,        # 1.5: no pass fits once |d| >= 1, and the search sees 16...64 pixels
                 "9x11": 0.75,      # 0.75: the same
                 "12x16": 0.26,     # 0.250: 4 x 8 pixels inside the margin at |d| = 2
                 "17x23": 0.05,     # 0.0445
                 "33x47": 0.0092,   # 0.0067; 0.0083 on the five-frame stack's texture
                 "1030x16": 0.008}  # 0.0070: 12 columns inside the margin
SUBPIXEL_BAR_FROM_64 = 0.006        # 0.0054 (31 x 255); 2.2e-4 ... 3.3e-3 elsewhere


@pytest.mark.parametrize("name", CLEAN)
def test_subpixel_shifts_at_the_error_the_size_allows(name):
    c = tr.case(name)
    sh, q, _ = tr.restated(name)["rows"]
    sub = np.nonzero(~c["exact"])[0]
    err = np.max(np.abs(sh[sub] - c["shifts"][sub]), axis=1)
    bar = SUBPIXEL_BARS.get(name, SUBPIXEL_BAR_FROM_64)
    print("%s: sub-pixel errors %s px, bar %g" % (name, np.array2string(err, precision=4), bar))
    assert np.max(err) <= bar, (name, err, bar)


@pytest.mark.parametrize("name", [n for n in tr.case_ids() if n.endswith("noise")])
def test_noisy_frames_keep_the_integer_part_and_a_tenth_of_a_pixel(name):
    """sigma = 0.01: the contract of the existing GPU test (0.1 px), held by the restatement at the table's sizes."""
    c = tr.case(name)
    sh, q, trace = tr.restated(name)["rows"]
    err = np.max(np.abs(sh[1:] - c["shifts"][1:]), axis=1)
    print("%s: errors %s px" % (name, np.array2string(err, precision=4)))
    assert np.max(err) <= 0.1
    assert np.all(q[1:, 1] > 0.5 * tr.NOISE_SIGMA)  # the residual sees the noise of two frames


def test_flat_pair_answers_the_first_candidate():
    """Every candidate ties at 0: the first in row-major order wins, (-R0, -R0); separation 0; one pass runs, finds no
    texture and reports the residual 0."""
    sh, q, trace = tr.restated("flat")["rows"]
    assert np.array_equal(sh[1], [-16.0, -16.0]) and list(q[1]) == [0.0, 0.0]
    assert len(trace[1]["passes"]) == 1 and trace[1]["passes"][0]["u"] is None and trace[1]["passes"][0]["det_ratio"] == 0.0


def test_periodic_pair_is_reported_as_ambiguous():
    """Candidates a period apart tie at exactly 0: the first wins -- an alias of (3, 2) by whole periods --, separation 0."""
    sh, q, trace = tr.restated("periodic")["rows"]
    k = (sh[1] - [3, 2]) / 16.0
    assert np.array_equal(k, np.round(k)) and q[1, 0] == 0.0 and q[1, 1] == 0.0
    assert np.array_equal(sh[1], [-13.0, -14.0])  # the first of the ties in row-major order: smallest uy, then ux
    assert np.count_nonzero(trace[1]["levels"][0]["msd"] == 0.0) == 4  # (3 - 16, 3) x (2 - 16, 2)


def test_frames_are_independent_of_the_rest_of_the_stack():
    st = tr.special("five")
    sh, q = tr.restated("five")["rows"][:2]
    perm = list(tr.FIVE_PERMUTATION)
    sp, qp = tr.register_translational(st[perm])
    assert np.array_equal(sp, sh[perm]) and np.array_equal(qp, q[perm])
    s3, q3 = tr.register_translational(st[:3])
    assert np.array_equal(s3, sh[:3]) and np.array_equal(q3, q[:3])
    truth = np.array(tr.FIVE_SHIFTS, dtype=float)
    assert np.array_equal(sh[2], truth[2]) and np.max(np.abs(sh - truth)) <= SUBPIXEL_BARS["33x47"]


# ------------------------------------------------------------------------------------------- pieces
def test_search_separation_equals_the_host_algebra():
    """The restated separation against csrc/affine_map.hpp's on the restatement's own coarsest tables (entries left out,
    -1, are test_affine_map_cpu.py's: no table here has one)."""
    for name, frames in (("8x8", (1, 5, 6)), ("33x47", (2, 7)), ("65x65", (2, 8)), ("periodic", (1,)), ("flat", (1,))):
        sh, q, trace = tr.restated(name)["rows"]
        for k in frames:
            lv = trace[k]["levels"][0]
            n1, bi = 2 * lv["R"] + 1, lv["winner"]
            got = _call("search_separation", n1, bi, *lv["msd"].ravel())[0]
            assert got == tr.search_separation(lv["msd"], bi) == q[k, 0], (name, k)


def test_warp_is_the_motion_module_convention():
    """out(q) = img(q - d), zero outside: an integer shift copies, a half-pixel shift averages, the border is zero."""
    img = tr.texture(np.random.default_rng(1), 9, 11)
    out = tr.warp(img, (2, -1))
    assert np.array_equal(out[:-1, 2:], img[1:, :-2]) and np.all(out[:, :2] == 0) and np.all(out[-1] == 0)
    assert np.array_equal(tr.warp(img, (0, 0)), img)
    half = tr.warp(img, (0.5, 0))
    assert np.array_equal(half[:, 1:], 0.5 * img[:, 1:] + 0.5 * img[:, :-1]) and np.array_equal(half[:, 0], 0.5 * img[:, 0])
    q = tr.warp(img, (-1.75, 1.5))  # out(x, y) = img(x + 1.75, y - 1.5)
    assert abs(q[4, 3] - (0.5 * (0.25 * img[2, 4] + 0.75 * img[2, 5]) + 0.5 * (0.25 * img[3, 4] + 0.75 * img[3, 5]))) <= 1e-15


def test_the_three_orders_really_differ():
    a = tr.texture(np.random.default_rng(2), 33, 47)
    sums = {o: tr.total(a * a, o) for o in tr.ORDERS}
    assert len(set(sums.values())) >= 2 and max(sums.values()) - min(sums.values()) <= 1e-11
    assert tr.total(np.ones((5, 7)), "rows") == tr.total(np.ones((5, 7)), "cols") == tr.total(np.ones((5, 7)), "reversed") == 35.0
    assert tr.total(np.zeros((0, 3)), "rows") == 0.0


def test_a_step_that_is_not_finite_is_refused():
    """Finite pixels can still overflow a product: the sums of gx e hold +inf and -inf, the step is NaN in every summation
    order, and a NaN shift must not reach the next pass (its margin and sample offsets would come from it)."""
    st = tr.special("overflow")
    assert np.all(np.isfinite(st))
    with np.errstate(all="ignore"):
        for order in tr.ORDERS:
            (sx, sy), _, _ = tr.integer_shift([st[0]], [st[1]], order)
            S = tr.lk_sums(st[0], st[1], float(sx), float(sy), max(abs(sx), abs(sy)) + 2, order)
            assert np.all(np.isfinite(S[:3])) and S[0] * S[2] - S[1] * S[1] > 1e-12 * S[0] * S[2]  # texture: the test passes
            assert np.isnan(S[3]) and np.isnan(S[4])
            with pytest.raises(tr.RegistrationError) as e:
                tr.register_translational(st, order)
            assert str(e.value) == "Could not determine motion shift between images."


@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("frame", [0, 2])
def test_both_restatements_refuse_a_non_finite_frame(frame, value):
    st = np.array(tr.case("12x16")["stack"][:3])
    st[frame, 5, 7] = value
    for fn, word in ((tr.register_translational, "registration: image %d is not finite"),
                     (rg.register_affine, "affine registration: image %d is not finite")):
        with pytest.raises(tr.RegistrationError) as e:
            fn(st)
        assert str(e.value) == word % frame
