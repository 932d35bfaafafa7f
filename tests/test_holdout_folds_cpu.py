"""The hold-out given as a fold and the cross-validated lambda path without a GPU (include/srmap.h:
srmap_problem_set_holdout_fold, srmap_solve_lambda_path_folds): the band mask of
tests/holdout_folds_restatement.py against literals and against the plain C++ twin (csrc/holdout_host.hpp through
tests/cpp/holdout_folds_test.cpp), the partition, the mean, the standard error and the choice, the tool's refusals, and the
table of the README re-measured: on the four inputs of tests/test_holdout_cpu.py five folds with the one-standard-error rule
choose a lambda whose PSNR is never below the single split's.

The table.  Inputs, geometry, grid and solves of tests/test_holdout_cpu.py; 5 folds, mask seed 1 on every input (the
single split needed seed 2 at sigma 0.03).  A case is in the table only if its decisions have room (ROOM, relative): the
least mean is that far below its runner-up and is not at the small-lambda end of the grid, and no row above it is that near
the one-standard-error threshold.  All four cases are admitted at seed 1.

The quality bar of the one-standard-error row is the distance to the grid's best PSNR this restatement measured (0 dB on
three inputs, 0.24 dB at sigma 0.003) plus 0.25 dB of margin (EXPECT below)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as orc
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import holdout_folds_restatement as hfr  # noqa: E402
import holdout_restatement as hr  # noqa: E402
import robust_restatement as rr  # noqa: E402
import test_holdout_cpu as cpu  # noqa: E402

NEW_SYMBOLS = ("srmap_problem_set_holdout_fold", "srmap_problem_get_holdout_fold", "srmap_lambda_cv_options_default",
               "srmap_solve_lambda_path_folds")
FOLDS = 5
SEEDS = {"sigma 0.01": 1, "sigma 0.03": 1, "sigma 0.003": 1, "salt and pepper": 1}
ROOM = 1e-3
# name: (lambda of the least mean, lambda under the one-standard-error rule, the most that one's PSNR may be below the grid's best [dB])
EXPECT = {"sigma 0.01": (0.02, 0.04, 0.25),       # measured: one_se 41.66 dB, the grid's best; min 41.04
          "sigma 0.03": (0.16, 0.16, 0.25),       # 37.78, the grid's best, under both rules
          "sigma 0.003": (0.005, 0.005, 0.49),    # 44.99 against 45.23 (lambda 0.01)
          "salt and pepper": (0.02, 0.04, 0.25)}  # one_se 39.80, the grid's best; min 39.32


def test_library_exports_and_header_declares_the_entry_points():
    import ctypes as C
    import __graft_entry__ as ge
    ge.build_lib()
    import srmap
    lib = srmap.load()
    text = open(os.path.join(ROOT, "include", "srmap.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in srmap.EXPORTED_SYMBOLS and name in text, name
    assert "#define SRMAP_LAMBDA_RULE_MIN 0" in text and "#define SRMAP_LAMBDA_RULE_ONE_SE 1" in text
    assert (srmap.LAMBDA_RULE_MIN, srmap.LAMBDA_RULE_ONE_SE) == (0, 1) == (hfr.RULE_MIN, hfr.RULE_ONE_SE)
    po = srmap.LambdaCvOptions()
    lib.srmap_lambda_cv_options_default(C.byref(po))
    assert po.struct_size == C.sizeof(srmap.LambdaCvOptions) and po.num_scales == 8 and list(po.scales)[:8] == [2.0 ** -j for j in range(8)]
    assert (po.folds, po.seed, po.rule, po.se_factor, po.patience, po.final_solve) == (5, 1, srmap.LAMBDA_RULE_ONE_SE, 1.0, 0, 1)


# ------------------------------------------------------------------------------------------------ the band and the mask
def _twin(*args):
    import __graft_entry__ as ge
    exe = ge.build_holdout_folds_test()
    assert exe, "tests/cpp/holdout_folds_test.cpp is missing"
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout.split()


def test_the_literals_hold_in_plain_cpp():
    import __graft_entry__ as ge
    r = subprocess.run([ge.build_holdout_folds_test()], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def test_band_literals_and_the_partition():
    assert hfr.fold_band(5, 0) == (0, 3355443) and hfr.fold_band(5, 3) == (10066329, 13421772) and hfr.fold_band(5, 4) == (13421772, 1 << 24)
    assert hfr.fold_band(3, 1) == (5592405, 11184810) and hfr.fold_band(7, 6) == (14380470, 1 << 24) and hfr.fold_band(32, 31) == (16252928, 1 << 24)
    assert hfr.fold_band(4, 0) == (0, hr.threshold(0.25))
    for bad in ((1, 0), (0, 0), (33, 0), (5, 5), (5, -1), (2, 2)):
        assert hfr.fold_band(*bad) is None and _twin("band", *bad) == ["refused"], bad
    for F in (2, 3, 5, 7, 32):
        bands = [hfr.fold_band(F, f) for f in range(F)]
        assert bands[0][0] == 0 and bands[-1][1] == 1 << 24 and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
        assert [tuple(int(v) for v in _twin("band", F, f)) for f in range(F)] == bands
        total = sum(hfr.fold_mask((2, 3, 17, 23), F, f, 7) for f in range(F))
        assert np.array_equal(total, np.ones((2, 3, 17, 23)))  # every observation is in exactly one fold
    # [0, T) is the fraction's mask; the band test is the scalar definition
    for fraction, seed in ((0.1, 1), (0.5, 2), (0.25, 2 ** 63 + 5)):
        assert np.array_equal(hfr.band_mask((2, 3, 17, 23), 0, hr.threshold(fraction), seed), hr.mask((2, 3, 17, 23), fraction, seed))
    lo, hi = hfr.fold_band(5, 2)
    flat = hfr.fold_mask((2, 3, 17, 23), 5, 2, 7).ravel()
    assert all((lo <= (hr.hash_one(i, 7) >> 40) < hi) == bool(flat[i]) for i in range(flat.size))
    assert hfr.fold_mask((1, 1, 5, 7), 2, 1, 3).ravel().astype(int).tolist() == [1 - v for v in hr.mask((1, 1, 5, 7), 0.5, 3).ravel().astype(int)]


@pytest.mark.parametrize("shape", [(1, 1, 5, 7), (2, 3, 17, 23), (5, 1, 70, 129)])
def test_fold_masks_equal_the_cpp_twin(shape):
    n = int(np.prod(shape))
    for folds, fold, seed in ((2, 1, 1), (3, 1, 2), (5, 0, 1), (5, 4, 3), (7, 3, 2 ** 63 + 5), (32, 31, 2 ** 64 - 1)):
        bits = _twin("mask", n, folds, fold, seed)[0]
        ref = hfr.fold_mask(shape, folds, fold, seed)
        assert np.array_equal(np.frombuffer(bits.encode(), dtype=np.uint8) - ord("0"), ref.ravel().astype(np.uint8)), (shape, folds, fold)


# ------------------------------------------------------------------------------------------------ the rules
def test_stats_and_choice_on_hand_cases():
    assert hfr.fold_stats([1.0, 2.0, 3.0, 4.0, 5.0]) == (3.0, float(np.sqrt(0.5))) and hfr.fold_stats([2.0, 4.0]) == (3.0, 1.0)
    m, e = hfr.fold_stats([1.0, float("nan"), 3.0])
    assert m != m and e != e
    mean, se = [5.0, 3.4, 3.0, 3.2, 4.0], [0.1, 0.1, 0.5, 0.1, 0.1]
    assert hfr.choose_folds(mean, se, hfr.RULE_MIN) == (2, 2) and hfr.choose_folds(mean, se, hfr.RULE_ONE_SE) == (1, 2)
    assert hfr.choose_folds(mean, se, hfr.RULE_ONE_SE, 0.5) == (2, 2) and hfr.choose_folds(mean, se, hfr.RULE_ONE_SE, 4.0) == (0, 2)
    assert hfr.choose_folds(mean, se, hfr.RULE_ONE_SE, 0.0) == hfr.choose_folds(mean, se, hfr.RULE_MIN)  # se_factor 0 is MIN
    assert hfr.choose_folds([3.0, 1.0, 1.0, 2.0], [0.0, 0.0, 9.0, 0.0], hfr.RULE_ONE_SE) == (1, 1)  # a tie: the earlier row, and its se
    nan = float("nan")
    assert hfr.choose_folds([nan, 2.05, nan, 2.0, 2.5], [nan, 0.1, nan, 0.1, 0.1], hfr.RULE_ONE_SE) == (1, 3)  # a NaN row: never
    assert hfr.choose_folds([nan], [nan]) == (-1, -1) and hfr.choose_folds([], []) == (-1, -1)
    assert hfr.choose_folds([1.0, 2.0, 3.0], [5.0, 5.0, 5.0], hfr.RULE_ONE_SE) == (0, 0)  # jstar at row 0
    assert np.isclose(hfr.pixel_se([6.0, 14.0, 3.0, 3]), np.sqrt((14.0 / 3 - 4.0) / 3))


def test_stats_and_choice_equal_the_cpp_twin():
    rng = np.random.default_rng(5)
    fmt = lambda v: "nan" if v != v else repr(float(v))  # noqa: E731
    for trial in range(12):
        rows, F = int(rng.integers(1, 9)), int(rng.integers(2, 8))
        s = np.round(1.0 + 0.05 * rng.standard_normal((rows, F)), 3)  # rounded: ties and exact thresholds happen
        if trial % 4 == 3:
            s[rng.integers(0, rows), rng.integers(0, F)] = np.nan
        stats = [hfr.fold_stats(r) for r in s]
        for r, (m, e) in zip(s, stats):
            got = [float(v) for v in _twin("stats", *[fmt(v) for v in r])]
            assert (got[0] == m or (m != m and got[0] != got[0])) and (got[1] == e or (e != e and got[1] != got[1])), (r, got, m, e)
        flat = [fmt(v) for pair in stats for v in pair]
        for rule, word in ((hfr.RULE_MIN, "min"), (hfr.RULE_ONE_SE, "one_se")):
            for factor in (0.0, 0.5, 1.0, 3.0):
                got = tuple(int(v) for v in _twin("choose", word, factor, *flat))
                assert got == hfr.choose_folds([m for m, _ in stats], [e for _, e in stats], rule, factor), (s, rule, factor)


def test_the_words_of_the_command_line():
    assert _twin("rule", "min") == ["0"] and _twin("rule", "one_se") == ["1"]
    for bad in ("", "MIN", "one-se", "mini", "1"):
        assert _twin("rule", bad) == ["refused"], bad
    assert _twin("factor", "1") == ["1"] and _twin("factor", "0") == ["0"] and _twin("factor", "0.5") == ["0.5"]
    for bad in ("", "-1", "nan", "inf", "1x", "x"):
        assert _twin("factor", bad) == ["refused"], bad


def test_the_tool_refuses_bad_flags_before_any_gpu_work(tmp_path):
    """super_resolution answers the misuses of the cross-validation flags with a message and exit status 1 before it loads a
    frame or touches a GPU: the data path does not even exist."""
    import __graft_entry__ as ge
    tools = {os.path.basename(t): t for t in ge.build_apps()}
    srbin = tools["super_resolution"]
    path = "--lambda_path=0.08:0.5:4"
    for flags, word in ((["--holdout_folds=5", "--holdout_fraction=0.1", path], "--holdout_folds and --holdout_fraction exclude each other"),
                        (["--holdout_fraction=0.1", path, "--lambda_rule=one_se"], "--lambda_rule and --lambda_se_factor need --holdout_folds"),
                        (["--holdout_fraction=0.1", path, "--lambda_se_factor=1"], "--lambda_rule and --lambda_se_factor need --holdout_folds"),
                        (["--lambda_rule=min"], "--lambda_rule and --lambda_se_factor need --holdout_folds"),
                        (["--holdout_folds=1", path], "--holdout_folds is in 2...32."),
                        (["--holdout_folds=33", path], "--holdout_folds is in 2...32."),
                        (["--holdout_folds=-5", path], "--holdout_folds is in 2...32."),
                        (["--holdout_folds=5", path, "--lambda_rule=best"], "--lambda_rule is min or one_se."),
                        (["--holdout_folds=5", path, "--lambda_rule=ONE_SE"], "--lambda_rule is min or one_se."),
                        (["--holdout_folds=5", path, "--lambda_se_factor=-1"], "--lambda_se_factor is a finite number >= 0."),
                        (["--holdout_folds=5", path, "--lambda_se_factor=x"], "--lambda_se_factor is a finite number >= 0."),
                        (["--holdout_folds=5"], "--holdout_folds needs --lambda_path."),
                        (["--holdout_folds=5", "--lambda_path=0.08:0.5"], "--lambda_path is <largest>:<ratio>:<count>"),
                        (["--holdout_folds=5", path, "--lambda_patience=-1"], "--lambda_patience is >= 0."),
                        (["--holdout_folds=5", path, "--holdout_seed=abc"], "--holdout_seed is a non-negative integer"),
                        (["--holdout_folds=5", path, "--refine_motion_rounds=1"], "runs plain solves"),
                        # as before without the new flags
                        ([path], "--lambda_path needs --holdout_fraction."),
                        (["--holdout_seed=3"], "--holdout_seed needs --holdout_fraction.")):
        o = subprocess.run([srbin, "--data_path=" + str(tmp_path / "nothing")] + flags, capture_output=True, text=True, timeout=60)
        assert o.returncode == 1 and word in o.stderr, (flags, o.stdout, o.stderr)
    # a well-formed command line passes every refusal above and fails only at the data path
    o = subprocess.run([srbin, "--data_path=" + str(tmp_path / "nothing"), "--holdout_folds=5", "--holdout_seed=3", path, "--lambda_rule=min",
                        "--lambda_se_factor=0.5", "--print_lambda_path"], capture_output=True, text=True, timeout=60)
    assert "--holdout" not in o.stderr and "--lambda" not in o.stderr, o.stderr


# ------------------------------------------------------------------------------------------------ the table
def run_path(P, y, delta, name):
    """The 5-fold path of the table on one input (tests/golden/make_holdout_folds_table.py runs the same)."""
    kind, _, rng_, decay = P["reg"]
    return hfr.lambda_path_folds(P["model"], y, rr.bilinear(y[0], P["s"]), (kind, cpu.LAMBDA, rng_, decay), cpu.SCALES[name], FOLDS,
                                 SEEDS[name], huber_delta=delta, final_solve=False)


@pytest.fixture(scope="module")
def table():
    P, inputs = cpu._inputs()
    model, gt, s = P["model"], P["gt"], P["s"]
    kind, _, rng_, decay = P["reg"]
    print("inner solver: %s" % ("ALGLIB (oracle/_ref)" if orc.have_ref() else "the oracle's mincg"))
    with open(os.path.join(GOLDEN, "holdout_table.json")) as f:
        single = json.load(f)["inputs"]  # the single split's chosen rows, which tests/test_holdout_cpu.py re-measures
    out = {}
    for name, (y, delta) in inputs.items():
        x0 = rr.bilinear(y[0], s)
        res = run_path(P, y, delta, name)
        psnr = [cpu._psnr(hr.solve(model, y, x0, (kind, cpu.LAMBDA * sc, rng_, decay), None, delta)[0], gt) for sc in cpu.SCALES[name]]
        mean, se = [r["mean"] for r in res["rows"]], [r["se"] for r in res["rows"]]
        out[name] = dict(rows=res["rows"], mean=mean, se=se, psnr=psnr, single=single[name]["chosen"],
                         chosen_min=hfr.choose_folds(mean, se, hfr.RULE_MIN)[0], chosen_one_se=res["chosen"], jstar=res["jstar"])
        print("%s (%d folds, mask seed %d)" % (name, FOLDS, SEEDS[name]))
        for j, sc in enumerate(cpu.SCALES[name]):
            print("  lambda %-8g mean %.6e +- %.3e (%.2f %%; per-pixel se %.2f %%)  PSNR(all observations) %.2f dB%s%s%s"
                  % (cpu.LAMBDA * sc, mean[j], se[j], 100 * se[j] / mean[j], 100 * hfr.pixel_se(res["rows"][j]["pooled"]) / mean[j], psnr[j],
                     "  <- least mean" if j == res["jstar"] else "", "  <- one_se" if j == res["chosen"] else "",
                     "  <- single split" if j == single[name]["chosen"] else ""))
    return out


@pytest.mark.parametrize("name", list(cpu.SCALES))
def test_one_se_over_five_folds_is_never_worse_than_the_single_split(table, name):
    t = table[name]
    mean, se, psnr, js = np.array(t["mean"]), np.array(t["se"]), np.array(t["psnr"]), t["jstar"]
    lam = [cpu.LAMBDA * sc for sc in cpu.SCALES[name]]
    # the decisions have room
    room = (np.min(np.delete(mean, js)) - mean[js]) / mean[js]
    bar = mean[js] + se[js]
    near = min([abs(mean[j] - bar) / bar for j in range(js)], default=np.inf)
    best = int(np.argmax(psnr))
    print("%s: least mean at lambda %g (room %.2e), one_se lambda %g (PSNR %.2f), nearest row to the threshold %.2e; single split lambda %g "
          "(PSNR %.2f); best on the grid %.2f at %g" % (name, lam[js], room, lam[t["chosen_one_se"]], psnr[t["chosen_one_se"]], near,
                                                         lam[t["single"]], psnr[t["single"]], psnr[best], lam[best]))
    assert room >= ROOM and near >= ROOM and js < len(mean) - 1
    lam_min, lam_one, below = EXPECT[name]
    assert t["chosen_min"] == js and lam[js] == lam_min and lam[t["chosen_one_se"]] == lam_one
    assert psnr[t["chosen_one_se"]] >= psnr[t["single"]]
    assert psnr[best] - psnr[t["chosen_one_se"]] <= below


def test_the_per_pixel_standard_error_chooses_the_end_of_the_grid_under_outliers(table):
    """Why the rule needs folds: on the salt-and-pepper input the standard error that S2 and n give, all folds pooled, is
    several times the spread over the folds -- the corrupted held-out pixels dominate it --, and a one-standard-error rule
    built on it takes the largest lambda of the grid."""
    t = table["salt and pepper"]
    js = t["jstar"]
    pix = [hfr.pixel_se(r["pooled"]) for r in t["rows"]]
    print("salt and pepper: at the least mean the fold se is %.2f %% of the score, the per-pixel se %.2f %%"
          % (100 * t["se"][js] / t["mean"][js], 100 * pix[js] / t["mean"][js]))
    assert pix[js] > 2.0 * t["se"][js]
    assert hfr.choose_folds(t["mean"], pix, hfr.RULE_ONE_SE)[0] == 0
    assert 0 < t["chosen_one_se"] < js


def test_patience_reads_the_mean(table):
    mean = table["sigma 0.01"]["mean"]
    want = next(n for n in range(1, len(mean) + 1) if hr.patience_stop(mean[:n], 1))
    assert want < len(mean)
    se = table["sigma 0.01"]["se"]
    assert hfr.choose_folds(mean[:want], se[:want], hfr.RULE_ONE_SE)[1] == hr.choose(mean[:want])


def test_the_recorded_table_is_what_the_restatement_measures(table):
    """tests/golden/holdout_folds_table.json (tests/golden/make_holdout_folds_table.py), which the GPU test of the path reads:
    bit for bit with the solver that recorded it; with the other inner solver the chosen rows, and means to 1e-6 or ten times
    the recorded movement, whichever is larger."""
    with open(os.path.join(GOLDEN, "holdout_folds_table.json")) as f:
        g = json.load(f)
    same_solver = g["solver"].startswith("ALGLIB") == orc.have_ref()
    for name, t in table.items():
        r = g["inputs"][name]
        assert r["scales"] == cpu.SCALES[name] and r["mask_seed"] == SEEDS[name] and r["lambda"] == cpu.LAMBDA and r["folds"] == FOLDS
        assert r["chosen_min"] == t["chosen_min"] == r["chosen_min_moved"], name
        assert r["chosen_one_se"] == t["chosen_one_se"] == r["chosen_one_se_moved"], name
        rel = np.abs(np.array(r["mean"]) - np.array(t["mean"])) / np.array(t["mean"])
        print("%s: recorded means against this run's: %.2e (%s)" % (name, rel.max(), "same solver" if same_solver else "other solver"))
        if same_solver:
            assert r["mean"] == t["mean"] and r["se"] == t["se"], name
            assert r["scores"] == [[f["score"] for f in row["folds"]] for row in t["rows"]], name
            assert r["counts"] == [[[f["report"].irls_rounds, f["report"].cg_iterations, f["report"].nfev] for f in row["folds"]] for row in t["rows"]]
        else:
            assert np.all(rel <= np.maximum(1e-6, 10 * np.array(r["mean_move"]))), name
