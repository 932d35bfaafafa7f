"""The hold-out given as a fold and the cross-validated lambda path on the GPU (include/srmap.h:
srmap_problem_set_holdout_fold, srmap_solve_lambda_path_folds) against the numpy restatement
(tests/holdout_folds_restatement.py over tests/holdout_restatement.py).

Bars.  The mask and its counts: exact.  A problem with a fold held out against its twin whose caller set the prior
m .* (1 - h): bits.  Fold 0 of 4 against the fraction 0.25: bits.  The score of a fold against the restatement: the bars of
tests/test_gpu_holdout.py -- 100 x the restatement's own summation-order sensitivity with a floor of 1e-13 relative in f64,
2e-5 in f32; the counts n exact.  The path against the four calls every (row, fold) is made of: bits; its mean and standard
error against the stated order: bits.  The symbol, mask and path tests fail on the parent commit: none of these entry points
exists there."""
import json
import os
import sys

import numpy as np
import pytest

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import holdout_folds_restatement as hfr  # noqa: E402
import holdout_restatement as hr  # noqa: E402
import robust_restatement as rr  # noqa: E402
import test_gpu_data_prior as gdp  # noqa: E402
import test_gpu_holdout as gh  # noqa: E402
from test_gpu_data_prior import in_dtype, make_problem, report_tuple, short_options  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


# ------------------------------------------------------------------------------------------------ mask and counts
@pytest.mark.parametrize("KC", [(1, 1), (2, 3), (5, 1)])
@pytest.mark.parametrize("size", [(5, 7), (17, 23), (70, 129)])  # 5 x 7: only tails, no 16-byte group
def test_fold_masks_and_counts_equal_the_restatement_and_partition(sr, ctx, size, KC):
    h, w = size
    K, Cn = KC
    y = np.random.default_rng(h + K).random((K, Cn, h, w))
    for dtype in (0, 1):
        p = make_problem(sr, ctx, "subpixel" if K <= 4 else "direct", h, w, Cn, dtype, y)
        assert p.holdout_fold() == (0, 0, 0)
        for F, seed in ((2, 1), (3, 2), (5, 1), (7, 2 ** 63 + 5), (32, 2 ** 64 - 1)):
            total = np.zeros(y.shape)
            for f in range(F):
                tag = "%s K%d C%d f%d fold %d of %d" % (size, K, Cn, 32 if dtype else 64, f, F)
                p.set_holdout_fold(F, f, seed)
                fr_, seed_, mask, counts = p.holdout()
                ref = hfr.fold_mask(y.shape, F, f, seed)
                lo, hi = hfr.fold_band(F, f)
                assert p.holdout_fold() == (F, f, seed) and seed_ == seed and fr_ == (hi - lo) / 2.0 ** 24, tag
                assert np.array_equal(mask, ref), tag
                assert counts[0] == ref.sum() and np.array_equal(counts[1:], ref.reshape(K, -1).sum(1)), tag
                assert np.array_equal(p.holdout(want_mask=False)[3], counts), tag  # the host's count of the band
                assert p.data_prior() is None and np.array_equal(p.data_weights(), 1.0 - ref), tag
                total += mask
            assert np.array_equal(total, np.ones(y.shape)), (size, KC, F)  # every observation in exactly one fold
        # a fraction replaces the fold and a fold the fraction; 0 in either call lifts either
        p.set_holdout(0.1, 3)
        assert p.holdout_fold() == (0, 0, 3) and np.array_equal(p.holdout()[2], hr.mask(y.shape, 0.1, 3))
        p.set_holdout_fold(3, 2, 4)
        assert p.holdout_fold() == (3, 2, 4) and np.array_equal(p.holdout()[2], hfr.fold_mask(y.shape, 3, 2, 4))
        p.set_holdout(0)
        assert p.holdout_fold() == (0, 0, 0) and p.holdout()[0] == 0.0 and not p.holdout()[2].any()
        p.set_holdout(0.1, 3)
        p.set_holdout_fold(0, 0)
        assert p.holdout()[0] == 0.0 and not p.holdout()[2].any()


@pytest.mark.parametrize("dtype", [0, 1])
def test_fold_0_of_4_is_the_fraction_a_quarter_bit_for_bit(sr, ctx, dtype):
    h, w, Cn, K, s = 17, 23, 2, 4, 2
    rng = np.random.default_rng(12)
    y = rng.random((K, Cn, h, w))
    x, x0 = rng.random((Cn, h * s, w * s)), rng.random((Cn, h * s, w * s))
    a, b = make_problem(sr, ctx, "subpixel", h, w, Cn, dtype, y), make_problem(sr, ctx, "subpixel", h, w, Cn, dtype, y)
    a.set_holdout_fold(4, 0, 5)
    b.set_holdout(0.25, 5)
    assert a.holdout()[0] == 0.25 and np.array_equal(a.holdout()[2], b.holdout()[2]) and np.array_equal(a.holdout()[3], b.holdout()[3])
    gh.assert_same_state("fold 0 of 4", sr, ctx, a, b, x, x0, dtype, ("cg",))
    for delta in (0.0, 0.3):
        sa, sb = a.holdout_score(x, delta), b.holdout_score(x, delta)
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]), delta


# ------------------------------------------------------------------------------------------------ the prior twin
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("path", ["tile", "subpixel", "affine", "flow"])
def test_a_fold_is_the_prior_its_caller_could_have_set(sr, ctx, path, dtype):
    h, w, Cn, K, s = 17, 23, 3, 4, 2
    rng = np.random.default_rng(43 + dtype)
    y = rng.random((K, Cn, h, w))
    x, x0 = rng.random((Cn, h * s, w * s)), rng.random((Cn, h * s, w * s))
    m = rng.random(y.shape)
    m[2] = 0.0
    keep = 1.0 - hfr.fold_mask(y.shape, 5, 3, 9)
    for name, mm in (("bare", None), ("prior", m)):
        tag = "%s f%d %s" % (path, 32 if dtype else 64, name)
        a, b = make_problem(sr, ctx, path, h, w, Cn, dtype, y), make_problem(sr, ctx, path, h, w, Cn, dtype, y)
        a.set_data_prior(mm)
        a.set_holdout_fold(5, 3, 9)
        b.set_data_prior(keep if mm is None else mm * keep)
        gh.assert_same_state(tag, sr, ctx, a, b, x, x0, dtype, ("cg", "lbfgs"))
        xd = gh.device(x, dtype)
        for mode in (sr.HUBER_DELTA_FIXED, sr.HUBER_DELTA_MAD):  # a Huber step, FIXED and MAD, and a Huber solve
            for p in (a, b):
                p.set_data_loss(sr.DATA_LOSS_HUBER, 0.2)
                p.set_huber_scale(mode, 1.345, 1e-4)
                p.update_data_weights_device(xd.data_ptr())
            ctx.synchronize()
            assert np.array_equal(a.data_weights(), b.data_weights()), (tag, mode)
            assert a.huber_delta()[1] == b.huber_delta()[1] and np.array_equal(a.huber_delta()[3], b.huber_delta()[3]), (tag, mode)
            gh.assert_same_state(tag + " huber", sr, ctx, a, b, x, x0, dtype, ("cg",))


@pytest.mark.parametrize("dtype", [0, 1])
def test_a_setter_sequence_against_a_fresh_twin(sr, ctx, dtype):
    """set a fold, set a prior, set weights, switch to Huber, set a fraction, lift the hold-out: after every step the
    problem is, bit for bit, a fresh one whose caller set the same state with the prior m .* (1 - h) itself, and at the end
    the allocations are those of the start."""
    h, w, Cn, K, s = 17, 23, 2, 4, 2
    rng = np.random.default_rng(15)
    y = rng.random((K, Cn, h, w))
    x, x0 = rng.random((Cn, h * s, w * s)), rng.random((Cn, h * s, w * s))
    m, wts = rng.random(y.shape), 2.0 * rng.random(y.shape)
    keep_fold, keep_fr = 1.0 - hfr.fold_mask(y.shape, 5, 2, 6), 1.0 - hr.mask(y.shape, 0.1, 7)
    lib = sr.load()
    xd = gh.device(x, dtype)
    # step: (what the sequence does to p, the twin's prior, weights and loss)
    steps = (("fold", lambda p: p.set_holdout_fold(5, 2, 6), keep_fold, None, False),
             ("prior", lambda p: p.set_data_prior(m), m * keep_fold, None, False),
             ("weights", lambda p: p.set_data_weights(wts), m * keep_fold, wts, False),
             ("huber", lambda p: p.set_data_loss(sr.DATA_LOSS_HUBER, 0.1), m * keep_fold, wts, True),
             ("fraction", lambda p: p.set_holdout(0.1, 7), m * keep_fr, wts, True),
             ("lift", lambda p: p.set_holdout_fold(0, 0), m, wts, True))
    # a solve moves the regulariser's IRLS weights, which are the problem's: every prefix of the sequence is walked by a
    # problem of its own, so that the solve at its end meets a twin that has not solved either
    for n in range(1, len(steps) + 1):
        a = make_problem(sr, ctx, "subpixel", h, w, Cn, dtype, y)
        for _, step, _, _, _ in steps[:n]:
            step(a)
            a.eval(x)
        name, _, prior, weights, huber = steps[n - 1]
        b = make_problem(sr, ctx, "subpixel", h, w, Cn, dtype, y)
        b.set_data_weights(weights)
        b.set_data_prior(prior)
        if huber:
            b.set_data_loss(sr.DATA_LOSS_HUBER, 0.1)
            for p in (a, b):  # the weights of a Huber problem are the last step's: take one on both
                p.update_data_weights_device(xd.data_ptr())
            ctx.synchronize()
        gh.assert_same_state("%s f%d" % (name, 32 if dtype else 64), sr, ctx, a, b, x, x0, dtype, ("cg",))
        del a, b
    # the allocations: the whole sequence with an evaluation after every step and a score while something is held out,
    # then the loss, the weights and the prior of the start
    c = make_problem(sr, ctx, "subpixel", h, w, Cn, dtype, y)
    c.residual_scale(x)  # its buffers are the problem's from here on
    before = c.eval(x)
    import gc
    gc.collect()  # the count is the whole process's: an earlier test's problem in a reference cycle must not be freed below
    live = lib.srmap_live_allocations()
    for name, step, _, _, _ in steps:
        step(c)
        c.eval(x)
        if name != "lift":
            c.holdout_score(x, 0.0)
    assert c.holdout()[0] == 0.0 and c.holdout_fold() == (0, 0, 0)
    c.set_data_loss(sr.DATA_LOSS_L2)
    c.set_data_weights(None)
    c.set_data_prior(None)
    assert lib.srmap_live_allocations() == live
    after = c.eval(x)
    assert before[0] == after[0] and np.array_equal(before[1], after[1])


# ------------------------------------------------------------------------------------------------ the score
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", [((5, 7), 1, 1), ((17, 23), 2, 3), ((70, 129), 5, 1)] + [(sz, 2, 1) for sz in gh.GROUP_EDGE],
                         ids=lambda c: "%dx%d-K%d-C%d" % (c[0][0], c[0][1], c[1], c[2]))
def test_score_of_a_fold_against_the_restatement(sr, ctx, case, dtype):
    (h, w), K, Cn = case
    s = 2
    rng = np.random.default_rng(h * 7 + K + dtype)
    shifts = gdp.SUB_SHIFTS[:K] if K <= 4 else [[0.25 * k, -0.5 * k] for k in range(K)]
    model = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=3, blur_sigma=1.0)
    gt = rng.random((Cn, h * s, w * s))
    y = np.stack([model.apply(gt, k) for k in range(K)]) + 0.05 * rng.standard_normal((K, Cn, h, w))
    y[rng.random(y.shape) < 0.05] = 1.0  # outliers: the two branches of rho both run
    x = gt + 0.02 * rng.standard_normal(gt.shape)
    m, wts = rng.random(y.shape), 2.0 * rng.random(y.shape)
    m[rng.random(y.shape) < 0.2] = 0.0
    p = sr.Problem(ctx, w * s, h * s, Cn, K, s, shifts, 3, 1.0, dtype)
    p.set_observations(y)
    p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
    r = gh.gpu_residuals(p, x, in_dtype(y, dtype), dtype)
    np_dtype = np.float32 if dtype else np.float64
    for F, f in ((2, 1), (5, 0), (5, 4)) if h * w < 100 else ((5, 0), (5, 2), (5, 4), (32, 31)):
        p.set_holdout_fold(F, f, 6)
        hmask = hfr.fold_mask(y.shape, F, f, 6)
        tag0 = "%dx%d K%d C%d f%d fold %d of %d" % (h, w, K, Cn, 32 if dtype else 64, f, F)
        for name, mm, ww in (("none", None, None), ("both", m, wts)):
            p.set_data_weights(ww)
            p.set_data_prior(mm)
            u = hr.base_weight(y.shape, mm, ww, huber=False, dtype=np_dtype)
            if not (hmask * u).any():
                continue  # nothing held out with weight: the call is refused (the statuses' test)
            for delta in (0.0, 0.04):
                ref = hr.score(r, hmask, u, delta)
                got = p.holdout_score(x, delta)
                gh.check_score("%s L2 %s delta %g" % (tag0, name, delta), got, ref[0], ref[1], hr.score_sensitivity(r, hmask, u, delta), dtype)
                again = p.holdout_score(x, delta)
                assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), (tag0, name, delta)
        p.set_data_weights(None)
        p.set_data_prior(None)


# ------------------------------------------------------------------------------------------------ the path
def hand_path(q, x0, o, scales, F, seed, loss, lam=0.08):
    """Every (row, fold) by hand: the four calls.  Returns fold_table [rows][F][11] as the path must give it."""
    out = np.zeros((len(scales), F, 11))
    delta = None
    for j, sc in enumerate(scales):
        q.set_regularizer_lambda(0, lam * sc)
        for f in range(F):
            q.set_holdout_fold(F, f, seed)
            xj, rj = q.solve(x0, o)
            if loss == "mad" and j == 0 and f == 0:
                delta = q.huber_delta()[1]
            d = {"l2": 0.0, "fixed": 0.05, "mad": delta}[loss]
            score, sums = q.holdout_score(xj, d)
            out[j, f] = [sc, score[0], sums[0, 0], sums[0, 1], sums[0, 2], sums[0, 3], rj.irls_rounds, rj.cg_iterations, rj.evaluations,
                         rj.final_cost, d]
    return out


def check_table(table, fold_table):
    """The table's rows from fold_table in the stated order: mean, se, the pooled sums, the summed counts, delta."""
    for j in range(len(table)):
        mean, se = hfr.fold_stats(list(fold_table[j, :, 1]))
        pooled = np.zeros(4)
        counts = np.zeros(3)
        for f in range(fold_table.shape[1]):
            pooled += fold_table[j, f, 2:6]
            counts += fold_table[j, f, 6:9]
        row = [fold_table[j, 0, 0], mean, se] + list(pooled) + list(counts) + [fold_table[j, 0, 10]]
        assert np.array_equal(table[j], np.array(row)), (j, table[j], row)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("loss", ["l2", "fixed", "mad"])
def test_every_row_and_fold_is_its_four_calls_and_the_final_solve_is_a_solve(sr, ctx, loss, dtype):
    p, y, x0, gt = gh.path_problem(sr, ctx, dtype, loss)
    q, _, _, _ = gh.path_problem(sr, ctx, dtype, loss)
    scales, F, seed = [1.0, 0.25, 0.0625], 3, 2
    o = gh.path_options(sr)
    x, table, fold_table, chosen, rep = p.solve_lambda_path_folds(x0, scales, folds=F, seed=seed, options=o)
    assert table.shape == (len(scales), sr.LAMBDA_PATH_ROW) and fold_table.shape == (len(scales), F, sr.LAMBDA_PATH_ROW)
    want = hand_path(q, x0, o, scales, F, seed, loss)
    assert np.array_equal(fold_table, want), (loss, dtype, fold_table[:, :, 1], want[:, :, 1])
    check_table(table, fold_table)
    if loss == "mad":
        assert table[0, 10] > 0 and np.all(fold_table[:, :, 10] == table[0, 10])
    assert chosen == hfr.choose_folds(list(table[:, 1]), list(table[:, 2]), hfr.RULE_ONE_SE, 1.0)[0]
    # on return: the chosen lambdas, and no hold-out, as at the call
    assert p.regularizer_lambda(0) == 0.08 * scales[chosen]
    assert p.holdout()[0] == 0.0 and p.holdout_fold() == (0, 0, 0) and not p.holdout()[2].any()
    # the final solve: no hold-out, the chosen lambda
    q.set_holdout_fold(0, 0)
    q.set_regularizer_lambda(0, 0.08 * scales[chosen])
    xf, rf = q.solve(x0, o)
    assert np.array_equal(x, xf) and report_tuple(rep) == report_tuple(rf)


def test_rules_patience_no_final_solve_and_the_holdout_on_return(sr, ctx):
    p, y, x0, gt = gh.path_problem(sr, ctx, 0)
    o = gh.path_options(sr)
    scales, F = [4.0 * 0.5 ** j for j in range(6)], 3
    p.set_holdout(0.1, 2)  # a fraction at the call: a fraction on return
    x, full, folds_full, chosen, rep = p.solve_lambda_path_folds(x0, scales, folds=F, seed=4, rule="min", options=o, final_solve=False)
    assert x is None and rep is None and len(full) == 6
    assert p.holdout()[:2] == (0.1, 2) and p.holdout_fold()[0] == 0 and np.array_equal(p.holdout()[2], hr.mask(y.shape, 0.1, 2))
    check_table(full, folds_full)
    mean, se = list(full[:, 1]), list(full[:, 2])
    print("means %s\nses   %s" % (" ".join("%.5e" % v for v in mean), " ".join("%.5e" % v for v in se)))
    jstar = hr.choose(mean)
    assert chosen == jstar == int(np.argmin(mean)) and p.regularizer_lambda(0) == 0.08 * scales[chosen]
    # both rules over several factors: the same table, the restatement's row; a fold at the call: that fold on return
    p.set_holdout_fold(3, 1, 7)
    for rule, word in ((hfr.RULE_MIN, "min"), (hfr.RULE_ONE_SE, "one_se")):
        for factor in (0.0, 1.0, 3.0, 1e6):
            p.set_regularizer_lambda(0, 0.08)
            _, table, fold_table, ch, _ = p.solve_lambda_path_folds(x0, scales, folds=F, seed=4, rule=word, se_factor=factor, options=o,
                                                                    final_solve=False)
            assert np.array_equal(table, full) and np.array_equal(fold_table, folds_full)
            assert ch == hfr.choose_folds(mean, se, rule, factor)[0], (word, factor)
            assert p.regularizer_lambda(0) == 0.08 * scales[ch] and p.holdout_fold() == (3, 1, 7)
    assert np.array_equal(p.holdout()[2], hfr.fold_mask(y.shape, 3, 1, 7))
    assert hfr.choose_folds(mean, se, hfr.RULE_ONE_SE, 1e6)[0] == 0 and hfr.choose_folds(mean, se, hfr.RULE_ONE_SE, 0.0)[0] == jstar
    # patience reads the mean
    for patience in (1, 2):
        p.set_regularizer_lambda(0, 0.08)
        want = next((n for n in range(1, 7) if hr.patience_stop(mean[:n], patience)), 6)
        _, table, fold_table, ch, _ = p.solve_lambda_path_folds(x0, scales, folds=F, seed=4, options=o, patience=patience, final_solve=False)
        assert len(table) == want == len(fold_table) and np.array_equal(table, full[:want]), patience
        assert ch == hfr.choose_folds(mean[:want], se[:want], hfr.RULE_ONE_SE, 1.0)[0], patience


def test_the_lambdas_and_the_holdout_after_an_error(sr, ctx):
    p, y, x0, gt = gh.path_problem(sr, ctx, 0)
    o = gh.path_options(sr)
    p.set_holdout(0.1, 2)

    def refused(call, *words):
        with pytest.raises(sr.SrmapError) as e:
            call()
        assert e.value.status == sr.EINVAL, str(e.value)
        for word in words:
            assert word in str(e.value), (word, str(e.value))
        assert p.regularizer_lambda(0) == 0.08 and p.holdout()[:2] == (0.1, 2) and p.holdout_fold()[0] == 0

    for bad in ([1.0, 1.0], [0.5, 1.0], [1.0, 0.0], [np.nan], [], [1.0 / (j + 1) for j in range(33)]):
        refused(lambda: p.solve_lambda_path_folds(x0, bad, options=o), "lambda path (folds)", "scale")
    for folds in (1, 0, 33, -2):
        refused(lambda: p.solve_lambda_path_folds(x0, [1.0, 0.5], folds=folds, options=o), "folds must be in 2...32")
    refused(lambda: p.solve_lambda_path_folds(x0, [1.0, 0.5], rule=2, options=o), "SRMAP_LAMBDA_RULE_MIN or SRMAP_LAMBDA_RULE_ONE_SE")
    for factor in (-0.5, np.nan, np.inf):
        refused(lambda: p.solve_lambda_path_folds(x0, [1.0, 0.5], se_factor=factor, options=o), "se_factor must be finite and >= 0")
    refused(lambda: p.solve_lambda_path_folds(x0, [1.0, 0.5], patience=-1, options=o), "patience")
    refused(lambda: p.solve_lambda_path_folds(x0, [1.0, 0.5], struct_size=4, options=o), "srmap_lambda_cv_options.struct_size")
    # a fold without held-out weight fails the path from inside: row 0, fold 1 of 3 -- lambdas and hold-out of the call's start
    p.set_data_prior(1.0 - hfr.fold_mask(y.shape, 3, 1, 4))
    refused(lambda: p.solve_lambda_path_folds(x0, [0.5, 0.25], folds=3, seed=4, options=o), "nothing is held out")
    assert np.array_equal(p.holdout()[2], hr.mask(y.shape, 0.1, 2))
    p.set_data_prior(None)
    p.set_regularizer_lambda(0, 0.0)
    refused_status = pytest.raises(sr.SrmapError)
    with refused_status as e:
        p.solve_lambda_path_folds(x0, [1.0, 0.5], options=o)
    assert e.value.status == sr.EINVAL and "srmap_add_regularizer" in str(e.value)


# ------------------------------------------------------------------------------------------------ the pinned table inputs
@pytest.mark.parametrize("name", ["sigma 0.01", "sigma 0.03", "sigma 0.003", "salt and pepper"])
def test_the_path_on_the_table_inputs_is_the_restatements(sr, ctx, name):
    """The GPU path against the independent restatement (tests/holdout_folds_restatement.py's lambda_path_folds, recorded by
    tests/golden/make_holdout_folds_table.py and re-measured on the CPU by tests/test_holdout_folds_cpu.py) on the README
    table's inputs, f64: the restatement's chosen rows under both rules; its held-out counts; its solve counts on the (row,
    fold) pairs whose counts are stable when the observations move by 1e-13; its means and standard errors to ten times what
    that move moved them."""
    import test_holdout_cpu as cpu
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "holdout_folds_table.json")) as f:
        g = json.load(f)["inputs"][name]
    P, inputs = cpu._inputs()
    y, delta = inputs[name]
    assert g["scales"] == cpu.SCALES[name] and g["huber_delta"] == delta and g["lambda"] == cpu.LAMBDA
    kind, _, rng_, decay = P["reg"]
    p = sr.Problem(ctx, P["W"], P["H"], P["C"], P["K"], P["s"], P["shifts"], P["blur"][0], P["blur"][1], sr.F64)
    p.set_observations(y)
    p.add_regularizer(sr.REG_BTV, g["lambda"], rng_, decay)
    if delta is not None:
        p.set_data_loss(sr.DATA_LOSS_HUBER, delta)
    _, table, fold_table, chosen, _ = p.solve_lambda_path_folds(rr.bilinear(y[0], P["s"]), g["scales"], folds=g["folds"], seed=g["mask_seed"],
                                                                rule="one_se", final_solve=False)
    assert len(table) == len(g["scales"])
    check_table(table, fold_table)
    mean, se = np.array(g["mean"]), np.array(g["se"])
    err_m, err_s = np.abs(table[:, 1] - mean) / mean, np.abs(table[:, 2] - se) / se
    stable = np.array(g["stable"])
    for j in range(len(table)):
        print("%s lambda %-8g mean %.9e +- %.6e (restatement %.9e +- %.6e): off by %.2e and %.2e, bars %.2e and %.2e; evaluations %s, "
              "restatement %s, stable %s" % (name, g["lambda"] * g["scales"][j], table[j, 1], table[j, 2], mean[j], se[j], err_m[j], err_s[j],
                                             10 * g["mean_move"][j], 10 * g["se_move"][j], [int(v) for v in fold_table[j, :, 8]],
                                             [c[2] for c in g["counts"][j]], [int(v) for v in stable[j]]))
    by_min = hfr.choose_folds(list(table[:, 1]), list(table[:, 2]), hfr.RULE_MIN)[0]
    print("%s: chosen rows min %d one_se %d, restatement %d %d" % (name, by_min, chosen, g["chosen_min"], g["chosen_one_se"]))
    assert g["chosen_min"] == g["chosen_min_moved"] and g["chosen_one_se"] == g["chosen_one_se_moved"]  # the decisions have room
    assert by_min == g["chosen_min"] and chosen == g["chosen_one_se"]
    assert np.array_equal(fold_table[:, :, 5], np.array(g["held"]))  # the held-out pixels that count, per fold
    got_counts = fold_table[:, :, 6:9].astype(int)
    assert np.array_equal(got_counts[stable], np.array(g["counts"])[stable]), name
    assert np.all(err_m <= 10 * np.array(g["mean_move"])) and np.all(err_s <= 10 * np.array(g["se_move"])), (name, err_m, err_s)


# ------------------------------------------------------------------------------------------------ statuses
def test_statuses_and_messages(sr, ctx):
    h, w, Cn, K, s = 5, 7, 1, 2, 2
    rng = np.random.default_rng(1)
    y = rng.random((K, Cn, h, w))
    x = rng.random((Cn, h * s, w * s))
    lib = sr.load()
    p = sr.Problem(ctx, w * s, h * s, Cn, K, s, gdp.SUB_SHIFTS[:K], 3, 1.0, 0)

    def refused(call, status, *words):
        with pytest.raises(sr.SrmapError) as e:
            call()
        assert e.value.status == status, str(e.value)
        for word in words:
            assert word in str(e.value), (word, str(e.value))

    for folds, fold in ((1, 0), (33, 0), (-1, 0), (5, 5), (5, -1), (2, 2), (32, 32)):
        refused(lambda: p.set_holdout_fold(folds, fold), sr.EINVAL, "srmap_problem_set_holdout_fold", "2...32")
        assert p.holdout_fold() == (0, 0, 0) and p.holdout()[0] == 0.0
    p.set_holdout_fold(5, 1, 3)
    refused(lambda: p.set_holdout_fold(5, 5, 3), sr.EINVAL, "srmap_problem_set_holdout_fold")
    assert p.holdout_fold() == (5, 1, 3)  # a refused call changes nothing
    p.set_holdout_fold(0, 0)
    # the path names what is missing
    refused(lambda: p.solve_lambda_path_folds(x, [1.0, 0.5]), sr.EINVAL, "srmap_add_regularizer")
    p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.6)
    refused(lambda: p.solve_lambda_path_folds(x, [1.0, 0.5]), sr.EINVAL, "srmap_set_observations")
    p.set_observations(y)
    refused(lambda: p.holdout_score(x, 0.0), sr.EINVAL, "srmap_problem_set_holdout")
    # null handles and missing outputs
    assert lib.srmap_problem_set_holdout_fold(None, 5, 0, 1) == sr.EINVAL
    assert lib.srmap_problem_get_holdout_fold(None, None, None, None) == sr.EINVAL
    assert lib.srmap_solve_lambda_path_folds(None, None, None, None, None, None, None, None, None, None) == sr.EINVAL
    assert lib.srmap_problem_get_holdout_fold(p._h, None, None, None) == sr.OK
    # a sharded solve or evaluation over more than one rank: the hold-out's own refusal

    class NoExchange:
        calls = []

        class ReduceOp:
            SUM, MAX = 0, 1

        def all_reduce(self, *a, **k):
            self.calls.append("all_reduce")

        def isend(self, *a, **k):
            self.calls.append("isend")

        def irecv(self, *a, **k):
            self.calls.append("irecv")

    p.set_holdout_fold(2, 1, 1)
    fake = NoExchange()
    comm = sr.Comm(ctx, 0, 2, backend="host", dist=fake)
    xd, gd = gh.device(x, 0), gh.device(x, 0)
    for mode in (sr.SHARD_FRAMES, sr.SHARD_ROWS, sr.SHARD_CHANNELS):
        sd = sr.ShardDesc()
        sd.mode = mode
        sd.own_row0, sd.own_row1, sd.own_ch0, sd.own_ch1 = 0, h * s, 0, 1
        refused(lambda: p.solve(x, comm=comm, shard=sd), sr.EUNSUPPORTED, "a hold-out is not sharded", "run the solve unsharded")
        refused(lambda: p.eval_sharded_device(comm, sd, xd.data_ptr(), gd.data_ptr()), sr.EUNSUPPORTED, "a hold-out is not sharded")
    assert fake.calls == []
    # a 2-fold path on 70 observations runs end to end
    xs, table, fold_table, chosen, rep = p.solve_lambda_path_folds(x, [1.0, 0.5], folds=2)
    assert np.all(np.isfinite(xs)) and len(table) == 2 and p.holdout_fold() == (2, 1, 1)


# ------------------------------------------------------------------------------------------------ the layers above
def test_host_facade_runs_the_path_as_the_calls_it_is_made_of():
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "super-resolution_amd", "lib", "holdout_folds_facade_test")
    assert os.path.exists(exe), "build() makes the facade test binary"
    o = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(o.stdout, o.stderr)
    assert o.returncode == 0 and "HOLDOUT FOLDS FACADE TESTS PASSED" in o.stdout


def test_the_tool_chooses_lambda_by_cross_validation(tmp_path):
    """generate_data makes the noisy 48 x 64 burst of tests/test_gpu_holdout.py's tool run; super_resolution --holdout_folds=3
    --lambda_path=0.32:0.5:5 prints a table of 5 rows with mean +- se, marks the least mean and the chosen row as the rules of
    the restatement give them, and its result is the plain run at the chosen lambda: the same PSNR line."""
    import re
    import subprocess
    import affine_restatement as ar
    from conftest import ROOT
    from test_gpu_apps import _write_envi
    libdir = os.path.join(ROOT, "super-resolution_amd", "lib")
    gen, srbin = os.path.join(libdir, "generate_data"), os.path.join(libdir, "super_resolution")
    assert os.path.exists(gen) and os.path.exists(srbin), "build() makes the tools"
    C_, H, W, s, K = 1, 48, 64, 2, 4
    rng = np.random.default_rng(21)
    gt = np.clip(0.8 * rr.prototype_ground_truth(C_, H, W) + 0.1 * rng.random((C_, H, W)), 0, 1).astype(np.float32).astype(np.float64)
    gt_cfg = _write_envi(str(tmp_path / "gt"), gt)
    motion = tmp_path / "motion.txt"
    motion.write_text("".join("%r %r\n" % (float(a), float(b)) for a, b in ar.TABLE_SHIFTS[:K]))
    lr_dir = tmp_path / "lr"
    lr_dir.mkdir()
    out = subprocess.run([gen, "--input_image=" + gt_cfg, "--output_image_dir=" + str(lr_dir), "--motion_sequence_path=" + str(motion),
                          "--blur_radius=3", "--blur_sigma=1.0", "--downsampling_scale=%d" % s, "--number_of_frames=%d" % K,
                          "--noise_sigma=%r" % (0.03 * 255)], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    base = [srbin, "--data_path=" + str(lr_dir), "--ground_truth_image=" + gt_cfg, "--upsampling_scale=%d" % s, "--blur_radius=3",
            "--blur_sigma=1.0", "--motion_sequence_path=" + str(motion), "--regularizer=btv", "--btv_scale_range=2",
            "--optimization_iterations=5", "--solver_iterations=30", "--evaluators=psnr"]

    def run(*flags):
        o = subprocess.run(base + list(flags), capture_output=True, text=True, timeout=600)
        print(o.stdout, o.stderr)
        assert o.returncode == 0
        return o.stdout, [l for l in o.stdout.splitlines() if l.startswith("PSNR score on result")][0]

    held = int(K * C_ * (H // s) * (W // s))  # the folds partition the pixels: pooled, all of them
    for word, rule, factor in (("one_se", hfr.RULE_ONE_SE, 1.0), ("min", hfr.RULE_MIN, 1.0), ("one_se", hfr.RULE_ONE_SE, 4.0)):
        text, psnr_line = run("--holdout_folds=3", "--holdout_seed=2", "--lambda_path=0.32:0.5:5", "--lambda_rule=" + word,
                              "--lambda_se_factor=%r" % factor, "--print_lambda_path")
        head = re.search(r"Lambda path, 3 folds, rule (\S+): 5 of 5 rows, chosen lambda (\S+) \(row (\d), mean score (\S+) \+- (\S+); "
                         r"least mean at row (\d)\)\.", text)
        rows = re.findall(r"^  lambda (\S+): mean score (\S+) \+- (\S+) over (\d+) held-out pixels.*?delta \S+?(  <- least mean)?(  <- chosen)?$",
                          text, flags=re.M)
        assert head and len(rows) == 5 and head.group(1) == word
        lambdas, mean, se = ([float(r[i]) for r in rows] for i in range(3))
        assert np.allclose(lambdas, [0.32 * 0.5 ** j for j in range(5)], rtol=1e-8) and all(int(r[3]) == held for r in rows)
        want, jstar = hfr.choose_folds(mean, se, rule, factor)
        chosen = int(head.group(3))
        assert (chosen, int(head.group(6))) == (want, jstar) and float(head.group(2)) == lambdas[chosen]
        assert [bool(r[4]) for r in rows] == [j == jstar for j in range(5)] and [bool(r[5]) for r in rows] == [j == chosen for j in range(5)]
        assert "Hold-out score of the result" not in text  # no hold-out is in force after the path
        if factor == 1.0:
            plain, plain_line = run("--regularization_parameter=%r" % (0.32 * 0.5 ** chosen))
            assert plain_line == psnr_line and "Lambda path" not in plain
