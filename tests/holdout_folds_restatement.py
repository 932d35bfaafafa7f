"""numpy restatement of the hold-out given as a fold and of the cross-validated lambda path (include/srmap.h:
srmap_problem_set_holdout_fold, srmap_solve_lambda_path_folds), from the definitions alone, over tests/holdout_restatement.py
-- the checker of tests/test_holdout_folds_cpu.py and tests/test_gpu_holdout_folds.py.

  band    observation i is held out iff lo <= v < hi, v = the top 24 bits of holdout_restatement's mix of (i, seed).  A
          fraction is the band [0, T); fold f of F is [floor(f 2^24 / F), floor((f + 1) 2^24 / F)) in integers
  stats   mean = (sum_f s[f]) / F added in fold order;  se = sqrt(sum_f (s[f] - mean)^2 / (F - 1) / F)
  choice  j* = the first minimum of mean;  MIN: j*;  ONE_SE: the smallest j with mean[j] <= mean[j*] + se_factor * se[j*]
  path    rows outside, folds inside: per scale and fold the lambdas times the scale, the solve from x0 with the prior
          m .* (1 - h_f), the score of fold f;  the final solve on all observations at the chosen lambdas
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import holdout_restatement as hr  # noqa: E402

BITS = 24
RULE_MIN, RULE_ONE_SE = 0, 1


def fold_band(folds, fold):
    """(lo, hi) of fold `fold` of `folds`, in Python integers; None where the pair is refused."""
    if not (2 <= folds <= 32 and 0 <= fold < folds):
        return None
    return (fold << BITS) // folds, ((fold + 1) << BITS) // folds


def hash24(n, seed):
    """The top 24 bits of the mix for the indices 0 ... n - 1 (uint64 arithmetic wraps as the definition asks)."""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64((seed * hr.GOLDEN) & hr.M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(hr.MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(hr.MIX2)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(64 - BITS)).astype(np.int64)


def band_mask(shape, lo, hi, seed):
    """h [K][C][h][w] of 0.0 / 1.0 for the band [lo, hi)."""
    v = hash24(int(np.prod(shape)), seed)
    return ((v >= lo) & (v < hi)).astype(np.float64).reshape(shape)


def fold_mask(shape, folds, fold, seed):
    lo, hi = fold_band(folds, fold)
    return band_mask(shape, lo, hi, seed)


def fold_stats(s):
    """(mean, se) of the fold scores s, every operation in the stated order."""
    F = len(s)
    total = 0.0
    for v in s:
        total += float(v)
    mean = total / F
    ss = 0.0
    for v in s:
        ss += (float(v) - mean) * (float(v) - mean)
    return mean, float(np.sqrt(ss / (F - 1) / F))


def choose_folds(mean, se, rule=RULE_ONE_SE, se_factor=1.0):
    """(chosen, jstar): jstar the first minimum of the means that are numbers (-1: none); the rule's row."""
    jstar = hr.choose(list(mean))
    if jstar < 0 or rule != RULE_ONE_SE:
        return jstar, jstar
    bar = mean[jstar] + se_factor * se[jstar]
    for j in range(jstar):
        if mean[j] <= bar:  # False for a mean that is not a number
            return j, jstar
    return jstar, jstar


def pixel_se(sums):
    """The per-pixel standard error that S1, S2, S0 and n give for the score S1 / S0: sqrt((S2 / S0 - (S1 / S0)^2) / n)."""
    s1, s2, s0, n = (float(v) for v in sums)
    return float(np.sqrt(max(s2 / s0 - (s1 / s0) ** 2, 0.0) / n))


def lambda_path_folds(model, y, x0, reg, scales, folds=5, seed=1, rule=RULE_ONE_SE, se_factor=1.0, prior=None, huber_delta=None,
                      score_delta=None, patience=0, final_solve=True, options=None, use_alglib=None):
    """srmap_solve_lambda_path_folds for one regulariser reg = (kind, lambda, btv_range, btv_decay).  Returns dict(x, rows =
    [dict(scale, mean, se, pooled, folds = [dict(score, sums, report)])], chosen, jstar)."""
    import robust_restatement as rr
    y = np.asarray(y, dtype=np.float64)
    masks = [fold_mask(y.shape, folds, f, seed) for f in range(folds)]
    u = hr.base_weight(y.shape, prior=prior)
    if score_delta is None:
        score_delta = 0.0 if huber_delta is None else huber_delta
    rows, means, ses = [], [], []
    for sc in scales:
        rg = (reg[0], reg[1] * sc, reg[2], reg[3])
        per_fold, pooled = [], np.zeros(4)
        for h in masks:
            m = (1.0 - h) if prior is None else np.asarray(prior, dtype=np.float64) * (1.0 - h)
            x, rep = hr.solve(model, y, x0, rg, m, huber_delta, options, use_alglib)
            s, sums = hr.score(rr.residuals(model, y, x), h, u, score_delta)
            per_fold.append(dict(score=s[0], sums=sums, report=rep))
            pooled += sums[0]
        mean, se = fold_stats([f["score"] for f in per_fold])
        rows.append(dict(scale=sc, mean=mean, se=se, pooled=pooled, folds=per_fold))
        means.append(mean)
        ses.append(se)
        if hr.patience_stop(means, patience):
            break
    chosen, jstar = choose_folds(means, ses, rule, se_factor)
    out = None
    if final_solve:
        rg = (reg[0], reg[1] * scales[chosen], reg[2], reg[3])
        out, _ = hr.solve(model, y, x0, rg, prior, huber_delta, options, use_alglib)
    return dict(x=out, rows=rows, chosen=chosen, jstar=jstar)
