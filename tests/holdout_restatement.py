"""numpy restatement of hold-out validation (include/srmap.h: srmap_problem_set_holdout, srmap_holdout_score,
srmap_solve_lambda_path), from the definitions alone -- the checker of tests/test_holdout_cpu.py and
tests/test_gpu_holdout.py.

  mask    observation i (flat index into [K][C][h][w]) is held out iff (z >> 40) < T, T = floor(fraction * 2^24),
          z = i + seed * 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;
          z ^= z >> 31                                                                                  (all mod 2^64)
  score   over the held-out observations, per frame: S1 = sum u rho(r), S2 = sum u rho(r)^2, S0 = sum u, n = #{u > 0};
          score[0] = sum_k S1_k / sum_k S0_k, score[1 + k] = S1_k / S0_k (0 where S0_k = 0);  rho(r) = r^2 for delta == 0
          or |r| <= delta, 2 delta |r| - delta^2 beyond;  u = the caller's prior times (under L2) the caller's weights
  path    per scale: the lambdas times the scale, the solve of data_prior_restatement / robust_restatement from x0 with the
          prior m .* (1 - h), the score;  chosen = the first minimum;  the final solve on all observations
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GOLDEN, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
M64 = (1 << 64) - 1


def hash_one(i, seed):
    """The mix of (i, seed) in Python integers."""
    z = (i + seed * GOLDEN) & M64
    z = ((z ^ (z >> 30)) * MIX1) & M64
    z = ((z ^ (z >> 27)) * MIX2) & M64
    return z ^ (z >> 31)


def threshold(fraction):
    """T = floor(fraction * 2^24) in double; 0 where the fraction is refused."""
    if not (0.0 < fraction <= 0.5):
        return 0
    return int(np.floor(np.float64(fraction) * np.float64(1 << 24)))


def mask(shape, fraction, seed):
    """h [K][C][h][w] of 0.0 / 1.0 (uint64 arithmetic wraps as the definition asks)."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64((seed * GOLDEN) & M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)) < np.uint64(threshold(fraction))).astype(np.float64).reshape(shape)


def rho(r, delta):
    r = np.asarray(r, dtype=np.float64)
    if delta == 0:
        return r * r
    a = np.abs(r)
    return np.where(a <= delta, r * r, 2.0 * delta * a - delta * delta)


def base_weight(shape, prior=None, weights=None, huber=False, dtype=np.float64):
    """u: the caller's prior times (under L2) the caller's weights, each rounded to the problem's dtype, the product
    rounded once in it."""
    u = np.ones(shape, dtype=dtype)
    if prior is not None:
        u = np.asarray(prior, dtype=np.float64).astype(dtype).reshape(shape)
    if weights is not None and not huber:
        u = (u * np.asarray(weights, dtype=np.float64).astype(dtype).reshape(shape)).astype(dtype)
    return u.astype(np.float64)


def score(r, h, u, delta, rng=None):
    """(score [1 + K], sums [1 + K][4]) of residuals r [K][C][h][w] with the mask h and the base weights u.  rng: the sums
    are taken over a random permutation of every frame's observations instead (the sensitivity to the order)."""
    K = r.shape[0]
    sums = np.zeros((1 + K, 4))
    for k in range(K):
        rk, hk, uk = (np.asarray(a, dtype=np.float64)[k].ravel() for a in (r, h, u))
        if rng is not None:
            perm = rng.permutation(rk.size)
            rk, hk, uk = rk[perm], hk[perm], uk[perm]
        sel = hk > 0
        rh, uh = rho(rk[sel], delta), uk[sel]
        sums[1 + k] = [np.sum(uh * rh), np.sum(uh * rh * rh), np.sum(uh), np.count_nonzero(uh > 0)]
    for k in range(K):
        sums[0] += sums[1 + k]
    sc = np.zeros(1 + K)
    sc[0] = sums[0, 0] / sums[0, 2] if sums[0, 2] != 0 else 0.0
    for k in range(K):
        sc[1 + k] = sums[1 + k, 0] / sums[1 + k, 2] if sums[1 + k, 2] != 0 else 0.0
    return sc, sums


def score_sensitivity(r, h, u, delta, seed=0):
    """|score - score over a permuted order| / |score|, per entry of score: what the order of summation alone moves."""
    a, _ = score(r, h, u, delta)
    b, _ = score(r, h, u, delta, rng=np.random.default_rng(seed))
    return np.abs(a - b) / np.maximum(np.abs(a), np.finfo(np.float64).tiny)


def choose(scores):
    """The first minimum: a tie goes to the earlier row, the larger lambda."""
    best = -1
    for j, s in enumerate(scores):
        if s == s and (best < 0 or s < scores[best]):
            best = j
    return best


def patience_stop(scores, patience):
    """Whether a path stops after these rows: the score rose `patience` rows in a row."""
    n = len(scores)
    if patience <= 0 or n <= patience:
        return False
    return all(scores[j] > scores[j - 1] for j in range(n - patience, n))


def solve(model, y, x0, reg, prior, huber_delta=None, options=None, use_alglib=None):
    """One solve with the prior `prior` (None: none): L2 through robust_restatement, Huber through data_prior_restatement."""
    import data_prior_restatement as dpr
    import robust_restatement as rr
    if huber_delta is None:
        x, rep, _ = rr.irls_solve(model, y, x0, reg=reg, loss="l2", weights=prior, options=options, use_alglib=use_alglib)
    elif prior is None:
        x, rep, _ = rr.irls_solve(model, y, x0, reg=reg, loss="huber", delta=huber_delta, options=options, use_alglib=use_alglib)
    else:
        x, rep, _ = dpr.irls_solve(model, y, x0, prior, reg=reg, delta=huber_delta, options=options, use_alglib=use_alglib)
    return x, rep


def lambda_path(model, y, x0, reg, scales, fraction, seed, prior=None, huber_delta=None, score_delta=None, patience=0,
                final_solve=True, options=None, use_alglib=None):
    """srmap_solve_lambda_path for one regulariser reg = (kind, lambda, btv_range, btv_decay).  score_delta None: the
    path's (0 under L2, huber_delta under Huber).  Returns dict(x, rows = [dict(scale, score, sums, x, report)], chosen)."""
    import robust_restatement as rr
    y = np.asarray(y, dtype=np.float64)
    h = mask(y.shape, fraction, seed)
    m = (1.0 - h) if prior is None else np.asarray(prior, dtype=np.float64) * (1.0 - h)
    u = base_weight(y.shape, prior=prior)
    if score_delta is None:
        score_delta = 0.0 if huber_delta is None else huber_delta
    rows, scores = [], []
    for sc in scales:
        rg = (reg[0], reg[1] * sc, reg[2], reg[3])
        x, rep = solve(model, y, x0, rg, m, huber_delta, options, use_alglib)
        s, sums = score(rr.residuals(model, y, x), h, u, score_delta)
        rows.append(dict(scale=sc, score=s[0], scores=s, sums=sums, x=x, report=rep))
        scores.append(s[0])
        if patience_stop(scores, patience):
            break
    chosen = choose(scores)
    out = rows[chosen]["x"]
    if final_solve:
        rg = (reg[0], reg[1] * scales[chosen], reg[2], reg[3])
        out, _ = solve(model, y, x0, rg, prior, huber_delta, options, use_alglib)
    return dict(x=out, rows=rows, chosen=chosen, mask=h)
