"""csrc/affine_map.hpp, the one copy of the motion fits' host algebra (tests/cpp/affine_map_test.cpp), CPU only: the
program's built-in cases, and its functions against the Python restatements of the same name on inputs where double
arithmetic is exact (dyadic entries, unit-determinant linear parts, integer Cholesky factors) -- every comparison is
equality."""
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_registration_restatement as rg  # noqa: E402
import motion_refinement_restatement as mr  # noqa: E402

SHEAR_X = [1.0, 0.25, 0.375, 0.0, 1.0, -1.125]
SHEAR_Y = [1.0, 0.0, -2.5, 0.5, 1.0, 0.625]
BOTH = [1.5, 0.25, 3.125, 2.0, 1.0, -0.875]  # determinant 1
MAPS = [SHEAR_X, SHEAR_Y, BOTH]
# increments whose W = I + D has determinant 1: a shear each way; translations in multiples of 1/8
DELTAS = [[0.0, 0.25, 0.625, 0.0, 0.0, -0.375], [0.0, 0.0, -1.125, 0.5, 0.0, 0.25]]
W, H = 9, 17  # centre (4, 8)


def _exe():
    import __graft_entry__ as ge
    exe = ge.build_affine_map_test()
    assert exe and os.path.exists(exe)
    return exe


def _call(fn, *numbers):
    out = subprocess.run([_exe(), fn] + [repr(float(v)) for v in numbers], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (fn, out.stdout, out.stderr)
    text = out.stdout.strip()
    return None if text == "none" else np.array([float(t) for t in text.split()])


def _same(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel())


def test_built_in_cases():
    out = subprocess.run([_exe()], capture_output=True, text=True, timeout=60)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "AFFINE MAP TESTS PASSED" in out.stdout


def test_map_algebra_equals_the_restatements():
    for F in MAPS:
        assert _same(_call("deviation", *F), [rg.deviation(F)])
        assert _same(_call("to_finer", *F), rg.to_finer(F))
        assert _same(_call("to_coarser", *F), rg.to_coarser(F))
        assert _same(_call("to_coarser", *_call("to_finer", *F)), F)
        assert _same(_call("inverse", *_call("inverse", *F)), F)
        # the inverse is the restatement's composition of the identity with F^-1
        assert _same(_call("inverse", *F), rg.compose_with_inverse(rg.identity(), np.reshape(F, (2, 3))))
        for G in MAPS:
            assert _same(_call("corner_displacement", *F, *G, W, H), [rg.corner_displacement(F, G, W, H)])
        for d in DELTAS:
            assert _same(_call("compose_with_inverse", *F, *d, W, H),
                         rg.compose_with_inverse(F, rg.increment_matrix(d, W, H)))
            assert _same(_call("increment", *F, *d, W, H), mr.increment(F, d, W, H))
    T = list(SHEAR_X)
    T[2] += 0.375
    T[5] += 0.5
    assert _same(_call("corner_displacement", *T, *SHEAR_X, W, H), [0.625])  # a translation by (3/8, 1/2)


def _integer_system(L, x):
    L = np.array(L, dtype=np.float64)
    A = L @ L.T
    return A, A @ np.array(x, dtype=np.float64)


L6 = [[2, 0, 0, 0, 0, 0], [1, 3, 0, 0, 0, 0], [0, 0, 2, 0, 0, 0], [2, 1, 1, 1, 0, 0], [1, 0, 3, 2, 2, 0], [2, 1, 1, 2, 0, 4]]
X6 = [3, -2, 5, 1, -4, 2]


def _solve(A, rhs):
    n = len(rhs)
    got = _call("cholesky_solve", n, *np.asarray(A).ravel(), *rhs)
    want = rg.cholesky_solve(np.asarray(A, dtype=np.float64), np.asarray(rhs, dtype=np.float64))
    assert (got is None) == (want is None)
    if want is not None:
        assert _same(got, want)
    return got


def test_cholesky_solve_is_exact_on_integer_factors():
    A, rhs = _integer_system(L6, X6)
    assert _same(_solve(A, rhs), X6)


def test_cholesky_solve_of_the_translation_sub_system():
    """The 2 x 2 system on the indices {2, 5} as the refinement's LM step forms it, lambda = 0 and 1."""
    A6, _ = _integer_system(L6, X6)
    H1 = np.zeros((6, 6))
    H1[2, 2], H1[2, 5], H1[5, 2], H1[5, 5] = 2.0, 2.0, 2.0, 5.0  # diagonal doubles to [[4, 2], [2, 10]] = [[2, 0], [1, 3]] [..]^T
    x = np.array([7.0, -3.0])
    for lam, Hm in ((0.0, A6), (1.0, H1)):
        idx = [2, 5]
        A = Hm[np.ix_(idx, idx)].copy()
        for i in range(2):
            A[i, i] = A[i, i] + lam * A[i, i]
        assert _same(_solve(A, A @ x), x)
        # and through the restatement's own LM step: S = the 21 sums of H, g = -A x at the indices, E
        S = np.zeros(28)
        S[:21] = Hm[np.triu_indices(6)]
        S[21 + 2], S[21 + 5] = -(A @ x)
        assert _same(mr.lm_step(S, lam, 2), [0, 0, x[0], 0, 0, x[1]])


def test_cholesky_solve_refuses_where_the_restatement_does():
    A, rhs = _integer_system(L6, X6)
    Z = A.copy()
    Z[3, 3] = 0.0
    assert _solve(Z, rhs) is None
    Z = A.copy()
    Z[0, 0] = -4.0
    assert _solve(Z, rhs) is None
    Ld = [row[:] for row in L6]
    Ld[2] = Ld[1][:]  # two equal rows of the factor: two equal columns of A
    Z, rhs = _integer_system(Ld, X6)
    assert np.array_equal(Z[:, 1], Z[:, 2])
    assert _solve(Z, rhs) is None


def test_search_separation():
    def sep(t, best):
        return _call("search_separation", 5, best, *t)[0]
    t = np.full(25, 4.0)
    t[12] = 1.0
    assert sep(t, 12) == 0.75  # one clear minimum
    t = np.full(25, 8.0)
    t[12], t[13], t[6] = 1.0, 2.0, 2.0
    assert sep(t, 12) == 0.875  # the 2s lie inside the 3 x 3 exclusion zone
    t[0], t[24], t[4] = -1.0, -1.0, 2.0
    assert sep(t, 12) == 0.5  # -1: not evaluated, skipped; the 2 two cells away counts
    # the fixed-window search of the restatement on a table with no negative entry
    rng = np.random.default_rng(5)
    t = rng.integers(2, 9, 25).astype(np.float64)
    t[7] = 1.0
    far = [c for c in range(25) if max(abs(c % 5 - 7 % 5), abs(c // 5 - 7 // 5)) >= 2]
    assert sep(t, 7) == 1.0 - 1.0 / min(t[c] for c in far)
