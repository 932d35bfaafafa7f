"""csrc/solver_host.hpp, the solvers' host arithmetic (tests/cpp/solver_host_test.cpp), CPU only, against
tests/lbfgs_restatement.py (bit-exact against ALGLIB, tests/test_lbfgs_cpu.py): the More'-Thuente step mt_step against
mcstep, the L-BFGS recursion on coefficients lbfgs_two_loop against _gram_direction.  Both sides are the same IEEE
double operations in the same order and neither build contracts a * b + c, so every comparison is equality of bits.
Further the unpacking of the update pass's rows into the Gram tables (lbfgs_unpack_rows) against numpy, and the polling
decision of csrc/solver_mailbox.hpp (poll_tag) on plain host memory."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_restatement as lr  # noqa: E402


def _run(lines):
    import __graft_entry__ as ge
    exe = ge.build_solver_host_test()
    assert exe and os.path.exists(exe)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stdout[-500:], out.stderr[-500:])
    rows = out.stdout.strip().split("\n")
    assert len(rows) == len(lines)
    return rows


def _hex(values):
    return " ".join(float(v).hex() for v in values)


def _bits(values):
    return np.asarray(values, dtype=np.float64).view(np.int64)


# ---- mt_step ------------------------------------------------------------------------------------------------------
FUNCTIONS = {
    "quadratic": lambda x: ((x - 2.0) ** 2, 2.0 * (x - 2.0)),
    "quartic with an inflection": lambda x: (x ** 4 - 2.0 * x ** 3 + 2.0 * x, 4.0 * x ** 3 - 6.0 * x ** 2 + 2.0),
    "-x / (x^2 + 2)": lambda x: (-x / (x * x + 2.0), (x * x - 2.0) / (x * x + 2.0) ** 2),
}
STARTS = (-3.0, -0.5, 0.25)
STEPS = (1.0e-3, 0.1, 1.0, 7.0, 300.0)
GTOLS = (0.001, 0.3, 0.4, 0.9)   # 0.3: mincg, 0.4: minlbfgs; the others reach the steps those rarely take

# the early return (info 0): a bracketed step on or outside the bracket, a step that is no descent step from stx, an
# empty [stmin, stmax]
HAND_MADE = [
    # stx, fx, dx, sty, fy, dy, stp, fp, dp, brackt, stmin, stmax
    (0.0, 1.0, -1.0, 2.0, 1.5, 0.5, 2.0, 1.5, 0.5, True, 0.0, 2.0),
    (0.0, 1.0, -1.0, 2.0, 1.5, 0.5, 0.0, 1.0, -1.0, True, 0.0, 2.0),
    (0.0, 1.0, -1.0, 2.0, 1.5, 0.5, 3.0, 2.0, 1.0, True, 0.0, 2.0),
    (1.0, 1.0, -1.0, 0.0, 1.5, 0.5, 0.5, 0.9, -0.5, False, 0.0, 5.0),
    (1.0, 1.0, 1.0, 0.0, 1.5, 0.5, 1.5, 0.9, -0.5, False, 0.0, 5.0),
    (0.0, 1.0, -1.0, 0.0, 1.0, -1.0, 1.0, 0.5, -0.25, False, 5.0, 4.0),
]


def _recorded_cases():
    """The argument tuples of every mcstep call while the restatement's mcsrch minimises the 1-D functions."""
    cases = []
    inner = lr.mcstep

    def recording(b, stp, fp, dp, brackt, stmin, stmax):
        cases.append(tuple(b) + (stp, fp, dp, bool(brackt), stmin, stmax))
        return inner(b, stp, fp, dp, brackt, stmin, stmax)

    lr.mcstep = recording
    try:
        for fun in FUNCTIONS.values():
            def fg(x, fun=fun):
                f, g = fun(float(x[0]))
                return f, np.array([g])
            for x0 in STARTS:
                f0, g0 = fg(np.array([x0]))
                if g0[0] == 0.0:
                    continue
                d = np.array([-1.0 if g0[0] > 0 else 1.0])
                for stp in STEPS:
                    for gtol in GTOLS:
                        lr.mcsrch(fg, np.array([x0]), f0, g0.copy(), d, stp, gtol, 1.0e300, None)
    finally:
        lr.mcstep = inner
    return cases


@pytest.fixture(scope="module")
def mt_cases():
    """(arguments, mcstep's result) of the recorded and the hand-made cases, and mt_step's output rows."""
    args = _recorded_cases() + HAND_MADE
    want = []
    for a in args:
        b = list(a[:6])
        stp, brackt, info = lr.mcstep(b, a[6], a[7], a[8], a[9], a[10], a[11])
        want.append((b + [stp], bool(brackt), info))
    rows = _run(["mt " + _hex(a[:9]) + " %d " % a[9] + _hex(a[10:]) for a in args])
    return args, want, rows


def test_mt_step_cases_cover_every_branch(mt_cases):
    """Every info value 0-4, and each of 1-4 entered both with and without a bracket (1 and 2 leave with one)."""
    args, want, _ = mt_cases
    seen = {(info, a[9]) for a, (_, _, info) in zip(args, want)}
    print(len(args), "cases;", sorted(seen))
    assert {info for info, _ in seen} == {0, 1, 2, 3, 4}
    for info in (1, 2, 3, 4):
        assert (info, False) in seen and (info, True) in seen, info
    assert all(brackt for (_, brackt, info) in want if info in (1, 2))
    assert sum(1 for (_, _, info) in want if info == 0) >= len(HAND_MADE)


def test_mt_step_equals_mcstep(mt_cases):
    args, want, rows = mt_cases
    for a, (nums, brackt, info), row in zip(args, want, rows):
        t = row.split()
        got = [float.fromhex(v) for v in t[:7]]
        assert np.array_equal(_bits(got), _bits(nums)), (a, got, nums)
        assert (int(t[7]), int(t[8])) == (int(brackt), info), (a, t[7:], brackt, info)


# ---- lbfgs_two_loop -----------------------------------------------------------------------------------------------
N = 7
# (m, k): k below m - 1, at m - 1, and beyond it so that the ring wraps (slot p = k % m, q = min(k, m - 1))
RING = [(1, 0), (1, 3), (3, 0), (3, 1), (3, 2), (3, 4), (3, 7), (8, 3), (8, 7), (8, 11), (8, 17)]


def _history(m, k, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(N)
    sk = rng.standard_normal((m, N))
    yk = sk + 0.3 * rng.standard_normal((m, N))  # s.y > 0, as after an accepted line search
    q = min(k, m - 1)
    return g, sk, yk, q


def _tables(g, sk, yk, m):
    """The Gram tables as _gram_direction forms them."""
    SY = [lr.dot(sk[a], yk[b]) for a in range(m) for b in range(m)]
    YY = [lr.dot(yk[a], yk[b]) for a in range(m) for b in range(m)]
    gs = [lr.dot(g, sk[j]) for j in range(m)]
    gy = [lr.dot(g, yk[j]) for j in range(m)]
    return SY, YY, gs, gy


def _line(m, k, q, tables, rho):
    return "tl %d %d %d " % (m, k, q) + " ".join(_hex(t) for t in tables) + " " + _hex(rho)


def test_two_loop_equals_the_restatement():
    cases, lines = [], []
    for i, (m, k) in enumerate(RING):
        g, sk, yk, q = _history(m, k, 100 + i)
        rho = np.array([1 / lr.dot(sk[j], yk[j]) for j in range(m)])
        given = rho.copy()
        given[k % m] = -7.0  # the function sets the newest slot's rho itself
        cases.append((m, k, q, g, sk, yk, rho))
        lines.append(_line(m, k, q, _tables(g, sk, yk, m), given))
    for (m, k, q, g, sk, yk, rho), row in zip(cases, _run(lines)):
        t = [float.fromhex(v) for v in row.split()]
        live = q + 1
        assert len(t) == 2 + 2 * live
        assert _bits([t[0]]) == _bits([rho[k % m]])
        cgc, cs, cy = t[1], t[2::2], t[3::2]
        w = cgc * g  # the direction from the coefficients, in _gram_direction's order
        for j in range(live):
            w = w + cs[j] * sk[j] + cy[j] * yk[j]
        want = lr._gram_direction(g, sk, yk, rho, k, q, m, False)
        assert np.all(np.isfinite(want)) and np.any(want != 0.0)
        assert np.array_equal(_bits(-w), _bits(want)), (m, k)


def test_two_loop_reports_a_zero_curvature_pair():
    m, k = 3, 4
    lines = []
    g, sk, yk, q = _history(m, k, 7)
    pp = (k % m) * m + k % m
    SY, YY, gs, gy = _tables(g, sk, yk, m)
    lines.append(_line(m, k, q, (SY, YY, gs, gy), np.ones(m)))
    for table in (SY, YY):  # v = s_p.y_p == 0, then vv = y_p.y_p == 0
        t = list(table)
        t[pp] = 0.0
        lines.append(_line(m, k, q, (t, YY, gs, gy) if table is SY else (SY, t, gs, gy), np.ones(m)))
    rows = _run(lines)
    assert rows[0] != "none" and rows[1:] == ["none", "none"]


# ---- lbfgs_unpack_rows --------------------------------------------------------------------------------------------
def test_unpack_rows_equals_numpy():
    """The rows [g.g, s.s, then per slot j: s.y_j, y.s_j, y.y_j, g.s_j, g.y_j] into row / column p of the tables; every
    other entry keeps its bits.  p at both ends of the ring, every live count."""
    rng = np.random.default_rng(29)
    cases, lines = [], []
    for m in (1, 3, 8):
        for live in range(1, m + 1):
            for p in sorted({0, m - 1}):
                SY, YY = rng.standard_normal((m, m)), rng.standard_normal((m, m))
                gs, gy = rng.standard_normal(m), rng.standard_normal(m)
                rows = rng.standard_normal(2 + 5 * live)
                lines.append("up %d %d %d " % (m, p, live) + " ".join(_hex(t.ravel()) for t in (SY, YY, gs, gy, rows)))
                per = rows[2:].reshape(live, 5)
                SY[p, :live] = per[:, 0]
                SY[:live, p] = per[:, 1]   # j == p: s_p.y_p is summed twice, the second sum stays
                YY[p, :live] = per[:, 2]
                YY[:live, p] = per[:, 2]
                gs[:live] = per[:, 3]
                gy[:live] = per[:, 4]
                cases.append((m, p, live, np.concatenate([SY.ravel(), YY.ravel(), gs, gy])))
    assert len(cases) == len(lines) == 1 + 2 * 3 + 2 * 8
    for (m, p, live, want), row in zip(cases, _run(lines)):
        got = [float.fromhex(v) for v in row.split()]
        assert np.array_equal(_bits(got), _bits(want)), (m, p, live)


# ---- poll_tag -----------------------------------------------------------------------------------------------------
def test_poll_tag_decisions():
    """Single-threaded on plain host memory: nothing changes the words while the call polls them."""
    rows = _run([
        "pt 7 0 7 0.003",    # the wanted tag is there
        "pt 9 0 7 0.003",    # a later kernel's tag: arrived all the same (tags only grow)
        "pt 7 1 7 0.003",    # arrived wins over a raised time-out word
        "pt 6 1 7 0.003",    # not there and the device gave up
        "pt 6 0 7 0.003",    # neither: the budget runs out
        "pt nan 0 7 0.003",  # a word that compares false is not an arrival
    ])
    assert rows == ["arrived", "arrived", "arrived", "timeout", "expired", "expired"]
