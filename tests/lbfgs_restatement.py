"""ALGLIB 3.10.0's L-BFGS (minlbfgs, libs/alglib/src/optimization.cpp:21640 ff.) restated in numpy, default
preconditioner, unit scales, no stpmax, analytic gradient: the configuration the reference drives
(src/optimization/alglib_objective.cpp:111-140).  It follows ALGLIB operation by operation, so it reproduces ALGLIB's
trajectory bit for bit (tests/test_lbfgs_cpu.py checks it against tests/golden/lbfgs_trajectories.json):

  - ae_v_dotproduct (ap.cpp:4667-4692) adds the products in groups of four, ((a0 b0 + a1 b1) + a2 b2) + a3 b3, the
    group sums in sequence, then the remainder in sequence (``dot``);
  - the norm loops of the stopping rules and of mcsrch are sequential sums (``seqsum``);
  - numpy does not contract a * b + c into an FMA, and neither does the oracle's build of ALGLIB (-ffp-contract=off);
  - mcsrch / mcstep (alglibinternal.cpp:12313-12632, 12972-13232), linminnormalized (:12165-12196) and trimfunction
    are restated below.

Two opt-in hooks, both off by default (the restatement is then ALGLIB bit for bit), serve the solver matrix
(tests/solver_matrix.py): ``store=np.float32`` rounds x, g, s, y and d where the device solver stores T (run_lbfgs,
kernels_lbfgs.hip), and ``plant=(kind, arg)`` plants one plausible pass bug (tests/test_solver_matrix_cpu.py shows that the
matrix's bars catch it):
  ("lose", keep)      the elements from index keep on are left out of s, y and every sum the L-BFGS passes reduce (a
                      ragged tail on the vector path: keep = n - n % V; a skipped grid-stride round: keep = nb 256 V)
  ("swap", None)      the direction formed from the Gram table as run_lbfgs does, with s_p.y_j and y_p.s_j swapped
  ("drop_oldest", None)  once the ring has wrapped, the oldest live pair is left out of the two loops
  ("maxsum", None)    max|d| of linminnormalized reduced as a sum

``irls_adapter(m)`` wraps it in the oracle's sro_cg_fn signature (oracle/srmap_oracle.h), so the oracle's own IRLS loop
(``sro_irls_solve``) runs with L-BFGS as its inner solver.  Test infrastructure only."""
import ctypes as C
import math

import numpy as np

GTOL = 0.4            # minlbfgs_gtol, optimization.cpp:8941
FTOL, XTOL = 0.001, 100 * 5e-16   # linmin_ftol, linmin_xtol (ae_machineepsilon = 5e-16)
STPMIN, STPMAX = 1.0e-50, 1.0e+50
MAXFEV = 20


def seqsum(v):
    """v[0] + v[1] + ... in index order (np.add.accumulate is sequential)."""
    return float(np.add.accumulate(v)[-1]) if v.size else 0.0


def dot(a, b):
    """ae_v_dotproduct: groups of four, the groups added in sequence, then the remainder."""
    n = a.size
    n4 = (n // 4) * 4
    p = a * b
    r = 0.0
    if n4:
        grp = ((p[0:n4:4] + p[1:n4:4]) + p[2:n4:4]) + p[3:n4:4]
        r = float(np.add.accumulate(np.concatenate(([0.0], grp)))[-1])
    for i in range(n4, n):
        r += float(p[i])
    return r


def _cubic_gamma(theta, da, db, clamp0):
    s = max(abs(theta), max(abs(da), abs(db)))
    t = (theta / s) * (theta / s) - da / s * (db / s)
    if clamp0:
        t = max(0.0, t)
    return s * math.sqrt(t)


def mcstep(b, stp, fp, dp, brackt, stmin, stmax):
    """linmin_mcstep on the bracket b = [stx, fx, dx, sty, fy, dy] (updated in place); returns (stp, brackt, info)."""
    stx, fx, dx, sty, fy, dy = b
    if (brackt and (stp <= min(stx, sty) or stp >= max(stx, sty))) or dx * (stp - stx) >= 0 or stmax < stmin:
        return stp, brackt, 0
    sgnd = dp * (dx / abs(dx))
    if fp > fx:
        info, bound = 1, True
        theta = 3 * (fx - fp) / (stp - stx) + dx + dp
        gamma = _cubic_gamma(theta, dx, dp, False)
        if stp < stx:
            gamma = -gamma
        p = gamma - dx + theta
        q = gamma - dx + gamma + dp
        r = p / q
        stpc = stx + r * (stp - stx)
        stpq = stx + dx / ((fx - fp) / (stp - stx) + dx) / 2 * (stp - stx)
        stpf = stpc if abs(stpc - stx) < abs(stpq - stx) else stpc + (stpq - stpc) / 2
        brackt = True
    elif sgnd < 0:
        info, bound = 2, False
        theta = 3 * (fx - fp) / (stp - stx) + dx + dp
        gamma = _cubic_gamma(theta, dx, dp, False)
        if stp > stx:
            gamma = -gamma
        p = gamma - dp + theta
        q = gamma - dp + gamma + dx
        r = p / q
        stpc = stp + r * (stx - stp)
        stpq = stp + dp / (dp - dx) * (stx - stp)
        stpf = stpc if abs(stpc - stp) > abs(stpq - stp) else stpq
        brackt = True
    elif abs(dp) < abs(dx):
        info, bound = 3, True
        theta = 3 * (fx - fp) / (stp - stx) + dx + dp
        gamma = _cubic_gamma(theta, dx, dp, True)
        if stp > stx:
            gamma = -gamma
        p = gamma - dp + theta
        q = gamma + (dx - dp) + gamma
        r = p / q
        if r < 0 and gamma != 0:
            stpc = stp + r * (stx - stp)
        else:
            stpc = stmax if stp > stx else stmin
        stpq = stp + dp / (dp - dx) * (stx - stp)
        if brackt:
            stpf = stpc if abs(stp - stpc) < abs(stp - stpq) else stpq
        else:
            stpf = stpc if abs(stp - stpc) > abs(stp - stpq) else stpq
    else:
        info, bound = 4, False
        if brackt:
            theta = 3 * (fp - fy) / (sty - stp) + dy + dp
            gamma = _cubic_gamma(theta, dy, dp, False)
            if stp > sty:
                gamma = -gamma
            p = gamma - dp + theta
            q = gamma - dp + gamma + dy
            r = p / q
            stpf = stp + r * (sty - stp)
        else:
            stpf = stmax if stp > stx else stmin
    if fp > fx:
        sty, fy, dy = stp, fp, dp
    else:
        if sgnd < 0.0:
            sty, fy, dy = stx, fx, dx
        stx, fx, dx = stp, fp, dp
    stpf = min(stmax, stpf)
    stpf = max(stmin, stpf)
    stp = stpf
    if brackt and bound:
        if sty > stx:
            stp = min(stx + 0.66 * (sty - stx), stp)
        else:
            stp = max(stx + 0.66 * (sty - stx), stp)
    b[:] = [stx, fx, dx, sty, fy, dy]
    return stp, brackt, info


def mcsrch(fun, x, f, g, d, stp, gtol, trim, trace, nfev=0, store=None, dginit_dot=dot):
    """mcsrch with the evaluation inlined and trimfunction after each evaluation.  x, g are updated in place; returns
    (f, stp, info, nfev).  nfev is reset only once the search starts: the early returns (stp <= 0, not a descent
    direction) hand back the caller's previous count, as ALGLIB's state->nfev."""
    info = 0
    if stp < STPMIN:
        stp = STPMIN
    if stp > STPMAX:
        stp = STPMAX
    if stp <= 0:
        return f, stp, info, nfev
    dginit = dginit_dot(g, d)
    if dginit >= 0:
        return f, stp, info, nfev
    nfev = 0
    infoc = 1
    brackt, stage1 = False, True
    finit = f
    dgtest = FTOL * dginit
    width = STPMAX - STPMIN
    width1 = width / 0.5
    wa = x.copy()
    b = [0.0, finit, dginit, 0.0, finit, dginit]
    while True:
        if brackt:
            stmin, stmax = (b[0], b[3]) if b[0] < b[3] else (b[3], b[0])
        else:
            stmin = b[0]
            stmax = stp + 4.0 * (stp - b[0])
        if stp > STPMAX:
            stp = STPMAX
        if stp < STPMIN:
            stp = STPMIN
        if (brackt and (stp <= stmin or stp >= stmax)) or nfev >= MAXFEV - 1 or infoc == 0 or \
                (brackt and stmax - stmin <= XTOL * stmax):
            stp = b[0]
        if store is None:
            x[:] = wa + stp * d
        else:  # the device's trial point: xk + (T)stp * d in T (one rounding: the FMA of k_axpy_out / the fold)
            x[:] = (wa + float(store(stp)) * d).astype(store)
        f, gn = fun(x.copy())
        f = float(f)
        g[:] = gn if store is None else np.asarray(gn).astype(store)
        if trace is not None:
            trace.append(f)
        if f >= trim:  # trimfunction
            f = trim
            g[:] = 0.0
        info = 0
        nfev += 1
        dg = dot(g, d)
        ftest1 = finit + stp * dgtest
        if (brackt and (stp <= stmin or stp >= stmax)) or infoc == 0:
            info = 6
        if stp == STPMAX and f < finit and f <= ftest1 and dg <= dgtest:
            info = 5
        if stp == STPMIN and (f >= finit or f > ftest1 or dg >= dgtest):
            info = 4
        if nfev >= MAXFEV:
            info = 3
        if brackt and stmax - stmin <= XTOL * stmax:
            info = 2
        if f < finit and f <= ftest1 and abs(dg) <= -gtol * dginit:
            info = 1
        if info != 0:
            if info in (1, 5):
                v = seqsum((wa - x) * (wa - x))
                if f >= finit or v == 0.0:
                    info = 6
            return f, stp, info, nfev
        if stage1 and f <= ftest1 and dg >= min(FTOL, gtol) * dginit:
            stage1 = False
        if stage1 and f <= b[1] and f > ftest1:
            fm = f - stp * dgtest
            m = [b[0], b[1] - b[0] * dgtest, b[2] - dgtest, b[3], b[4] - b[3] * dgtest, b[5] - dgtest]
            stp, brackt, infoc = mcstep(m, stp, fm, dg - dgtest, brackt, stmin, stmax)
            b = [m[0], m[1] + m[0] * dgtest, m[2] + dgtest, m[3], m[4] + m[3] * dgtest, m[5] + dgtest]
        else:
            stp, brackt, infoc = mcstep(b, stp, f, dg, brackt, stmin, stmax)
        if brackt:
            if abs(b[3] - b[0]) >= 0.66 * width1:
                stp = b[0] + 0.5 * (b[3] - b[0])
            width1 = width
            width = abs(b[3] - b[0])


def linminnormalized(d, stp, store=None, maxsum=False, dot_=dot, keep=None):
    a = np.abs(d[:keep])
    mx = (float(np.sum(a)) if maxsum else float(np.max(a))) if a.size else 0.0
    if mx == 0:
        return stp
    s = 1 / mx
    d *= s
    stp = stp / s
    s = dot_(d, d)
    s = 1 / math.sqrt(s)
    d *= s
    if store is not None:  # the normalised direction as the device forms it: (T)((dn s1) s2)
        d[:] = d.astype(store)
    return stp / s


class Report:
    def __init__(self):
        self.termination_type = 0
        self.iterations = 0
        self.nfev = 0
        self.f = 0.0
        self.updates = 0  # successful iterations (k): history pairs the direction was formed from, counting overwritten ones


def _gram_direction(g, sk, yk, rho, k, q, m, swap):
    """-work by run_lbfgs's host loops (ALGLIB's two loops on the coefficients over {g, s_j, y_j}, each dot product from
    the Gram table), the table's s_a.y_b entries transposed when swap."""
    SY = np.array([[dot(sk[a], yk[b]) for b in range(m)] for a in range(m)])
    YY = np.array([[dot(yk[a], yk[b]) for b in range(m)] for a in range(m)])
    if swap:
        SY = SY.T.copy()
    gs = [dot(g, sk[j]) for j in range(m)]
    gy = [dot(g, yk[j]) for j in range(m)]
    live = q + 1
    p = k % m
    gammak = SY[p, p] / YY[p, p]
    cgc, cs, cy, theta = 1.0, np.zeros(m), np.zeros(m), np.zeros(m)
    for i in range(k, k - q - 1, -1):
        ic = i % m
        t = cgc * gs[ic]
        for j in range(live):
            t += cy[j] * SY[ic, j]
        theta[ic] = t
        cy[ic] -= t * rho[ic]
    cgc *= gammak
    cy[:live] *= gammak
    for i in range(k - q, k + 1):
        ic = i % m
        t = cgc * gy[ic]
        for j in range(live):
            t += cs[j] * SY[j, ic] + cy[j] * YY[ic, j]
        cs[ic] += rho[ic] * (-t + theta[ic])
    w = cgc * g
    for j in range(live):
        w = w + cs[j] * sk[j] + cy[j] * yk[j]
    return -w


def minlbfgs(fun, x0, m, epsg, epsf, epsx, maxits, trace=None, xrep=None, store=None, plant=None):
    """Minimise fun(x) -> (f, g).  trace: f of every evaluation, in order; xrep: (x, f) of every point ALGLIB reports
    (the start point, then the accepted point of every iteration).  store, plant: the hooks of the module docstring
    (default off).  Returns (x, Report)."""
    assert m >= 1
    if epsg == 0 and epsf == 0 and epsx == 0 and maxits == 0:
        epsx = 1.0e-6
    kind, arg = plant if plant is not None else (None, None)
    x = np.array(x0, dtype=np.float64).ravel().copy()
    n = x.size
    if kind == "lose":
        def pdot(a, b):
            return dot(a[:arg], b[:arg])

        def psq(v):
            return seqsum(v[:arg] * v[:arg])
    else:
        pdot = dot

        def psq(v):
            return seqsum(v * v)
    if store is not None:
        x = x.astype(store).astype(np.float64)
    rep = Report()
    f, g = fun(x.copy())
    f = float(f)
    g = np.array(g, dtype=np.float64).ravel().copy()
    if store is not None:
        g = g.astype(store).astype(np.float64)
    if trace is not None:
        trace.append(f)
    trim = 10 * (abs(f) + 1)  # trimprepare
    if xrep is not None:
        xrep.append((x.copy(), f))
    rep.nfev = 1
    fold = f
    if math.sqrt(seqsum(g * g)) <= epsg:
        rep.termination_type = 4
        rep.f = f
        return x, rep
    d = -g
    stp = min(1.0 / math.sqrt(pdot(g, g)), 1.0)
    sk = np.zeros((m, n))
    yk = np.zeros((m, n))
    rho = np.zeros(m)
    theta = np.zeros(m)
    nfev = 0
    k = 0
    while True:
        p = k % m
        q = min(k, m - 1)
        sk[p] = -x
        yk[p] = -g
        if k != 0:
            stp = 1.0
        stp = linminnormalized(d, stp, store, kind == "maxsum", pdot, arg if kind == "lose" else None)
        f, stp, mcinfo, nfev = mcsrch(fun, x, f, g, d, stp, GTOL, trim, trace, nfev, store, pdot)
        if xrep is not None:
            xrep.append((x.copy(), f))
        rep.nfev += nfev
        rep.iterations += 1
        sk[p] += x
        yk[p] += g
        if store is not None:  # s = -x_k + x, y = -g_k + g in T
            sk[p] = sk[p].astype(store)
            yk[p] = yk[p].astype(store)
        if kind == "lose":
            sk[p][arg:] = 0.0
            yk[p][arg:] = 0.0
        v = psq(g)
        if not math.isfinite(v) or not math.isfinite(f):
            rep.termination_type = -8
            break
        if rep.iterations >= maxits and maxits > 0:
            rep.termination_type = 5
            break
        if math.sqrt(v) <= epsg:
            rep.termination_type = 4
            break
        if fold - f <= epsf * max(abs(fold), max(abs(f), 1.0)):
            rep.termination_type = 1
            break
        if math.sqrt(psq(sk[p])) <= epsx:
            rep.termination_type = 2
            break
        if mcinfo != 1:
            fold = f
            d = -g
        else:
            v = pdot(yk[p], sk[p])
            vv = pdot(yk[p], yk[p])
            if v == 0 or vv == 0:
                rep.termination_type = -2
                break
            rho[p] = 1 / v
            gammak = v / vv
            if kind == "swap":
                d = _gram_direction(g, sk, yk, rho, k, q, m, True)
            else:
                qq = q - 1 if (kind == "drop_oldest" and k >= m and m >= 2) else q
                work = g.copy()
                for i in range(k, k - qq - 1, -1):
                    ic = i % m
                    v = pdot(sk[ic], work)
                    theta[ic] = v
                    vv = v * rho[ic]
                    work += (-vv) * yk[ic]   # ae_v_subd = ae_v_addd with -alpha
                work *= gammak
                for i in range(k - qq, k + 1):
                    ic = i % m
                    v = pdot(yk[ic], work)
                    vv = rho[ic] * (-v + theta[ic])
                    work += vv * sk[ic]
                d = -work
            if store is not None:  # dn in T
                d = d.astype(store).astype(np.float64)
            fold = f
            k += 1
            rep.updates = k
    rep.f = f
    return x, rep


def irls_adapter(m=5, log=None):
    """A function with sro_cg_fn's signature (oracle/srmap_oracle.h) running minlbfgs with m pairs: pass it to
    ``sro_irls_solve`` (the returned object must stay alive while the solve runs).  log, when given, receives one
    Report per inner run."""
    import oracle as orc

    def _run(n, px, epsg, epsf, epsx, maxits, fg, rp, ctx, report):
        x0 = np.ctypeslib.as_array(px, shape=(n,)).copy()
        buf_x = np.empty(n)
        buf_g = np.empty(n)

        def fun(v):
            buf_x[:] = v
            f = fg(ctx, buf_x.ctypes.data_as(orc.c_double_p), buf_g.ctypes.data_as(orc.c_double_p))
            return f, buf_g.copy()

        x, rep = minlbfgs(fun, x0, m, epsg, epsf, epsx, maxits)
        np.ctypeslib.as_array(px, shape=(n,))[:] = x
        report.contents.termination_type = rep.termination_type
        report.contents.iterations = rep.iterations
        report.contents.nfev = rep.nfev
        report.contents.f = rep.f
        if log is not None:
            log.append(rep)

    return orc.CG_FN(_run)


def oracle_solve(problem, x0, m=5, options=None):
    """The oracle's IRLS solve (sro_irls_solve) with L-BFGS(m) as the inner solver: (x, SolveReport)."""
    import oracle as orc
    a = np.ascontiguousarray(x0, dtype=np.float64)
    out = np.empty_like(a)
    o = orc.default_irls_options() if options is None else options
    rep = orc.SolveReport()
    fn = irls_adapter(m)
    orc.lib().sro_irls_solve(problem._p, C.byref(o), a.ctypes.data_as(orc.c_double_p), out.ctypes.data_as(orc.c_double_p),
                             C.cast(fn, C.c_void_p), C.byref(rep))
    return out, rep
