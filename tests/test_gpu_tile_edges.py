"""Tile-path parity matrix: every instance of the fused tile kernel k_eval_z (csrc/kernels_ztile.hip, csrc/ztile_dev.hpp)
at ragged right / bottom edges, large integer shifts, the tile plan's size and frame-table limits, sub-pixel edges and
every cost-reduction variant, against the f64 oracle with the term-scaled bars of tests/error_bars.py; and the g.d of the
integer-shift tile launch (the WD instance) against the direct kernels' separate reduction through a CG trace.

Inputs are dyadic (error_bars.dyadic_inputs): f32 casts are exact, so kernel and oracle differ by rounding alone.
"""
import numpy as np
import pytest

import oracle as orc
import error_bars as eb
import tile_matrix as tm
from parity_log import note

pytestmark = pytest.mark.gpu

DT = {"f64": 0, "f32": 1}


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


def _setup(sr, ctx, W, H, C, S, B, shifts, regs, dtype, seed, M_too=True):
    """GPU problem, oracle problem, x, and the term magnitudes; regs: [(kind, lam, R, decay)]."""
    rng = np.random.default_rng(seed)
    K = len(shifts)
    x, lr = eb.dyadic_inputs(rng, K, C, H, W, S)
    sigma = 1.0 if B > 1 else 0.0
    model = orc.ImageModel(scale=S, shifts=shifts, blur_ksize=B if B > 1 else 0, blur_sigma=sigma)
    p = sr.Problem(ctx, W, H, C, K, S, shifts, B if B > 1 else 0, sigma, dtype)
    p.set_observations(lr)
    ref = orc.Problem(model, lr)
    wregs = []
    for kind, lam, R, dc in regs:
        w = eb.dyadic_weights(rng, C, H, W)
        i = p.add_regularizer(kind, lam, R, dc)
        j = ref.add_regularizer(kind, lam, R, dc)
        p.set_irls_weights(i, w)
        ref.set_irls_weights(j, w)
        wregs.append((kind, lam, R, dc, w))
    if not M_too:
        return p, ref, x, None, None
    Mf, M = eb.term_magnitude(model, lr, x, wregs)
    E = int(np.ceil(max(max(abs(a), abs(b)) for a, b in shifts)))
    return p, ref, x, Mf, eb.with_ring(M, E, S, (B - 1) // 2)


def _check(sr, p, ref, x, Mf, M, dtype, ref_fg=None):
    """Cost and gradient of the problem's current implementation against the oracle, within the term-scaled bars."""
    f, g = p.eval(x)
    f_ref, g_ref = ref_fg if ref_fg is not None else ref.objective(x)
    rg = eb.check_gradient(g, g_ref.reshape(g.shape), M, dtype)
    rf = eb.check_cost(f, f_ref, Mf, dtype)
    assert rg <= eb.C_BAR[dtype], rg
    assert rf <= eb.C_COST[dtype], rf
    # a cost-only call through the same plan
    fc, _ = p.eval(x, sr.TERM_ALL, want_grad=False)
    assert abs(fc - f) <= 1e-12 * max(1.0, abs(f))


def _tiled(sr, p):
    p.set_impl(sr.IMPL_TILED)
    assert p.active_impl() == sr.IMPL_TILED


def _falls_back(sr, p, x):
    """The plan rejected the geometry: IMPL_TILED refuses it, AUTO runs the direct kernels."""
    p.set_impl(sr.IMPL_TILED)
    with pytest.raises(sr.SrmapError) as e:
        p.eval(x)
    assert e.value.status == sr.EUNSUPPORTED
    p.set_impl(sr.IMPL_AUTO)
    assert p.active_impl() == sr.IMPL_DIRECT


# ---------------------------------------------------------------- instances x edges
MATRIX = tm.matrix()


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("case", range(len(MATRIX)), ids=[tm.geo_id(*c) for c in MATRIX])
def test_instance_at_edges(sr, ctx, case, dt):
    """Every (dtype, S, B, regulariser leg) instance on the covering geometries of tests/tile_matrix.py.  B = 1 and
    E = 0 geometries reduce the cost inside the tile kernel (mfin: no ring pixel needs a correction); B = 3 with positive
    shifts has ring corrections (rg[0], rg[1] > 0), so k_finish_eval applies them and reduces."""
    S, B, leg, gi, (W, H, C, shifts, decay) = MATRIX[case]
    dtype = DT[dt]
    p, ref, x, Mf, M = _setup(sr, ctx, W, H, C, S, B, shifts, tm.regs_of(leg, decay), dtype, 8000 + case)
    _tiled(sr, p)
    _check(sr, p, ref, x, Mf, M, dtype)


# ---------------------------------------------------------------- plan thresholds
def _mult_below(v, S):
    return (v // S) * S


def _mult_above(v, S):
    return (v // S + 1) * S


@pytest.mark.parametrize("axis", ["W", "H"])
@pytest.mark.parametrize("S", tm.SCALES)
def test_integer_plan_threshold(sr, ctx, S, axis):
    """The integer plan needs W, H > 4E + 2S (the border frame of width 2E stays a small part of the image).  HR sizes are
    multiples of S, so the pair is the last multiple of S at or below 4E + 2S (falls back: IMPL_TILED refuses, AUTO
    matches the oracle on the direct kernels) and the first above it (plans tiled and matches)."""
    E = 5
    shifts = [[0, 0], [E, -2], [-1, E], [-E, 1], [2, -E]] + [[a, b] for a in range(S) for b in range(S)]
    t = 4 * E + 2 * S
    big = _mult_above(t + 40, S)
    for n, tiled in ((_mult_below(t, S), False), (_mult_above(t, S), True)):
        W, H = (n, big) if axis == "W" else (big, n)
        p, ref, x, Mf, M = _setup(sr, ctx, W, H, 1, S, 3, shifts, [(2, eb.LAMBDA, 3, 0.5)], 0, 8500 + n)
        if tiled:
            _tiled(sr, p)
        else:
            _falls_back(sr, p, x)
        _check(sr, p, ref, x, Mf, M, 0)


def _warp_offsets(d):
    """cv::warpAffine's integer source offset of a shift d (csrc/model_tables.hpp warp_tables: 1/32-px fixed point)."""
    x0 = (int(np.rint(-d * 1024)) + 16) >> 5
    return x0 >> 5


def _sp_reach(shifts, B):
    """Dr = amax + 2 + hb of the sub-pixel plan: amax over the forward and backward warps' integer offsets."""
    amax = 0
    for dx, dy in shifts:
        for s in (1, -1):
            amax = max(amax, abs(_warp_offsets(s * dx)), abs(_warp_offsets(s * dy)))
    return amax + 2 + (B - 1) // 2


@pytest.mark.parametrize("axis", ["W", "H"])
@pytest.mark.parametrize("S", tm.SCALES)
def test_subpixel_plan_threshold(sr, ctx, S, axis):
    """The sub-pixel plan needs W, H > 4 Dr + 2S, Dr = amax + 2 + hb: the multiples of S on either side."""
    B = 3
    shifts = [[0.5, 0.25], [-3.25, 1.75], [2.0, -3.5], [0, 0]]
    t = 4 * _sp_reach(shifts, B) + 2 * S
    big = _mult_above(t + 40, S)
    for n, tiled in ((_mult_below(t, S), False), (_mult_above(t, S), True)):
        W, H = (n, big) if axis == "W" else (big, n)
        p, ref, x, Mf, M = _setup(sr, ctx, W, H, 1, S, B, shifts, [(0, eb.LAMBDA, 0, 0.0)], 0, 8600 + n)
        if tiled:
            _tiled(sr, p)
        else:
            _falls_back(sr, p, x)
        _check(sr, p, ref, x, Mf, M, 0)


# ---------------------------------------------------------------- large integer shifts
@pytest.mark.parametrize("S,E", [(3, 33), (2, 150), (4, 300)])
def test_large_integer_shifts(sr, ctx, S, E):
    """Borders wider than a tile (150 > 128 px at S = 2, 300 > 256 px at S = 4): k_border and the ring corrections over
    a frame of width 2E, mixed signs, one frame at (0, 0), every phase.  Both dtypes against one oracle evaluation."""
    shifts = [[0, 0], [E, -E], [-E, E - 1], [E - 2, 3], [-7, -E]] + [[a - S // 2, b - S // 2] for a in range(S) for b in range(S)]
    W = _mult_above(4 * E + 2 * S, S) + 2 * S
    H = _mult_above(4 * E + 2 * S, S) + 3 * S
    ref_fg = None
    for dtype in (0, 1):
        p, ref, x, Mf, M = _setup(sr, ctx, W, H, 1, S, 3, shifts, [(2, eb.LAMBDA, 3, 0.625)], dtype, 8700 + E, M_too=ref_fg is None)
        if ref_fg is None:
            ref_fg = ref.objective(x) + (Mf, M)
        _tiled(sr, p)
        _check(sr, p, ref, x, *ref_fg[2:], dtype, ref_fg=ref_fg[:2])


# ---------------------------------------------------------------- frame-table limit
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [256, 257])
def test_frame_table_limit(sr, ctx, K, B):
    """k_border stages the frame table (one entry per frame) in LDS, kBorderTabEntries = 256: K = 256 plans tiled,
    K = 257 falls back; both match the oracle."""
    S = 2
    rng = np.random.default_rng(K)
    shifts = [[int(a), int(b)] for a, b in rng.integers(-1, 2, size=(K, 2))]
    W, H = 34, 22
    p, ref, x, Mf, M = _setup(sr, ctx, W, H, 1, S, B, shifts, [(2, eb.LAMBDA, 2, 0.5)], 0, 8800 + K + B)
    if K <= 256:
        _tiled(sr, p)
    else:
        _falls_back(sr, p, x)
    _check(sr, p, ref, x, Mf, M, 0)


# ---------------------------------------------------------------- sub-pixel edges
SP_FRACS = [1 / 64, 63 / 64, -1 / 64, 3 - 2.0 ** -20]


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("leg", ["btv3", "tv"])
@pytest.mark.parametrize("B", tm.BLURS)
@pytest.mark.parametrize("S", tm.SCALES)
def test_subpixel_edges(sr, ctx, S, B, leg, dt):
    """Fractions at the 1/32-px quantisation edges (1/64 is a rounding tie that is exact in double: forward and backward
    warps quantise it differently), shifts up to 40 px, sizes just above 4 Dr + 2S with ragged tiles."""
    dtype = DT[dt]
    f = SP_FRACS
    shifts = [[0, 0], [40 - f[0], -37 + f[1]], [-40 + f[1], 12 + f[2]], [f[3], -f[0]], [-21 + f[2], 40 - f[1]],
              [f[1], f[3] - 5]]
    t = 4 * _sp_reach(shifts, B) + 2 * S
    W, H = _mult_above(t, S) + S, _mult_above(t, S)
    p, ref, x, Mf, M = _setup(sr, ctx, W, H, 1, S, B, shifts, tm.regs_of(leg, 0.5), dtype, 8900 + 10 * S + B)
    _tiled(sr, p)
    _check(sr, p, ref, x, Mf, M, dtype)


def test_rounding_tie_shift_stays_direct(sr, ctx):
    """A dy within floating-point rounding of a 1/32-px tie gives a per-row table: the plan leaves it to the direct
    kernels, which still match the oracle."""
    S = 2
    shifts = [[0.25, -0.0151367187499999], [-1.5, 0.0161132812500001], [0.0, 0.0]]
    p, ref, x, Mf, M = _setup(sr, ctx, 96, 96, 1, S, 3, shifts, [(0, eb.LAMBDA, 0, 0.0)], 0, 8990)
    _falls_back(sr, p, x)
    _check(sr, p, ref, x, Mf, M, 0)


# ---------------------------------------------------------------- reduction variants
@pytest.mark.parametrize("dt", list(DT))
def test_two_stage_reduction_by_the_caller(sr, ctx, dt):
    """More than kMaxFusedPartials = 65536 cost partials (one per tile and channel): 33 channels of 2048 one-column-tile
    x 8-row tiles = 67584, so neither the in-kernel finish nor k_finish_eval reduces; the caller's two-stage reduction
    does.  Not observable through the Python surface: this geometry is the only one of the file that reaches it."""
    dtype = DT[dt]
    S, W, H, C = 2, 6, 16384, 33
    assert ((W // S + 63) // 64) * ((H + 7) // 8) * C > 65536
    p, ref, x, Mf, M = _setup(sr, ctx, W, H, C, S, 1, [[0, 0]], [(0, eb.LAMBDA, 0, 0.0)], dtype, 8995)
    _tiled(sr, p)
    _check(sr, p, ref, x, Mf, M, dtype)


# ---------------------------------------------------------------- g.d of the integer tile launch
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("leg", list(tm.LEGS))
@pytest.mark.parametrize("B", tm.BLURS)
@pytest.mark.parametrize("S", tm.SCALES)
def test_integer_cg_on_tiles_follows_direct_kernels(sr, ctx, S, B, leg, dt):
    """g.d out of the integer-shift tile launch (the WD instance, partial edge tiles included) against the direct kernels,
    where g.d comes from a separate reduction: a 4-iteration CG run follows evaluation for evaluation."""
    dtype = DT[dt]
    W, H, C, shifts, decay = tm.geometries(S, leg)[1]
    rng = np.random.default_rng(9100 + 10 * S + B)
    x0, lr = eb.dyadic_inputs(rng, len(shifts), C, H, W, S)
    wts = eb.dyadic_weights(rng, C, H, W)
    res = {}
    for name, impl in (("tiled", sr.IMPL_TILED), ("direct", sr.IMPL_DIRECT)):
        p = sr.Problem(ctx, W, H, C, len(shifts), S, shifts, B if B > 1 else 0, 1.0 if B > 1 else 0.0, dtype)
        p.set_impl(impl)
        p.set_observations(lr)
        for kind, lam, R, dc in tm.regs_of(leg, decay):
            p.set_irls_weights(p.add_regularizer(kind, lam, R, dc), wts)
        x, its, nfev, term, trace = p.cg_trace(x0, 0.0, 0.0, 0.0, 4)
        res[name] = (x, its, nfev, term, np.asarray(trace))
    (x1, i1, n1, t1, tr1), (x2, i2, n2, t2, tr2) = res["tiled"], res["direct"]
    assert (i1, n1, t1) == (i2, n2, t2) and len(tr1) == len(tr2)
    e_tr = note(np.max(np.abs(tr1 - tr2) / np.maximum(1.0, np.abs(tr2))), "trace")
    e_x = note(np.max(np.abs(x1 - x2)), "x")
    # f64: the bars of test_subpixel_cg_on_tiles_follows_direct_kernels; f32: the f32 cost bar of the parity tests (1e-5)
    # on the trace and the f32 operator bar (2e-5) on the iterate
    assert e_tr <= (1e-11 if dtype == 0 else 1e-5)
    assert e_x <= (1e-9 if dtype == 0 else 2e-5)
