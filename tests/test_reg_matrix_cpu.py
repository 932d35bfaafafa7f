"""The direct regulariser matrix (tests/reg_matrix.py) and its bars (tests/error_bars.py) without a GPU: the dispatch
mirror reaches every kernel variant at every edge the matrix is meant to cover, the magnitudes bound every oracle term,
and plausible kernel bugs, planted into a numpy restatement of the kernels, exceed the f32 bars on the geometries meant
to catch them."""
import numpy as np
import pytest

import oracle as orc
import error_bars as eb
import reg_matrix as rm

LAM = eb.LAMBDA
F32 = eb.F32


def _x(rng, C, H, W):
    return rng.integers(0, 65, size=(C, H, W)) / 64.0


# ---------------------------------------------------------------- the mirror reaches every cell
def test_mirror_matches_the_launchers_on_known_cases():
    assert rm.values_kernel(rm.BTV, 3, 1, 16, 4) == "strip"
    assert rm.values_kernel(rm.BTV, 3, 1, 15, 4) == "values4_R3"
    assert rm.values_kernel(rm.BTV, 3, 1, 16, 5) == "reg_values"
    assert rm.values_kernel(rm.BTV, 4, 1, 16, 8) == "reg_values"
    assert rm.values_kernel(rm.TV, 0, 1, 16, 8) == "reg_values"
    assert [rm.march_chunk(C, 5, 4) for C in (2, 16, 17, 33, 40, 50)] == [2, 16, 9, 9, 10, 13]
    assert rm.march_chunk(20, 16384, 4) == 20 and rm.march_chunk(20, 16380, 4) == 10
    assert rm.grad_kernel(rm.TV3D, 1, 8, 8, False) == "onepass3d"
    assert rm.grad_kernel(rm.TV3D, 2, 8, 9, False) == "onepass3d"
    assert rm.grad_kernel(rm.TV3D, 2, 8, 8, True) == "reg_gradient_direct"
    assert rm.onepass_paths(2, 8) == {"masked"} and rm.onepass_paths(3, 8) == {"fast", "masked"}


def test_values_cells_cover_every_kernel_and_edge():
    by = {}
    for cell in rm.VALUE_CELLS:
        kind, R, dc, C, H, W = cell
        by.setdefault(rm.values_kernel(kind, R, C, H, W), []).append(cell)
    assert set(by) == {"strip", "values4_R1", "values4_R2", "values4_R3", "reg_values"}
    strip = by["strip"]
    assert {H for *_, H, W in strip} >= {16, 17, 18, 19}
    assert {H % 4 for *_, H, W in strip if H > 19} == {0, 1, 2, 3}
    assert {W // 4 for *_, W in strip} == {1, 3, 16, 63, 64, 65}
    assert {c[2] for c in strip} == {0.5, 1.0} and any(c[3] > 1 for c in strip)
    for R in (1, 2):
        hs = {c[4] for c in by["values4_R%d" % R]}
        assert min(hs) < 16 <= max(hs)
    assert 15 in {c[4] for c in by["values4_R3"]}
    rv = by["reg_values"]
    assert {W % 4 for k, R, d, C, H, W in rv if k == rm.BTV and R <= 3} == {1, 2, 3}
    assert any(k == rm.BTV and R == 4 for k, R, *_ in rv)
    assert {rm.TV, rm.TV3D} <= {c[0] for c in rv}


def test_gradient_cells_cover_every_kernel_and_edge():
    by = {}
    for cell in rm.GRAD_CELLS:
        kind, R, dc, C, H, W = cell
        by.setdefault(rm.grad_kernel(kind, C, H, W, False), []).append(cell)
    assert set(by) == {"march", "onepass2d", "onepass3d", "reg_gradient_direct"}
    march = by["march"]
    lengths = [[n for _, n in rm.march_chunks(C, H, W)] for *_, C, H, W in march]
    assert {rm.march_chunk(C, H, W) % 3 for *_, C, H, W in march} == {0, 1, 2}  # the chunk length
    assert {ls[-1] % 3 for ls in lengths} == {0, 1, 2}                   # last chunks
    assert any(len(ls) == 1 and ls[0] > 16 for ls in lengths)            # no halving above 16 channels
    assert {C for *_, C, H, W in march if rm.cdiv(W, 256) * rm.cdiv(H, 4) <= 6} >= {2, 3, 4, 17, 40, 50}  # small planes
    assert {H % 4 for *_, H, W in march} == {0, 1, 2, 3}
    assert {W for *_, W in march} == {4, 252, 256, 260}
    for k in ("onepass2d", "onepass3d"):
        cells = by[k]
        paths = set().union(*(rm.onepass_paths(H, W) for *_, H, W in cells))
        assert paths == {"fast", "masked"}
        assert any(W % 4 for *_, W in cells)
    assert all(C == 1 for *_, C, H, W in by["onepass3d"] if W % 4 == 0)
    op = by["onepass2d"] + by["onepass3d"]
    assert {H for *_, H, W in op} >= {1, 2, 3, 4, 5}
    assert {W for *_, W in op} >= {1, 255, 257}
    btv = by["reg_gradient_direct"]
    assert {R for _, R, *_ in btv} == {1, 2, 3, 4}
    assert {W % 4 for *_, W in btv} >= {1, 3} and {H % 4 for *_, H, W in btv} >= {1, 2, 3}


# ---------------------------------------------------------------- the magnitudes bound the oracle
ALL_CELLS = rm.VALUE_CELLS + rm.GRAD_CELLS


@pytest.mark.parametrize("cell", ALL_CELLS, ids=[rm.cell_id(c) for c in ALL_CELLS])
def test_magnitudes_bound_every_oracle_term(cell):
    kind, R, dc, C, H, W = cell
    rng = np.random.default_rng(C * 11 + H * 5 + W)
    x = _x(rng, C, H, W) - 0.5  # both signs
    w = eb.dyadic_weights(rng, C, H, W)
    v, g = orc.reg_values_and_gradient(kind, x, LAM * w, R, dc)
    Mv = eb.value_magnitude(kind, x, R, dc)
    Mf, M = eb.reg_magnitude(kind, x, w, LAM, R, dc)
    f = LAM * float(np.sum(w * v * v))
    assert np.all(v <= Mv * (1 + 1e-12))
    assert np.all(np.abs(g) <= M * (1 + 1e-12))
    assert f <= Mf * (1 + 1e-12)
    # and each bound is attained somewhere up to a small factor (it is not vacuous)
    assert np.max(Mv) <= 8 * max(np.max(v), 1e-300) and np.max(M) <= 8 * max(np.max(np.abs(g)), 1e-300)


# ---------------------------------------------------------------- a numpy restatement with planted bugs
def _sgn(a):
    return np.sign(a)


def btv_values_np(x, R, dc, bug=None):
    """k_btv_values4 / k_btv_values_strip per pixel: taps (i, j) in 0..R, the out-of-image ones skipped.
    bug: 'tail'  the last partial strip of 4 rows not written (left at 0);
         'nin'   a row-final cell reads its own cell as the next one (taps past the row's end wrap back by 4 columns);
         'pow'   the decay power off by one."""
    C, H, W = x.shape
    v = np.zeros_like(x)
    for i in range(R + 1):
        for j in range(R + 1):
            a = dc ** (i + j + (1 if bug == "pow" else 0))
            for col in range(W):
                cc = col + j
                if cc >= W:
                    if bug != "nin":
                        continue
                    cc -= 4
                v[:, :H - i, col] += a * np.abs(x[:, :H - i, col] - x[:, i:, cc])
    if bug == "tail":
        v[:, 4 * (H // 4):] = 0.0
    return v


def tv_values_np(x, kind):
    v = np.zeros_like(x)
    v[:, :-1, :] += np.abs(x[:, 1:, :] - x[:, :-1, :])
    v[:, :, :-1] += np.abs(x[:, :, 1:] - x[:, :, :-1])
    if kind == rm.TV3D:
        v[:-1] += np.abs(x[1:] - x[:-1])
    return v


def tv_gradient_np(x, cw, kind, bug=None, chunks=()):
    """k_tv_onepass / k_tv3d_march: 2 c r * (own differences) + the left, upper and (3-D) previous-channel neighbours.
    bug: 'prev_at_chunk'  the march takes the previous plane from the chunk's own first channel at a chunk start;
         'chunk_last'     the march drops each chunk's last plane (its gradient stays at the memset 0);
         'no_prev'        the previous-channel term dropped."""
    r = tv_values_np(x, kind)
    cr = 2.0 * cw * r
    g = np.zeros_like(x)
    g[:, :, :-1] -= cr[:, :, :-1] * _sgn(x[:, :, 1:] - x[:, :, :-1])
    g[:, :-1, :] -= cr[:, :-1, :] * _sgn(x[:, 1:, :] - x[:, :-1, :])
    g[:, :, 1:] += cr[:, :, :-1] * _sgn(x[:, :, 1:] - x[:, :, :-1])
    g[:, 1:, :] += cr[:, :-1, :] * _sgn(x[:, 1:, :] - x[:, :-1, :])
    if kind == rm.TV3D and bug != "no_prev":
        prev = cr[:-1] * _sgn(x[1:] - x[:-1])
        if bug == "prev_at_chunk":
            for c0, _ in chunks:
                if c0 > 0:
                    prev[c0 - 1] = 0.0  # x[c0] - x[c0] = 0: sgn 0
        g[1:] += prev
    if bug == "chunk_last":
        for c0, n in chunks:
            g[c0 + n - 1] = 0.0
    return g


def _beyond_f32(a, ref, M, c):
    """True where some element lies outside the f32 bar c * u * M (NaN and inf count as outside)."""
    a = np.asarray(a, dtype=np.float64)
    ok = np.abs(a - ref) <= c * eb.U[F32] * M
    return not np.all(ok & np.isfinite(a))


BTV4_CELLS = [c for c in rm.VALUE_CELLS if c[0] == rm.BTV and c[5] % 4 == 0 and 1 <= c[1] <= 3]


@pytest.mark.parametrize("cell", BTV4_CELLS, ids=[rm.cell_id(c) for c in BTV4_CELLS])
def test_planted_values_bugs_exceed_the_bar(cell):
    kind, R, dc, C, H, W = cell
    x = _x(np.random.default_rng(H * 17 + W), C, H, W)
    v_ref = orc.reg_values(kind, x, R, dc)
    Mv = eb.value_magnitude(kind, x, R, dc)
    c = eb.C_REG_VAL[F32]
    assert np.max(np.abs(btv_values_np(x, R, dc) - v_ref)) <= 1e-14  # the restatement is the oracle
    assert _beyond_f32(btv_values_np(x, R, dc, "nin"), v_ref, Mv, c)
    if rm.values_kernel(kind, R, C, H, W) == "strip" and H % 4:
        assert _beyond_f32(btv_values_np(x, R, dc, "tail"), v_ref, Mv, c)
    if dc != 1.0:  # 1^(n + 1) = 1^n: an off-by-one power cannot show at decay 1
        assert _beyond_f32(btv_values_np(x, R, dc, "pow"), v_ref, Mv, c)


TV_CELLS = [c for c in rm.GRAD_CELLS if c[0] == rm.TV3D and c[3] >= 2 and c[4] < 1000]


@pytest.mark.parametrize("cell", TV_CELLS, ids=[rm.cell_id(c) for c in TV_CELLS])
def test_planted_tv3d_gradient_bugs_exceed_the_bar(cell):
    kind, R, dc, C, H, W = cell
    rng = np.random.default_rng(C * 7 + H * 3 + W)
    x, w = _x(rng, C, H, W), eb.dyadic_weights(rng, C, H, W)
    _, g_ref = orc.reg_values_and_gradient(kind, x, LAM * w, R, dc)
    _, M = eb.reg_magnitude(kind, x, w, LAM, R, dc)
    c = eb.C_REG_GRAD[F32]
    assert np.max(np.abs(tv_gradient_np(x, LAM * w, kind) - g_ref)) <= 1e-14 * max(1.0, np.max(np.abs(g_ref)))
    assert _beyond_f32(tv_gradient_np(x, LAM * w, kind, "no_prev"), g_ref, M, c)
    if rm.grad_kernel(kind, C, H, W, False) == "march":
        chunks = rm.march_chunks(C, H, W)
        assert _beyond_f32(tv_gradient_np(x, LAM * w, kind, "chunk_last", chunks), g_ref, M, c)
        if len(chunks) > 1:
            assert _beyond_f32(tv_gradient_np(x, LAM * w, kind, "prev_at_chunk", chunks), g_ref, M, c)


def test_march_chunk_bugs_have_cells_to_catch_them():
    multi = [c for c in TV_CELLS if rm.grad_kernel(c[0], c[3], c[4], c[5], False) == "march"
             and len(rm.march_chunks(c[3], c[4], c[5])) > 1]
    assert len(multi) >= 3


@pytest.mark.parametrize("cell", rm.VALUE_CELLS, ids=[rm.cell_id(c) for c in rm.VALUE_CELLS])
def test_planted_clamp_bugs_exceed_the_bar(cell):
    """IRLS weights built at x, the objective evaluated at x' (the only place a wrong clamp shows): the clamp missing
    (1 / r) or applied as min (1 / min(1e-5, r)) exceed the gradient or the cost bar of that evaluation."""
    kind, R, dc, C, H, W = cell
    rng = np.random.default_rng(C * 977 + H * 13 + W)
    xw = rm.weights_input(rng, C, H, W)
    x2 = _x(rng, C, H, W)
    v = orc.reg_values(kind, xw, R, dc)
    assert np.any((v > 0) & (v < 1e-5)) or np.any(v > 1e-5)
    with np.errstate(divide="ignore", invalid="ignore"):
        candidates = {"right": 1.0 / np.maximum(1e-5, v), "missing": 1.0 / v, "min": 1.0 / np.minimum(1e-5, v)}
    out = {}
    for name, w in candidates.items():
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            vals, g = orc.reg_values_and_gradient(kind, x2, LAM * w, R, dc)
            out[name] = (LAM * float(np.sum(w * vals * vals)), g)
    w = candidates["right"]
    Mf, M = eb.reg_magnitude(kind, x2, w, LAM, R, dc)
    extra = eb.weights_rel(kind, R)
    f_ref, g_ref = out["right"]

    def caught(name):
        f, g = out[name]
        return _beyond_f32(g, g_ref, M, eb.C_REG_GRAD[F32] + extra) or \
            _beyond_f32([f], [f_ref], [Mf], eb.C_REG_COST[F32] + extra)

    if np.any(v == 0):
        assert caught("missing")
    assert caught("min")


def test_weights_inputs_reach_the_clamp_on_both_sides():
    """Over the values cells the weights inputs hold flat patches (r = 0) and values just below and above 1e-5."""
    below = above = zero = 0
    for kind, R, dc, C, H, W in rm.VALUE_CELLS:
        rng = np.random.default_rng(C * 977 + H * 13 + W)
        v = orc.reg_values(kind, rm.weights_input(rng, C, H, W), R, dc)
        zero += int(np.any(v == 0))
        below += int(np.any((v > 0) & (v < 1e-5)))
        above += int(np.any((v > 1e-5) & (v < 2e-4)))
    n = len(rm.VALUE_CELLS)
    assert zero >= n - 3 and below >= n // 2 and above >= n - 3, (zero, below, above, n)
