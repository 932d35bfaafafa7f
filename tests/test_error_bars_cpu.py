"""The term-scaled bars of tests/error_bars.py are tight enough to matter: on the geometries of the tile-path matrix
(tests/tile_matrix.py) M bounds every oracle gradient element, and each of five plausible kernel bugs moves at least one
element beyond the f32 bar (the looser of the two).  CPU only: the oracle and numpy restatements stand in for a kernel."""
import numpy as np
import pytest

import oracle as orc
import error_bars as eb
import tile_matrix as tm


def _problem(S, B, leg, geo, seed):
    W, H, C, shifts, decay = geo
    rng = np.random.default_rng(seed)
    x, lr = eb.dyadic_inputs(rng, len(shifts), C, H, W, S)
    regs = [(kind, lam, R, dc, eb.dyadic_weights(rng, C, H, W)) for kind, lam, R, dc in tm.regs_of(leg, decay)]
    model = orc.ImageModel(scale=S, shifts=shifts, blur_ksize=B if B > 1 else 0, blur_sigma=1.0 if B > 1 else 0.0)
    return model, x, lr, regs


def _objective(model, lr, x, regs):
    ref = orc.Problem(model, lr)
    for kind, lam, R, dc, w in regs:
        i = ref.add_regularizer(kind, lam, R, dc)
        ref.set_irls_weights(i, w)
    f, g = ref.objective(x)
    return f, g.reshape(x.shape)


def _data_grad_np(x, lr, S, shifts, k2):
    """2 s^2 sum_k A_k^T (A_k x - y_k), A_k = decimate o correlate(k2) o shift, written out with the oracle's image ops."""
    C, H, W = x.shape
    g = np.zeros_like(x)
    for k, (dx, dy) in enumerate(shifts):
        for c in range(C):
            z = orc.filter2d(orc.warp_shift(x[c], dx, dy), k2)
            r = np.zeros((H, W))
            r[::S, ::S] = z[::S, ::S] - lr[k, c]
            g[c] += 2.0 * S * S * orc.warp_shift(orc.filter2d(r, k2[::-1, ::-1]), -dx, -dy)
    return g


def _caught(g_mut, g_ref, M):
    return not np.all(eb.within_bar(g_mut, g_ref, M, eb.F32))


CASES = tm.matrix()


@pytest.mark.parametrize("case", range(len(CASES)), ids=[tm.geo_id(*c) for c in CASES])
def test_bars_bound_and_bite(case):
    S, B, leg, gi, geo = CASES[case]
    W, H, C, shifts, decay = geo
    model, x, lr, regs = _problem(S, B, leg, geo, 7000 + case)
    f_ref, g_ref = _objective(model, lr, x, regs)
    Mf, M = eb.term_magnitude(model, lr, x, regs)
    # sanity: the bound bounds (up to the rounding of computing it)
    assert np.all(np.abs(g_ref) <= M * (1 + 1e-12)) and abs(f_ref) <= Mf * (1 + 1e-12)
    # the bars the GPU matrix applies: near the edges M takes in the terms the ring corrections cancel
    E = max(max(abs(a), abs(b)) for a, b in shifts)
    M = eb.with_ring(M, E, S, (B - 1) // 2)

    # 1. the last ragged column / row of the gradient taken from the one S pixels before it (an edge-tile index bug; the
    # last column / row that carries terms at all -- without blur or regulariser only phase-0 pixels of E = 0 do)
    c = int(np.nonzero(M.max(axis=(0, 1)))[0][-1])
    r = int(np.nonzero(M.max(axis=(0, 2)))[0][-1])
    g_col = g_ref.copy(); g_col[:, :, c] = g_ref[:, :, c - S]
    g_row = g_ref.copy(); g_row[:, r, :] = g_ref[:, r - S, :]
    assert _caught(g_col, g_ref, M) and _caught(g_row, g_ref, M)

    # 2. one frame's contribution missing
    if len(shifts) > 1:
        k = len(shifts) - 1
        m2 = orc.ImageModel(scale=S, shifts=shifts[:k], blur_ksize=model.blur_ksize, blur_sigma=model.blur_sigma)
        f_m, g_m = _objective(m2, lr[:k], x, regs)
        assert _caught(g_m, g_ref, M)
        assert not eb.within_bar(f_m, f_ref, Mf, eb.F32, eb.C_COST[eb.F32])

    if regs and regs[0][0] == orc.REG_BTV and regs[0][2] >= 2:
        kind, lam, R, dc, w = regs[0]
        # 3. BTV evaluated with R - 1 (one ring of taps lost)
        _, g_m = _objective(model, lr, x, [(kind, lam, R - 1, dc, w)])
        assert _caught(g_m, g_ref, M)
        # 4. the decay off by 2^-10
        _, g_m = _objective(model, lr, x, [(kind, lam, R, dc + 2.0 ** -10, w)])
        assert _caught(g_m, g_ref, M)

    if B == 3:
        # 5. one blur weight replaced by its neighbour's value (the restatement first reproduces the oracle)
        k2 = orc.gaussian_kernel(3, 1.0)[1]
        g_data = _data_grad_np(x, lr, S, shifts, k2)
        fd, gd = orc.Problem(model, lr).data_term(x)
        assert np.max(np.abs(g_data - gd.reshape(x.shape))) <= 1e-12 * max(1.0, np.max(np.abs(g_data)))
        k2m = k2.copy(); k2m[0, 1] = k2[0, 0]
        assert _caught(g_ref - g_data + _data_grad_np(x, lr, S, shifts, k2m), g_ref, M)


def test_bars_catch_one_far_btv_tap():
    """The case the relative f32 bar (2e-5 of max(1, |g|)) cannot see: the farthest gradient tap of BTV R = 3 (decay 1/2,
    IRLS weight 1/16 at that pixel) dropped at ONE pixel: 2 lambda w r alpha^4 sgn ~ 1e-4 r."""
    S, B, leg, gi, geo = [c for c in CASES if c[:3] == (4, 3, "btv3")][1]
    model, x, lr, regs = _problem(S, B, leg, geo, 1)
    kind, lam, R, _, w = regs[0]
    dc = 0.5
    C, H, W = x.shape
    i, j = H // 2, W // 2
    x[0, i, j] = 1.0
    x[0, i + R - 1, j + R - 1] = 0.0
    w[0, i, j] = 1.0 / 16
    regs = [(kind, lam, R, dc, w)]
    _, g_ref = _objective(model, lr, x, regs)
    _, M = eb.term_magnitude(model, lr, x, regs)
    r = sum(dc ** (a + b) * abs(x[0, i, j] - x[0, i + a, j + b]) for a in range(R + 1) for b in range(R + 1))
    tap = 2 * lam * w[0, i, j] * r * dc ** (2 * R - 2)
    g_m = g_ref.copy()
    g_m[0, i, j] -= tap
    assert 0 < tap <= 2e-5 * max(1.0, np.max(np.abs(g_ref)))  # invisible to the relative bar
    assert _caught(g_m, g_ref, M)


def test_matrix_covers_every_instance_and_edge_residue():
    """Every (S, B, leg) instance is in the matrix, and over each (S, leg) the right / bottom edge residues the tile
    kernel distinguishes are all reached: w mod 64 in {0, 1, 2, 63} LR cells, 1 and 2 column tiles, H mod 8 in
    {0, 1, R, 7} as far as a multiple of S can have that residue."""
    seen = {(S, B, leg) for S, B, leg, _, _ in CASES}
    assert seen == {(S, B, leg) for S in tm.SCALES for B in tm.BLURS for leg in tm.LEGS}
    for S in tm.SCALES:
        have = {(h * S) % 8 for h in range(8)}
        for leg in tm.LEGS:
            geos = tm.geometries(S, leg)
            assert {(W // S) % 64 for W, *_ in geos} == {0, 1, 2, 63}
            assert {-(-W // (64 * S)) for W, *_ in geos} >= {1, 2}
            want = {0, 1, tm.leg_reach(leg), 7}
            rows = {H % 8 for _, H, *_ in geos}
            assert rows >= (want & have)
            assert len(rows) >= min(len(have), 3)
            assert any(C > 1 for _, _, C, *_ in geos)
            for W, H, C, shifts, _ in geos:
                E = max(max(abs(a), abs(b)) for a, b in shifts)
                assert W % S == 0 and H % S == 0 and W > 4 * E + 2 * S and H > 4 * E + 2 * S
                if E:
                    assert {(a % S, b % S) for a, b in shifts} == {(a, b) for a in range(S) for b in range(S)}
                    assert [E, -E] in shifts and [-E, E] in shifts
