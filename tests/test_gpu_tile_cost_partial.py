"""The tile kernel k_eval_z publishes a workgroup's cost partial at the barrier between its two phases (the cost terms are
complete there); the g.d partial of the WD instances follows the g stores.  Every path that carries a partial, on the
smallest problems that reach it, in f64 and f32, against the CPU oracle at the bars of tests/test_gpu_configs.py (f64
1e-12; f32 2e-5 per gradient element, 1e-5 on the cost):
  * 520 x 520 HR, S = 4, 16 frames, blur 3, BTV(3): three tile columns (the last one partial), 65 tile rows, edge tiles,
    border blocks (shifts up to 3) -- all terms, TERM_DATA only, TERM_REG only, cost only (no gradient pointer), and a
    set_cost_rows band;
  * an S = 2 problem with shifts of both signs (border rectangles on every side);
  * a blur-free S = 3 problem with TV;
  * a short CG run whose line search evaluates through the g.d (WD) instances, against the oracle's mincg.
Three consecutive evaluations of one problem must return bit-identical cost and gradient: the in-kernel finish re-arms
the granules it consumed, and a partial published early must not be consumed twice or lost."""
import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

TOL_G = {0: 1e-12, 1: 2e-5}
TOL_F = {0: 1e-12, 1: 1e-5}

from parity_log import relerr  # noqa: E402  (max |a - ref| / max(1, |ref|))


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


class Case:
    """Inputs and the oracle's results of one problem (computed once per module, never modified)."""

    def __init__(self, seed, s, K, w, h, shifts, blur, reg):
        rng = np.random.default_rng(seed)
        self.s, self.K, self.w, self.h, self.shifts, self.blur, self.reg = s, K, w, h, shifts, blur, reg
        self.W, self.H = w * s, h * s
        model = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=blur[0], blur_sigma=blur[1])
        gt = rng.random((1, self.H, self.W))
        self.lr = np.stack([model.apply(gt, k) for k in range(K)]) + (5 / 255) * rng.standard_normal((K, 1, h, w))
        x = np.clip(gt + 0.05 * rng.standard_normal(gt.shape), 0, 1)
        self.x = np.round(x * 256) / 256  # ties exercise sgn(0) = 0
        self.wts = 0.5 + rng.random((1, self.H, self.W))
        ref = orc.Problem(model, self.lr)
        ref.set_irls_weights(ref.add_regularizer(*reg), self.wts)
        self.f_all, self.g_all = ref.objective(self.x)
        self.f_data, self.g_data = ref.data_term(self.x)
        self.f_reg, self.g_reg = ref.reg_term(0, self.x)
        for a in (self.lr, self.x, self.wts, self.g_all, self.g_data, self.g_reg):
            a.setflags(write=False)

    def problem(self, sr, ctx, dtype):
        p = sr.Problem(ctx, self.W, self.H, 1, self.K, self.s, self.shifts, self.blur[0], self.blur[1], dtype)
        p.set_observations(self.lr)
        p.set_irls_weights(p.add_regularizer(*self.reg), self.wts)
        assert p.active_impl() != sr.IMPL_DIRECT  # the tile kernel, not the direct family
        return p


@pytest.fixture(scope="module")
def main_case():
    s, K = 4, 16
    return Case(41, s, K, 130, 130, [[k % s, (k // s) % s] for k in range(K)], (3, 1.0), (2, 0.01, 3, 0.5))


@pytest.fixture(scope="module")
def s2_case():
    # HR 140 x 46: two tile columns (the second holds 6 of its 64 cells), six tile rows (the last one partial)
    return Case(42, 2, 4, 70, 23, [[0, 0], [-1, 1], [1, -1], [1, 1]], (3, 1.0), (2, 0.01, 2, 0.6))


@pytest.fixture(scope="module")
def blur_free_case():
    # HR 261 x 93 (S = 3: 192-pixel tile columns, the second partial), TV
    s, K = 3, 9
    return Case(43, s, K, 87, 31, [[k % s, (k // s) % s] for k in range(K)], (0, 0.0), (0, 0.01, 0, 0.0))


def check(f, g, f_ref, g_ref, dtype, what):
    ef = abs(f - f_ref) / max(1.0, abs(f_ref))
    eg = relerr(g, g_ref) if g is not None else 0.0
    print("%s dtype %d: cost err %.3e  gradient err %.3e" % (what, dtype, ef, eg))
    assert ef <= TOL_F[dtype], (what, ef)
    assert eg <= TOL_G[dtype], (what, eg)


@pytest.mark.parametrize("dtype", [0, 1])
def test_every_term_selection_matches_oracle(sr, ctx, main_case, dtype):
    c = main_case
    p = c.problem(sr, ctx, dtype)
    f, g = p.eval(c.x)
    check(f, g, c.f_all, c.g_all, dtype, "all terms")
    f, g = p.eval(c.x, sr.TERM_DATA)
    check(f, g, c.f_data, c.g_data, dtype, "data only")
    f, g = p.eval(c.x, sr.TERM_REG)
    check(f, g, c.f_reg, c.g_reg, dtype, "regulariser only")
    for terms, f_ref, what in ((sr.TERM_ALL, c.f_all, "cost only, all terms"), (sr.TERM_DATA, c.f_data, "cost only, data"),
                               (sr.TERM_REG, c.f_reg, "cost only, regulariser")):
        f, g = p.eval(c.x, terms, want_grad=False)
        assert g is None
        check(f, None, f_ref, None, dtype, what)
    # a cost-only evaluation leaves the next full one as it was
    f, g = p.eval(c.x)
    check(f, g, c.f_all, c.g_all, dtype, "all terms after cost only")


@pytest.mark.parametrize("dtype", [0, 1])
def test_cost_row_bands_sum_to_the_whole(sr, ctx, main_case, dtype):
    """set_cost_rows: the cost terms of the owned rows only, the gradient of every row.  Two bands that split the image
    (inside a tile row: 260 = 32 * 8 + 4) must sum to the oracle's cost, each with the oracle's gradient."""
    c = main_case
    p = c.problem(sr, ctx, dtype)
    total = 0.0
    for r0, r1 in ((0, 260), (260, c.H)):
        p.set_cost_rows(r0, r1)
        f, g = p.eval(c.x)
        assert 0.0 < f < c.f_all
        total += f
        assert relerr(g, c.g_all) <= TOL_G[dtype], (r0, r1)
    check(total, None, c.f_all, None, dtype, "sum of the bands")
    p.set_cost_rows(0, c.H)
    f, g = p.eval(c.x)
    check(f, g, c.f_all, c.g_all, dtype, "whole image again")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("which", ["s2", "blur_free"])
def test_other_instances_match_oracle(sr, ctx, s2_case, blur_free_case, which, dtype):
    c = s2_case if which == "s2" else blur_free_case
    p = c.problem(sr, ctx, dtype)
    f, g = p.eval(c.x)
    check(f, g, c.f_all, c.g_all, dtype, which + " all terms")
    f, g = p.eval(c.x, sr.TERM_DATA)
    check(f, g, c.f_data, c.g_data, dtype, which + " data only")
    f, g = p.eval(c.x, sr.TERM_ALL, want_grad=False)
    check(f, None, c.f_all, None, dtype, which + " cost only")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("which", ["main", "s2"])
def test_three_consecutive_evaluations_are_bit_identical(sr, ctx, main_case, s2_case, which, dtype):
    c = main_case if which == "main" else s2_case
    p = c.problem(sr, ctx, dtype)
    f0, g0 = p.eval(c.x)
    check(f0, g0, c.f_all, c.g_all, dtype, which + " first evaluation")
    for _ in range(2):
        f, g = p.eval(c.x)
        assert f == f0
        assert np.array_equal(g, g0)
    # a cost-only evaluation in between publishes and re-arms the same granules
    f, _ = p.eval(c.x, sr.TERM_ALL, want_grad=False)
    assert f == f0
    f, g = p.eval(c.x)
    assert f == f0 and np.array_equal(g, g0)


def test_short_cg_run_through_the_gd_instances(sr, ctx):
    """The solver's line search evaluates through k_eval_z<..., WD = true> (cost and g.d out of one launch, trial point
    folded into the window): three CG iterations on the tile path against the oracle's mincg (ALGLIB's when built) --
    same iteration / evaluation counts and termination, every accepted cost to 1e-11, x to 1e-8 (the bars of
    tests/test_gpu_sharded.py)."""
    rng = np.random.default_rng(44)
    s, K, h, w = 2, 4, 23, 70
    H, W = h * s, w * s
    shifts = [[0, 0], [-1, 1], [1, -1], [1, 1]]
    model = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=3, blur_sigma=1.0)
    gt = rng.random((1, H, W))
    lr = np.stack([model.apply(gt, k) for k in range(K)]) + 0.01 * rng.standard_normal((K, 1, h, w))
    ref = orc.Problem(model, lr)
    x0 = orc.resize_nearest(lr[0, 0], W, H)[None]
    trace = []
    x_ref, rep_ref = orc.mincg(lambda x: (lambda fg: (fg[0], fg[1].ravel()))(ref.objective(x.reshape(1, H, W))),
                               x0, 0.0, 0.0, 0.0, 3, use_alglib=orc.have_ref(), trace=trace)
    p = sr.Problem(ctx, W, H, 1, K, s, shifts, 3, 1.0, sr.F64)
    p.set_impl(sr.IMPL_TILED)
    p.set_observations(lr)
    x, its, nfev, term, ftrace = p.cg_trace(x0, 0.0, 0.0, 0.0, 3)
    assert (its, nfev, term) == (rep_ref.iterations, rep_ref.nfev, rep_ref.termination_type)
    assert len(ftrace) == nfev
    for _, f in trace[1:]:
        assert np.min(np.abs(ftrace - f) / max(1.0, abs(f))) <= 1e-11
    assert np.max(np.abs(x - x_ref.reshape(1, H, W))) <= 1e-8
    # the plain instance after the solve: the granules the WD launches used are armed for it
    f, g = p.eval(x)
    f_ref, g_ref = ref.objective(x)
    assert abs(f - f_ref) <= 1e-12 * max(1.0, abs(f_ref)) and relerr(g, g_ref) <= 1e-12
