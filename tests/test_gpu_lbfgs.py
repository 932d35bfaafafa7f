"""The L-BFGS inner solver on the GPU (srmap_problem_set_solver / srmap_lbfgs_trace; csrc/solver.hip run_lbfgs,
csrc/kernels_lbfgs.hip) against the numpy restatement of ALGLIB's minlbfgs (tests/lbfgs_restatement.py, bit-exact
against the reference's ALGLIB: tests/test_lbfgs_cpu.py), and against itself across the solver's switches."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as orc
import parity_log

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_restatement as lbr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


def _smooth_case(blur):
    rng = np.random.default_rng(9)
    s, K, h, w = 2, 4, 20, 28
    H, W = h * s, w * s
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    model = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=blur, blur_sigma=1.0 if blur else 0.0)
    gt = rng.random((1, H, W))
    lr = np.stack([model.apply(gt, k) for k in range(K)]) + 0.01 * rng.standard_normal((K, 1, h, w))
    x0 = orc.resize_nearest(lr[0, 0], W, H)[None]
    return s, K, H, W, shifts, model, lr, x0


@pytest.mark.parametrize("m", [1, 3, 5, 7])
@pytest.mark.parametrize("blur", [0, 3])
def test_lbfgs_trajectory_matches_minlbfgs(sr, ctx, blur, m):
    """run_lbfgs against minlbfgs on the SMOOTH data term: same iteration count, evaluation count and termination, the
    cost of every accepted iterate present in the GPU's evaluation log to 1e-11, x to 1e-8."""
    s, K, H, W, shifts, model, lr, x0 = _smooth_case(blur)
    ref = orc.Problem(model, lr)
    eps = 1e-7
    xrep = []
    x_ref, rep_ref = lbr.minlbfgs(lambda v: (lambda fg: (fg[0], fg[1].ravel()))(ref.objective(v.reshape(1, H, W))),
                                  x0, m, eps, eps, eps, 40, xrep=xrep)
    p = sr.Problem(ctx, W, H, 1, K, s, shifts, blur, 1.0 if blur else 0.0, sr.F64)
    p.set_observations(lr)
    x, its, nfev, term, ftrace = p.lbfgs_trace(x0, m, eps, eps, eps, 40)
    print("m %d: iterations %d/%d nfev %d/%d termination %d/%d" % (m, its, rep_ref.iterations, nfev, rep_ref.nfev, term,
                                                                     rep_ref.termination_type))
    assert (its, nfev, term) == (rep_ref.iterations, rep_ref.nfev, rep_ref.termination_type)
    assert len(ftrace) == nfev
    worst = 0.0
    for _, f in xrep[1:]:
        worst = max(worst, float(np.min(np.abs(ftrace - f) / max(1.0, abs(f)))))
    parity_log.note(worst, "f")
    assert worst <= 1e-11
    assert parity_log.relerr(x, x_ref.reshape(1, H, W)) <= 1e-8


def _cfg1():
    import bench
    s, K, W, H = 2, 4, 256, 256
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    gt = bench.synth_ground_truth(W, H, 1)
    model = orc.ImageModel(scale=s, shifts=shifts)
    lr = np.stack([model.apply(gt, k) for k in range(K)])
    lr = lr + (5.0 / 255.0) * np.random.default_rng(777).standard_normal(lr.shape)
    return gt, lr, bench.bilinear_upsample(lr[0], s), s, shifts, (0, 0.0), (orc.REG_TV, 0.01, 0, 0.0)


def _cfg2(W=512, H=512, seed=777):
    import bench
    s, K = 4, 16
    shifts = [[k % s, (k // s) % s] for k in range(K)]
    gt = bench.synth_ground_truth(W, H, 1)
    model = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=3, blur_sigma=1.0)
    lr = np.stack([model.apply(gt, k) for k in range(K)])
    lr = lr + (5.0 / 255.0) * np.random.default_rng(seed).standard_normal(lr.shape)
    return gt, lr, bench.bilinear_upsample(lr[0], s), s, shifts, (3, 1.0), (orc.REG_BTV, 0.01, 3, 0.5)


def _gpu_solve(sr, ctx, lr, x0, s, shifts, blur, reg, m=5, dtype=0, opts=None, impl=None):
    K, C, h, w = lr.shape
    p = sr.Problem(ctx, w * s, h * s, C, K, s, shifts, blur[0], blur[1], dtype)
    if impl is not None:
        p.set_impl(impl)
    p.set_observations(lr)
    p.add_regularizer(*reg)
    p.set_solver(sr.SOLVER_LBFGS, m)
    return p.solve(x0, opts)


def _compare(sr, ctx, case, cost_tol=1e-9, x_tol=1e-7):
    gt, lr, x0, s, shifts, blur, reg = case
    model = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=blur[0], blur_sigma=blur[1])
    ref = orc.Problem(model, lr)
    ref.add_regularizer(*reg)
    x_ref, rep_ref = lbr.oracle_solve(ref, x0, m=5)
    x, rep = _gpu_solve(sr, ctx, lr, x0, s, shifts, blur, reg)
    psnr0, psnr_ref, psnr_gpu = orc.psnr(gt, x0), orc.psnr(gt, x_ref), orc.psnr(gt, x)
    print("PSNR x0 %.4f | oracle L-BFGS %.4f | GPU L-BFGS %.4f dB; IRLS rounds %d/%d, iterations %d/%d, evaluations %d/%d, "
          "final cost %.12g / %.12g, max |x - x_ref| %.3e" % (
              psnr0, psnr_ref, psnr_gpu, rep_ref.irls_rounds, rep.irls_rounds, rep_ref.cg_iterations, rep.cg_iterations,
              rep_ref.nfev, rep.evaluations, rep_ref.final_cost, rep.final_cost, np.max(np.abs(x - x_ref))))
    parity_log.note(abs(psnr_ref - psnr_gpu), "psnr")
    parity_log.note(abs(rep.final_cost - rep_ref.final_cost) / abs(rep_ref.final_cost), "cost")
    parity_log.note(np.max(np.abs(x - x_ref)), "x")
    assert abs(psnr_ref - psnr_gpu) < 0.01
    assert (rep.irls_rounds, rep.cg_iterations, rep.evaluations) == (rep_ref.irls_rounds, rep_ref.cg_iterations, rep_ref.nfev)
    assert abs(rep.final_cost - rep_ref.final_cost) <= cost_tol * abs(rep_ref.final_cost)
    assert np.max(np.abs(x - x_ref)) <= x_tol
    return ref, x_ref, rep_ref, x, rep


def test_cfg1_lbfgs_solve_matches_oracle(sr, ctx):
    """configs[0] exactly (TV): cost and iterate bars are the oracle's own sensitivity to a 1e-14 perturbation of x0
    (test_gpu_solve_parity.py::test_cfg1_solve_matches_oracle), measured here for the L-BFGS solve."""
    case = _cfg1()
    ref, x_ref, rep_ref, x, rep = _compare(sr, ctx, case, cost_tol=1e-6, x_tol=1e-3)
    x0 = case[2]
    rng = np.random.default_rng(1)
    x_p, rep_p = lbr.oracle_solve(ref, x0 * (1 + 1e-14 * rng.standard_normal(x0.shape)), m=5)
    own_cost, own_x = abs(rep_p.final_cost - rep_ref.final_cost), np.max(np.abs(x_p - x_ref))
    print("oracle under a 1e-14 perturbation of x0: cost %.3e, x %.3e; GPU vs oracle: %.3e, %.3e" % (
        own_cost, own_x, abs(rep.final_cost - rep_ref.final_cost), np.max(np.abs(x - x_ref))))
    assert abs(rep.final_cost - rep_ref.final_cost) <= 10 * max(own_cost, 1e-12 * abs(rep_ref.final_cost))
    assert np.max(np.abs(x - x_ref)) <= 10 * max(own_x, 1e-9)


def test_cfg2_class_lbfgs_solve_matches_oracle(sr, ctx):
    """configs[1]-class at 512 x 512 HR (16 frames, blur 3 / 1.0, BTV(3, 0.5)): the bars of test_gpu_solve_parity.py."""
    _compare(sr, ctx, _cfg2())


SUBPIX = (4, 3, 200, 136, 1, 16, (2, 0.01, 3, 0.5), 0)


@pytest.mark.parametrize("case", range(10))
def test_lbfgs_fold_equals_separate_passes(sr, ctx, case):
    """host_paced_passes = 1 (every trial point formed by its own pass from the stored d) against 0 (the evaluation forms
    it from the unnormalised L-BFGS direction and the norms on the device): bit for bit, over the geometries of
    test_gpu_solve_parity.py::test_fold_equals_separate_passes_over_geometries and one with sub-pixel shifts."""
    from test_gpu_solve_parity import FOLD_GEOMS
    s, b, W, H, C, K, reg, dtype = (FOLD_GEOMS + [SUBPIX])[case]
    rng = np.random.default_rng(900 + case)
    if case < len(FOLD_GEOMS):
        shifts = [[int(rng.integers(-(s - 1), s)), int(rng.integers(-(s - 1), s))] for _ in range(K)]
    else:
        shifts = [[float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2))] for _ in range(K)]
    shifts[0] = [0, 0]
    w, h = W // s, H // s
    W, H = w * s, h * s
    lr = rng.random((K, C, h, w))
    x0 = rng.random((C, H, W))
    out = {}
    for paced in (0, 1):
        p = sr.Problem(ctx, W, H, C, K, s, shifts, b, 1.0 if b > 1 else 0.0, dtype)
        p.set_observations(lr)
        p.add_regularizer(*reg)
        p.set_solver(sr.SOLVER_LBFGS, 3 + case % 3)
        opts = sr.default_irls_options()
        opts.max_num_irls_iterations = 2
        opts.max_num_solver_iterations = 8
        opts.host_paced_passes = paced
        x, rep = p.solve(x0, opts)
        out[paced] = (x, rep.irls_rounds, rep.cg_iterations, rep.evaluations, rep.final_cost)
    assert out[0][1:] == out[1][1:]
    assert np.array_equal(out[0][0], out[1][0])


@pytest.mark.parametrize("blur", [1, 3])
def test_lbfgs_tiles_match_direct_kernels(sr, ctx, blur):
    """The same L-BFGS run on the tile kernels and on the direct kernels: same counts, f to 1e-11, x to 1e-9."""
    rng = np.random.default_rng(31 + blur)
    s, K, W, H = 4, 16, 200, 136
    shifts = [[k % s, (k // s) % s] for k in range(K)]
    lr = rng.random((K, 1, H // s, W // s))
    x0 = rng.random((1, H, W))
    res = {}
    for impl in (sr.IMPL_TILED, sr.IMPL_DIRECT):
        p = sr.Problem(ctx, W, H, 1, K, s, shifts, blur, 1.0 if blur > 1 else 0.0, sr.F64)
        p.set_impl(impl)
        p.set_observations(lr)
        p.add_regularizer(sr.REG_BTV, 0.01, 3, 0.5)
        res[impl] = p.lbfgs_trace(x0, 5, 1e-7, 1e-7, 1e-7, 30)
    (xa, ia, na, ta, fa), (xb, ib, nb, tb, fb) = res[sr.IMPL_TILED], res[sr.IMPL_DIRECT]
    assert (ia, na, ta) == (ib, nb, tb)
    assert parity_log.relerr(fa, fb) <= 1e-11
    assert parity_log.relerr(xa, xb) <= 1e-9


def test_lbfgs_f32_solve_psnr(sr, ctx):
    """An f32 L-BFGS solve of the cfg2 class ends within 0.01 dB PSNR of the f64 one."""
    gt, lr, x0, s, shifts, blur, reg = _cfg2()
    x64, r64 = _gpu_solve(sr, ctx, lr, x0, s, shifts, blur, reg, dtype=sr.F64)
    x32, r32 = _gpu_solve(sr, ctx, lr, x0, s, shifts, blur, reg, dtype=sr.F32)
    p64, p32 = orc.psnr(gt, x64), orc.psnr(gt, x32)
    print("PSNR f64 %.4f (%d its, %d evals) f32 %.4f (%d its, %d evals)" % (p64, r64.cg_iterations, r64.evaluations, p32,
                                                                          r32.cg_iterations, r32.evaluations))
    assert abs(parity_log.note(p64 - p32, "psnr")) < 0.01


def test_lbfgs_split_channels_equals_per_channel_solves(sr, ctx):
    """split_channels with C = 3: every channel solved on its own, bit for bit the one-channel solves."""
    rng = np.random.default_rng(55)
    s, K, W, H, C = 2, 4, 96, 64, 3
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    lr = rng.random((K, C, H // s, W // s))
    x0 = rng.random((C, H, W))
    opts = sr.default_irls_options()
    opts.split_channels = 1
    opts.max_num_irls_iterations = 3
    x, rep = _gpu_solve(sr, ctx, lr, x0, s, shifts, (3, 1.0), (sr.REG_TV, 0.01), opts=opts)
    its = evs = 0
    for c in range(C):
        o = sr.default_irls_options()
        o.max_num_irls_iterations = 3
        xc, rc = _gpu_solve(sr, ctx, lr[:, c:c + 1], x0[c:c + 1], s, shifts, (3, 1.0), (sr.REG_TV, 0.01), opts=o)
        assert np.array_equal(x[c:c + 1], xc), c
        its += rc.cg_iterations
        evs += rc.evaluations
    assert (rep.cg_iterations, rep.evaluations) == (its, evs)


def test_lbfgs_argument_and_sharding_errors(sr, ctx):
    rng = np.random.default_rng(2)
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    p = sr.Problem(ctx, 48, 32, 1, 4, 2, shifts, 3, 1.0, sr.F64)
    p.set_observations(rng.random((4, 1, 16, 24)))
    p.add_regularizer(sr.REG_TV, 0.01)
    for solver, m, status in ((sr.SOLVER_LBFGS, 0, sr.EINVAL), (sr.SOLVER_LBFGS, 9, sr.EUNSUPPORTED), (7, 5, sr.EINVAL)):
        with pytest.raises(sr.SrmapError) as e:
            p.set_solver(solver, m)
        assert e.value.status == status
    x0 = rng.random((1, 32, 48))
    for m, status in ((0, sr.EINVAL), (9, sr.EUNSUPPORTED)):
        with pytest.raises(sr.SrmapError) as e:
            p.lbfgs_trace(x0, m, 1e-6, 1e-6, 1e-6, 5)
        assert e.value.status == status
    p.set_solver(sr.SOLVER_LBFGS, 5)

    class NoExchange:
        """A torch.distributed stand-in that records every collective the solve would make."""
        calls = []

        class ReduceOp:
            SUM, MAX = 0, 1

        def all_reduce(self, *a, **k):
            self.calls.append("all_reduce")

        def isend(self, *a, **k):
            self.calls.append("isend")

        def irecv(self, *a, **k):
            self.calls.append("irecv")

    fake = NoExchange()
    comm = sr.Comm(ctx, 0, 2, backend="host", dist=fake)
    for mode in (sr.SHARD_FRAMES, sr.SHARD_ROWS, sr.SHARD_CHANNELS):
        sd = sr.ShardDesc()
        sd.mode = mode
        sd.own_row0, sd.own_row1, sd.own_ch0, sd.own_ch1 = 0, 32, 0, 1
        with pytest.raises(sr.SrmapError) as e:
            p.solve(x0, comm=comm, shard=sd)
        assert e.value.status == sr.EUNSUPPORTED
    assert fake.calls == []
    # the problem still solves unsharded with L-BFGS, and with CG again after switching back
    x, rep = p.solve(x0)
    assert np.all(np.isfinite(x)) and rep.cg_iterations > 0
    p.set_solver(sr.SOLVER_CG)
    x, rep = p.solve(x0)
    assert np.all(np.isfinite(x)) and rep.cg_iterations > 0


def test_cli_solver_flag(sr, ctx, tmp_path):
    """super_resolution --solver=lbfgs runs L-BFGS: its result equals a Python L-BFGS solve from the tool's own x0 (bit
    for bit in the float32 result file); --solver=bogus warns and runs CG, the same file as --solver=cg."""
    import __graft_entry__ as ge
    from test_gpu_apps import _ground_truth, _read_envi, _write_envi
    ge.build_lib()
    gen, srbin = ge.build_apps()
    C, H, W, s, K = 1, 48, 64, 2, 4
    gt = _ground_truth(C, H, W)
    gt_cfg = _write_envi(str(tmp_path / "gt"), gt)
    motion = tmp_path / "motion.txt"
    motion.write_text("0 0\n1 1\n0 1\n1 0\n")
    lr_dir = tmp_path / "lr"
    lr_dir.mkdir()
    out = subprocess.run([gen, "--input_image=" + gt_cfg, "--output_image_dir=" + str(lr_dir),
                          "--motion_sequence_path=" + str(motion), "--blur_radius=3", "--blur_sigma=1.0",
                          "--downsampling_scale=%d" % s, "--number_of_frames=%d" % K],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    frames = np.stack([_read_envi(str(lr_dir / ("low_res_%d" % i)), (C, H // s, W // s)) for i in range(K)])

    def run(solver):
        res = str(tmp_path / ("result_" + solver))
        o = subprocess.run([srbin, "--data_path=" + str(lr_dir), "--upsampling_scale=%d" % s, "--blur_radius=3",
                            "--blur_sigma=1.0", "--motion_sequence_path=" + str(motion), "--regularizer=btv",
                            "--btv_scale_range=2", "--regularization_parameter=0.001", "--optimization_iterations=5",
                            "--solver_iterations=30", "--solver=" + solver, "--result_path=" + res,
                            "--save_initial_estimate=" + str(tmp_path / ("x0_" + solver))],
                           capture_output=True, text=True, timeout=600)
        print(o.stdout, o.stderr)
        assert o.returncode == 0
        return res, o.stderr

    res_lb, err_lb = run("lbfgs")
    assert "WARNING" not in err_lb
    x0 = np.fromfile(str(tmp_path / "x0_lbfgs"), dtype=np.float64).reshape(C, H, W)
    p = sr.Problem(ctx, W, H, C, K, s, [[0, 0], [1, 1], [0, 1], [1, 0]], 3, 1.0, sr.F64)
    p.set_observations(frames)
    p.add_regularizer(sr.REG_BTV, 0.001, 2, 0.5)
    p.set_solver(sr.SOLVER_LBFGS, 5)
    o = sr.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = 5, 30
    x, _ = p.solve(x0, o)
    cli = np.fromfile(res_lb, dtype="<f4").reshape(C, H, W)
    assert np.array_equal(x.astype(np.float32), cli)
    res_cg, err_cg = run("cg")
    res_bogus, err_bogus = run("bogus")
    assert "WARNING" in err_bogus
    assert open(res_cg, "rb").read() == open(res_bogus, "rb").read()
    assert open(res_cg, "rb").read() != open(res_lb, "rb").read()
