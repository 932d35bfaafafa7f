"""The affine registration on the GPU (include/srmap.h: srmap_register_affine; k_affine_gn_sums and k_ssd_window of
csrc/registration_affine.hip, k_fit_reduce of csrc/motion_fit.hip) against its numpy restatement (tests/affine_registration_restatement.py),
against the matrices that made the frames, and against itself.

Bars.  One Gauss-Newton step: the corner displacement between the GPU's and the restatement's matrix is at most 100 x the
restatement's own sensitivity to the ORDER of its sums (the same step with the sums taken by rows, by columns and in
reverse), floor 1e-10 px -- the two evaluate the same positions bit for bit, what differs is summation order.  Whole runs:
1e-3 px, ten stop thresholds, since the two may stop one iteration apart.  Against the truth: the CPU contract's 0.05 px
(noise-free) and 0.1 px (sigma 0.01)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as orc

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import affine_registration_restatement as rg  # noqa: E402
import robust_restatement as rr  # noqa: E402
import test_affine_registration_cpu as cpu  # noqa: E402
from test_gpu_registration import texture  # noqa: E402

pytestmark = pytest.mark.gpu

LIBDIR = os.path.join(ROOT, "super-resolution_amd", "lib")


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


# ------------------------------------------------------------------------------------------- one step
def one_step_stack(H, W, n):
    """(stack, init, truth) of n frames: [1] a small rotation started nearby; [2] a translation large enough that whole
    rows (and columns) of the template have no valid pixel; [3] frame 0 itself started at the identity (its step is 0);
    [4] another rotation with scale."""
    img = texture(np.random.default_rng(H * 1000 + W), H, W)
    ty, tx = max(2.0, np.floor(0.3 * H)), max(1.0, np.floor(0.1 * W))
    truth = [ar.translation(0, 0), ar.rotation_about_centre(0.6, (0.3, -0.2), W, H),
             ar.translation(tx + 0.25, ty + 0.4), ar.translation(0, 0), ar.rotation_about_centre(-0.8, (-0.4, 0.3), W, H, 1.004)]
    init = [ar.translation(0, 0), ar.rotation_about_centre(0.5, (0.2, -0.1), W, H),
            ar.translation(tx + 0.1, ty + 0.3), ar.translation(0, 0), ar.rotation_about_centre(-0.7, (-0.3, 0.2), W, H)]
    stack = np.stack([img] + [img if k == 3 else cpu.warped(img, truth[k]) for k in range(1, n)])
    return stack, np.stack(init[:n]), np.stack(truth[:n])


def restated_steps(ref, img, F, count, order):
    for _ in range(count):
        Fn = rg.gn_step(ref, img, F, order)[0]
        if Fn is None:
            break
        F = Fn
    return F


def step_bar(stack, init, k, count=1):
    """100 x the restatement's summation-order sensitivity of frame k's step(s), floor 1e-10 px."""
    H, W = stack.shape[1:]
    Fs = [restated_steps(stack[0], stack[k], init[k], count, order) for order in ("rows", "cols", "reversed")]
    sens = max(rg.corner_displacement(Fs[0], Fs[1], W, H), rg.corner_displacement(Fs[0], Fs[2], W, H))
    return Fs[0], sens, max(100 * sens, 1e-10)


@pytest.mark.parametrize("n", [2, 5])
@pytest.mark.parametrize("size", [(8, 8), (9, 300), (37, 53), (64, 64), (70, 129)])
def test_one_step_matches_the_restatement(sr, ctx, size, n):
    H, W = size
    stack, init, _ = one_step_stack(H, W, n)
    got, q = ctx.register_affine(stack, init=init, max_levels=1, max_iterations=1, with_quality=True)
    assert np.array_equal(got[0], rg.identity())
    for k in range(1, n):
        F_ref, sens, bar = step_bar(stack, init, k)
        dev = rg.corner_displacement(got[k], F_ref, W, H)
        moved = rg.corner_displacement(F_ref, init[k], W, H)
        _, _, ee, cnt = rg.gn_sums(stack[0], stack[k], F_ref)
        print("%3d x %3d frame %d: GPU - restatement %.2e px (sensitivity %.2e, bar %.2e), step %.3f px, used %.3f"
              % (H, W, k, dev, sens, bar, moved, q[k, 2]))
        assert dev <= bar
        assert q[k, 0] == 1.0 and q[k, 3] == 1.0
        assert q[k, 2] == cnt / float(W * H)                      # the residual pass counts the same pixels
        assert abs(q[k, 1] - np.sqrt(ee / cnt)) <= 1e-12
    if n == 5:
        used = q[2, 2]
        assert used < 0.75                                        # rows and columns without a valid pixel were there


def test_a_converged_frame_is_skipped_without_changing_the_others(sr, ctx):
    H, W = 37, 53
    stack, init, _ = one_step_stack(H, W, 5)
    got, q = ctx.register_affine(stack, init=init, max_levels=1, max_iterations=2, with_quality=True)
    assert np.array_equal(got[3], rg.identity()) and q[3, 3] == 1.0 and q[3, 1] == 0.0   # exact start: one pass, step 0
    assert list(q[[1, 2, 4], 3]) == [2.0, 2.0, 2.0]
    keep = [0, 1, 2, 4]
    without = ctx.register_affine(stack[keep], init=init[keep], max_levels=1, max_iterations=2)
    assert np.array_equal(without, got[keep])                     # bit for bit
    for k in (1, 2, 4):
        F_ref, sens, bar = step_bar(stack, init, k, count=2)
        dev = rg.corner_displacement(got[k], F_ref, W, H)
        print("frame %d after two steps: GPU - restatement %.2e px (sensitivity %.2e, bar %.2e)" % (k, dev, sens, bar))
        assert dev <= bar


# ------------------------------------------------------------------------------------------- whole runs
@pytest.fixture(scope="module")
def contract():
    """{(H, W, noise): (stack, truth, restatement's matrices, its iteration counts)}, computed once."""
    out = {}
    for H, W in ((96, 128), (131, 157)):
        for noise in (0.0, 0.01):
            stack, truth = cpu.contract_stack(H, W, noise)
            ref, q = rg.register_affine(stack, with_quality=True)
            out[(H, W, noise)] = (stack, truth, ref, q[:, 3])
    return out


@pytest.mark.parametrize("noise", [0.0, 0.01])
@pytest.mark.parametrize("size", [(96, 128), (131, 157)])
def test_full_run_matches_the_restatement_and_the_truth(sr, ctx, contract, size, noise):
    H, W = size
    stack, truth, ref, its_ref = contract[(H, W, noise)]
    got, q = ctx.register_affine(stack, with_quality=True)
    for k, (name, _) in enumerate(cpu.contract_cases(W, H), start=1):
        dev = rg.corner_displacement(got[k], ref[k], W, H)
        err = rg.corner_displacement(got[k], truth[k], W, H)
        print("%3d x %3d noise %.2f %-12s GPU - restatement %.2e px, GPU - truth %.4f px, iterations GPU %d restatement %d, quality %s"
              % (H, W, noise, name, dev, err, q[k, 3], its_ref[k], np.round(q[k, :3], 4)))
        assert dev <= 1e-3
        assert err <= (cpu.NOISE_BAR if noise else cpu.NOISE_FREE_BAR)


def test_central_window_case(sr, ctx):
    H, W = 240, 320
    img = texture(np.random.default_rng(H + W), H, W)
    M = ar.rotation_about_centre(7, (0, 0), W, H)
    got, q = ctx.register_affine(np.stack([img, cpu.warped(img, M)]), with_quality=True)
    err = rg.corner_displacement(got[1], M, W, H)
    print("corner error %.4f px, quality %s" % (err, q[1]))
    assert err <= cpu.NOISE_FREE_BAR


def test_results_are_bit_identical_and_independent_of_the_other_frames(sr, ctx, contract):
    stack = contract[(131, 157, 0.01)][0]
    a, qa = ctx.register_affine(stack, with_quality=True)
    b, qb = ctx.register_affine(stack, with_quality=True)
    assert np.array_equal(a, b) and np.array_equal(qa, qb)
    perm = [0, 5, 3, 7, 1, 2, 6, 4]
    c, qc = ctx.register_affine(stack[perm], with_quality=True)
    assert np.array_equal(c, a[perm]) and np.array_equal(qc, qa[perm])


def test_hr_scale_returns_hr_pixel_matrices(sr, ctx):
    """LR frames from the library's own affine model at scale 2 (blur 3 / sigma 1): t comes back doubled, L unchanged."""
    H, W, s = 96, 128, 2
    img = texture(np.random.default_rng(9), H, W)
    mats = np.stack([ar.rotation_about_centre(d, sh, W, H) for d, sh in ((0, (0, 0)), (1.5, (1.25, .75)), (-2, (-3, 2)), (0.5, (.5, -1)))])
    p = sr.Problem(ctx, W, H, 1, len(mats), s, None, 3, 1.0, sr.F64)
    p.set_affine_motion(mats)
    lr = np.stack([p.apply(img[None], k)[0] for k in range(len(mats))])
    assert lr.shape == (4, H // s, W // s)
    got1 = ctx.register_affine(lr)
    got2 = ctx.register_affine(lr, hr_scale=s)
    assert np.array_equal(got2[:, :, :2], got1[:, :, :2]) and np.array_equal(got2[:, :, 2], s * got1[:, :, 2])
    ref = rg.register_affine(lr, hr_scale=s)
    for k in range(1, len(mats)):
        dev = rg.corner_displacement(got2[k], ref[k], W, H)    # HR corners, HR pixels: two LR thresholds' worth
        err = rg.corner_displacement(got2[k], mats[k], W, H)
        print("frame %d: GPU - restatement %.2e HR px, GPU - generating matrix %.3f HR px" % (k, dev, err))
        assert dev <= s * 1e-3
    # against the generating matrices the figure is printed only: the zero border of the warped, blurred frames biases a
    # dense estimate by a few tenths of an HR pixel (test_affine_registration_cpu.py holds the loop to the solve's PSNR)


def test_edge_and_error_paths(sr, ctx):
    rng = np.random.default_rng(5)
    img = texture(rng, 40, 48)
    pair = np.stack([img, cpu.warped(img, ar.translation(0.5, -0.25))])
    assert ctx.register_affine(np.zeros((0, 16, 16))).shape == (0, 2, 3)
    one, q1 = ctx.register_affine(pair[:1], with_quality=True)
    assert np.array_equal(one, rg.identity()[None]) and list(q1[0]) == [1.0, 0.0, 1.0, 0.0]
    for bad in (np.zeros((2, 4, 4)), np.zeros((2, 7, 40)), np.zeros((2, 40, 7))):
        with pytest.raises(sr.SrmapError) as e:
            ctx.register_affine(bad)
        assert e.value.status == sr.EINVAL
    with pytest.raises(sr.SrmapError) as e:
        ctx.register_affine(pair, struct_size=8)
    assert e.value.status == sr.EINVAL
    for v in (np.nan, np.inf):
        init = np.stack([ar.translation(0, 0), ar.translation(v, 0)])
        with pytest.raises(sr.SrmapError) as e:
            ctx.register_affine(pair, init=init)
        assert e.value.status == sr.EINVAL
    # frame 0's row of init is ignored, whatever it says
    init = np.stack([np.full((2, 3), np.nan), ar.translation(0, 0)])
    assert np.array_equal(ctx.register_affine(pair, init=init), ctx.register_affine(pair, init=np.stack([ar.translation(0, 0)] * 2)))
    # flat frames: the first candidate of the seed wins, no texture at any level: finite, no error
    flat, qf = ctx.register_affine(np.full((2, 64, 64), 0.5), with_quality=True)
    ref = rg.register_affine(np.full((2, 64, 64), 0.5))
    assert np.all(np.isfinite(flat)) and np.all(np.isfinite(qf)) and np.array_equal(flat, ref)
    # a start that leaves less than a quarter of the frame in view
    with pytest.raises(sr.SrmapError) as e:
        ctx.register_affine(pair, init=np.stack([ar.translation(0, 0), ar.translation(40, 0)]))
    assert e.value.status == sr.EINVAL and "Could not determine motion" in str(e.value)


# ------------------------------------------------------------------------------------------- end to end
def _table_problem(sr, ctx, T, y, mats):
    p = sr.Problem(ctx, T["W"], T["H"], T["C"], T["K"], T["s"], T["shifts"], T["blur"][0], T["blur"][1], sr.F64)
    if mats is not None:
        p.set_affine_motion(mats)
    p.set_observations(y)
    p.add_regularizer(*T["reg"])
    return p


@pytest.fixture(scope="module")
def table():
    return ar.table_inputs()


@pytest.mark.parametrize("name", ["0.5deg", "2deg"])
def test_frames_to_matrices_to_solve(sr, ctx, table, name):
    """Matrices estimated on the GPU from the LR frames, set_affine_motion, solve: the PSNR holds the restatement's pinned
    figure within max(0.01 dB, 10 x the restatement's PSNR change when its matrices move by 1e-3 px at the corners)."""
    T = table
    _, _, y = T["inputs"][name]
    x0 = rr.bilinear(y[0], T["s"])
    est = ctx.register_affine(y[:, 0], hr_scale=T["s"])
    est_ref = rg.register_affine(y[:, 0], hr_scale=T["s"])
    devs = [rg.corner_displacement(est[k], est_ref[k], T["W"], T["H"]) for k in range(1, T["K"])]
    x, rep = _table_problem(sr, ctx, T, y, est).solve(x0)
    ps = orc.psnr(T["gt"], x)
    pinned = cpu.TABLE[name]["estimated_l2"][0]
    moved = est_ref.copy()
    moved[1:, 0, 2] += 1e-3  # a translation moves all four corners by exactly that much
    x_m, _, _ = rr.irls_solve(ar.AffineImageModel(T["s"], moved, *T["blur"]), y, x0, reg=T["reg"], composed=True)
    sens = abs(orc.psnr(T["gt"], x_m) - pinned)
    x_t, _ = _table_problem(sr, ctx, T, y, None).solve(x0)
    ps_t = orc.psnr(T["gt"], x_t)
    print("%s: GPU - restatement matrices %s HR px; GPU estimated-affine L2 %.3f dB (%d/%d/%d), pinned %.2f dB, sensitivity %.4f dB; "
          "GPU translation-only L2 %.3f dB" % (name, np.array2string(np.array(devs), precision=2), ps, rep.irls_rounds,
                                               rep.cg_iterations, rep.evaluations, pinned, sens, ps_t))
    assert abs(ps - pinned) <= max(0.01, 10 * sens)
    if name == "2deg":
        assert ps >= ps_t + 10.0


def test_cli_registration_flags(sr, ctx, table, tmp_path):
    """super_resolution --generate_lr_images --affine_motion_path=<2 degrees> --registration=affine --save_motion_path:
    runs, writes a file AffineMotionSequence loads (six numbers per line; the facade binary's loader is the C++ side),
    and ends within 1 dB of the run given the true matrices."""
    from test_gpu_apps import _write_envi
    srbin = os.path.join(LIBDIR, "super_resolution")
    assert os.path.exists(srbin), "build() makes the tools"
    T = table
    Cn, H, W, s, K = T["C"], T["H"], T["W"], T["s"], T["K"]
    mats = T["inputs"]["2deg"][0]
    gt = T["gt"].astype(np.float32).astype(np.float64)
    gt_cfg = _write_envi(str(tmp_path / "gt"), gt)
    affine = tmp_path / "affine.txt"
    affine.write_text("".join(" ".join(repr(float(v)) for v in m.ravel()) + "\n" for m in mats))
    saved = tmp_path / "estimated.txt"

    def run(tag, *flags):
        res = str(tmp_path / ("result_" + tag))
        o = subprocess.run([srbin, "--data_path=" + gt_cfg, "--generate_lr_images", "--number_of_frames=%d" % K,
                            "--noise_sigma=2.55", "--upsampling_scale=%d" % s, "--blur_radius=3", "--blur_sigma=1.0",
                            "--affine_motion_path=" + str(affine), "--regularizer=btv", "--btv_scale_range=2",
                            "--regularization_parameter=0.005", "--result_path=" + res] + list(flags),
                           capture_output=True, text=True, timeout=600)
        print(o.stdout, o.stderr)
        assert o.returncode == 0
        return orc.psnr(gt, np.fromfile(res, dtype="<f4").reshape(Cn, H, W).astype(np.float64))

    ps_true = run("true")
    ps_est = run("estimated", "--registration=affine", "--save_motion_path=" + str(saved))
    ps_trans = run("translational", "--registration=translational")
    print("CLI: true matrices %.3f dB, --registration=affine %.3f dB, --registration=translational %.3f dB" % (ps_true, ps_est, ps_trans))
    assert abs(ps_est - ps_true) <= 1.0
    est = np.array([[float(v) for v in line.split()] for line in saved.read_text().splitlines()]).reshape(K, 2, 3)
    assert np.array_equal(est[0], rg.identity())
    errs = [rg.corner_displacement(est[k], mats[k], W, H) for k in range(1, K)]
    print("saved estimate: corner error per frame (HR px) %s" % np.round(errs, 3))
    # the saved file drives a second run as --affine_motion_path for the SOLVER only when frames are loaded; here: it loads
    again = tmp_path / "again"
    o = subprocess.run([srbin, "--data_path=" + gt_cfg, "--generate_lr_images", "--number_of_frames=%d" % K,
                        "--upsampling_scale=%d" % s, "--affine_motion_path=" + str(saved), "--optimization_iterations=1",
                        "--solver_iterations=2", "--result_path=" + str(again)], capture_output=True, text=True, timeout=600)
    assert o.returncode == 0, o.stderr
    # refusals
    for flags, word in ((["--registration=affine", "--affine_motion_path=" + str(affine)], "excludes"),
                        (["--registration=homography"], "'translational' or 'affine'"),
                        (["--save_motion_path=" + str(saved)], "needs --registration")):
        o = subprocess.run([srbin, "--data_path=" + str(tmp_path)] + flags, capture_output=True, text=True, timeout=120)
        assert o.returncode == 1 and word in o.stderr, (flags, o.stderr)


def test_host_facade_returns_what_the_c_call_returns():
    exe = os.path.join(LIBDIR, "affine_registration_test")
    assert os.path.exists(exe), "build() makes the facade test binary"
    o = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(o.stdout, o.stderr)
    assert o.returncode == 0 and "AFFINE REGISTRATION FACADE TESTS PASSED" in o.stdout
