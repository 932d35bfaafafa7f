"""The dense flow registration on the GPU (include/srmap.h: srmap_register_flow; k_flow_lk_pass, k_flow_smooth,
k_flow_resample, k_flow_finish and k_flow_maxdiff of csrc/registration_flow.hip) against its numpy restatement
(tests/flow_registration_restatement.py) and against itself.

Bars.  One warp pass at one level (u in -> u out): 100 x the restatement's own sensitivity to the ORDER of its window and
box sums (the same pass with the sums taken along y first and descending), floor 1e-12 px -- the two evaluate the same
positions bit for bit, and the kernels keep fp contraction off.  Whole runs: 1e-6 px, the mask identical, the quality
figures within 1e-10.  These tests fail on the parent commit: srmap_register_flow and Context.register_flow do not exist."""
import os
import sys

import numpy as np
import pytest

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import flow_registration_restatement as fq  # noqa: E402
import flow_restatement as fr  # noqa: E402
import robust_restatement as rr  # noqa: E402
import test_flow_registration_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    return sr.Context(0)


# ------------------------------------------------------------------------------------------- one pass
def one_pass_stack(H, W, n):
    """(stack, init) of n frames: [1] a smooth deformation on a small rotation, started at the rotation; [2] started at a
    translation that pushes a third of the taps outside; [3] frame 0 itself started at the identity; [4] a deformation
    started at a rotation with scale."""
    img = cpu.texture(H * 1000 + W, H, W)
    tx = np.floor(0.34 * W) + 0.3
    init = [ar.translation(0, 0), ar.rotation_about_centre(0.7, (0.3, -0.2), W, H), ar.translation(tx, -0.4),
            ar.translation(0, 0), ar.rotation_about_centre(-1.1, (-0.4, 0.6), W, H, 1.01)]
    fields = fr.from_affine(init, H, W)
    fields[1] += fr.sinusoid(H, W, 0.4, 23.0)
    fields[2] += 0.2
    fields[4] += fr.sinusoid(H, W, 0.3, 17.0, phase=0.5)
    stack = np.stack([img] + [cpu.warp_by_field(img, fields[k]) for k in range(1, n)])
    return stack, np.stack(init[:n])


def pass_reference(stack, init, k, r, smooth):
    """(u out of the restatement, its summation-order sensitivity) of frame k."""
    H, W = stack.shape[1:]
    u0 = fq.affine_start(init[k], 1, H, W)
    a = fq.lk_pass(stack[0], stack[k], u0, r, 0.05, smooth)
    b = fq.lk_pass(stack[0], stack[k], u0, r, 0.05, smooth, order="permuted")
    return a, float(np.max(np.abs(a - b))), u0


# the tiles are 32 x 16 (r <= 4) and 16 x 16 (r > 4): 31 / 32 / 33 and 17 straddle one tile's width
SIZES = [(16, 16), (17, 23), (33, 47), (70, 129), (20, 31), (20, 32), (19, 33), (33, 17)]
VARIANTS = [(1, 0, 2), (4, 2, 5), (8, 2, 2), (4, 0, 2), (8, 0, 5), (1, 2, 5)]


@pytest.mark.parametrize("r,smooth,n", VARIANTS)
@pytest.mark.parametrize("size", SIZES)
def test_one_pass_matches_the_restatement(ctx, size, r, smooth, n):
    H, W = size
    stack, init = one_pass_stack(H, W, n)
    flow, valid, q = ctx.register_flow(stack, init=init, max_levels=1, warps=1, window_radius=r, smooth_radius=smooth)
    assert np.all(flow[0] == 0) and np.all(valid[0] == 1)
    for k in range(1, n):
        ref, sens, u0 = pass_reference(stack, init, k, r, smooth)
        err = float(np.max(np.abs(flow[k] - ref)))
        bar = max(100 * sens, 1e-12)
        print("%dx%d r=%d smooth=%d frame %d: |GPU - restatement| %.2e px (sensitivity %.2e, bar %.2e), step %.3f px"
              % (H, W, r, smooth, k, err, sens, bar, np.max(np.abs(ref - u0))))
        assert np.all(np.isfinite(flow[k]))
        assert err <= bar, (k, err, bar)
        if k == 2:
            assert 0.3 <= 1 - np.mean(fq.inside(u0)[0]) <= 0.45
        assert np.array_equal(valid[k], fq.valid_mask(ref, 3).astype(np.float64))


def test_a_textureless_stack_keeps_its_start(ctx):
    """det = 0 everywhere: du = 0, no NaN; the field stays the start's (the box mean of a constant is that constant only up
    to rounding, so the start is u = 0)."""
    flat = np.full((3, 24, 40), 0.5)
    flow, valid, q = ctx.register_flow(flat)
    assert np.all(flow == 0.0) and np.all(np.isfinite(q))
    ref = fq.register_flow(flat)
    assert np.array_equal(valid, ref[1]) and np.array_equal(q, ref[2])


# ------------------------------------------------------------------------------------------- whole runs
@pytest.fixture(scope="module")
def whole_runs():
    out = {}
    for H, W in ((33, 47), (70, 129), (48, 64)):
        stack = cpu.deformed_stack(H, W, 3)
        out[(H, W)] = (stack, fq.register_flow(stack, hr_scale=2))
    return out


@pytest.mark.parametrize("size", [(33, 47), (70, 129), (48, 64)])
def test_whole_runs_match_the_restatement(ctx, whole_runs, size):
    stack, (rflow, rvalid, rq) = whole_runs[size]
    assert fq.num_levels(size[1], size[0]) == {33: 2, 70: 3, 48: 2}[size[0]]
    flow, valid, q = ctx.register_flow(stack, hr_scale=2)
    err = float(np.max(np.abs(flow - rflow)))
    print("%s: |GPU - restatement| %.2e px, quality %.2e, largest displacement %.2f px" %
          (size, err, np.max(np.abs(q - rq)), np.max(np.abs(rflow))))
    assert err <= 1e-6
    assert np.array_equal(valid, rvalid)
    assert np.max(np.abs(q - rq)) <= 1e-10


def test_repeats_are_bit_identical_and_frames_do_not_see_each_other(ctx):
    stack = cpu.deformed_stack(40, 72, 4)
    a = ctx.register_flow(stack, hr_scale=2)
    b = ctx.register_flow(stack, hr_scale=2)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    perm = [0, 3, 1, 2]
    c = ctx.register_flow(stack[perm], hr_scale=2)
    for x, y in zip(a, c):
        assert np.array_equal(x[perm], y)
    d = ctx.register_flow(stack[[0, 2]], hr_scale=2)
    for x, y in zip(a, d):
        assert np.array_equal(x[[0, 2]], y)


# ------------------------------------------------------------------------------------------- options and errors
@pytest.mark.parametrize("scale", [1, 2, 3, 4])
def test_hr_scale(ctx, scale):
    H, W = 21, 34
    stack = cpu.deformed_stack(H, W, 2)
    flow, valid, q = ctx.register_flow(stack, hr_scale=scale)
    u, rvalid, rq, _ = fq.register_pair(stack[0], stack[1], 1)
    assert flow.shape == (2, 2, scale * H, scale * W)
    assert np.max(np.abs(flow[1] - fq.to_output(u, scale))) <= 1e-9
    assert np.array_equal(flow[1][:, ::scale, ::scale], scale * ctx.register_flow(stack)[0][1])
    assert np.array_equal(valid[1], rvalid)


def test_initial_matrices_max_levels_and_the_other_options(ctx):
    H, W = 40, 72
    img = cpu.texture(5, H, W)
    M = ar.rotation_about_centre(3.0, (2.5, -1.5), W, H)
    stack = np.stack([img, cpu.warp_by_field(img, fr.from_affine([M], H, W)[0])])
    init = np.stack([ar.translation(0, 0), M])
    for kw in (dict(init=init), dict(init=init, max_levels=1, warps=3), dict(max_levels=1, warps=2, damping=0.5, valid_margin=0),
               dict(window_radius=2, smooth_radius=1, valid_margin=7, warps=4), dict(max_levels=7)):
        got = ctx.register_flow(stack, hr_scale=2, **kw)
        ref = fq.register_flow(stack, hr_scale=2, **kw)
        assert np.max(np.abs(got[0] - ref[0])) <= 1e-6, kw
        assert np.array_equal(got[1], ref[1]), kw
        assert np.max(np.abs(got[2] - ref[2])) <= 1e-10, kw
    # row 0 of the initial matrices is ignored
    init2 = init.copy()
    init2[0] = np.nan
    assert np.array_equal(ctx.register_flow(stack, init=init2)[0], ctx.register_flow(stack, init=init)[0])


def test_error_paths(sr, ctx):
    pair = cpu.deformed_stack(16, 20, 2)
    f, v, q = ctx.register_flow(np.zeros((0, 16, 16)))
    assert f.shape == (0, 2, 16, 16) and v.shape == (0, 16, 16) and q.shape == (0, 3)
    f, v, q = ctx.register_flow(pair[:1], hr_scale=3)
    assert np.all(f == 0) and np.all(v == 1) and np.array_equal(q, [[0.0, 1.0, 0.0]])
    bad = [dict(images=np.zeros((2, 15, 40))), dict(images=np.zeros((2, 40, 15))), dict(struct_size=8), dict(hr_scale=0),
           dict(warps=0), dict(window_radius=0), dict(window_radius=9), dict(smooth_radius=-1), dict(smooth_radius=9),
           dict(damping=-0.1), dict(damping=np.nan), dict(valid_margin=-1), dict(max_levels=-1)]
    for name, value in (("nan", np.nan), ("inf", np.inf)):
        im = pair.copy()
        im[1, 3, 4] = value
        bad.append(dict(images=im))
    for m in (np.full((2, 3), np.nan), ar.rotation_about_centre(20.0, (0, 0), 20, 16)):
        bad.append(dict(init=np.stack([ar.translation(0, 0), m])))
    for kw in bad:
        kw = dict(kw)
        images = kw.pop("images", pair)
        with pytest.raises(sr.SrmapError) as e:
            ctx.register_flow(images, **kw)
        assert e.value.status == sr.EINVAL, kw
    lib = sr.load()
    out = np.zeros((2, 2, 16, 20))
    assert lib.srmap_register_flow(None, 2, 20, 16, pair.ctypes.data_as(sr.c_double_p), None, out.ctypes.data_as(sr.c_double_p),
                                   None, None) == sr.EINVAL
    # NULL options = the defaults; valid_out and quality_out are optional
    assert lib.srmap_register_flow(ctx._h, 2, 20, 16, pair.ctypes.data_as(sr.c_double_p), None, out.ctypes.data_as(sr.c_double_p),
                                   None, None) == sr.OK
    assert np.array_equal(out, ctx.register_flow(pair)[0])


# ------------------------------------------------------------------------------------------- frames -> fields -> solve
@pytest.fixture(scope="module")
def table():
    return fr.table_inputs()


def test_the_table_frames_register_as_the_restatement_pins(ctx, table):
    T = table
    flow, valid, q = ctx.register_flow(T["y"][:, 0], hr_scale=T["s"])
    errs = [fq.endpoint_error(flow[k], T["fields"][k]) for k in range(1, T["K"])]
    print("mean endpoint error %.4f HR px (pinned %.3f)" % (np.mean(errs), cpu.PINNED["epe_noisy"]))
    assert abs(np.mean(errs) - cpu.PINNED["epe_noisy"]) <= 1e-3
    assert abs(1 - np.mean(valid[1:]) - cpu.PINNED["off_margin3"]) <= 1e-12
    assert np.all(q[1:, 2] <= fr.NEIGHBOUR_BOUND)


@pytest.mark.parametrize("variant", ["l2", "huber", "mask3"])
def test_register_set_flow_weights_and_solve(sr, ctx, table, variant):
    """Frames -> register_flow -> set_flow + the validity mask as data weights -> solve, against the figures
    tests/test_flow_registration_cpu.py pins: the same rounds / iterations / evaluations and PSNR within 0.01 dB."""
    T = table
    flow, valid, _ = ctx.register_flow(T["y"][:, 0], hr_scale=T["s"])
    p = sr.Problem(ctx, T["W"], T["H"], T["C"], T["K"], T["s"], T["shifts"], T["blur"][0], T["blur"][1], sr.F64)
    p.set_flow(flow)
    p.set_observations(T["y"])
    p.add_regularizer(*T["reg"])
    if variant == "huber":
        p.set_data_loss(sr.DATA_LOSS_HUBER, T["delta"])
    if variant == "mask3":
        p.set_data_weights(np.broadcast_to(valid[:, None], T["y"].shape).copy())
    x, rep = p.solve(rr.bilinear(T["y"][0], T["s"]), sr.default_irls_options())
    ps, counts = orc.psnr(T["gt"], x), (rep.irls_rounds, rep.cg_iterations, rep.evaluations)
    ps_ref, counts_ref = cpu.PINNED["solve_" + variant]
    print("%s: GPU %.3f dB %s | restatement %.3f dB %s" % (variant, ps, counts, ps_ref, counts_ref))
    assert counts == counts_ref
    assert abs(ps - ps_ref) <= 0.01
    if variant == "mask3":
        assert ps >= fr.TABLE["translation_l2"][0] + 12.0 and abs(ps - fr.TABLE["flow_l2"][0]) <= 0.5


# ------------------------------------------------------------------------------------------- the tools and the facade
def test_cli_registration_flow_and_save_flow_path(sr, ctx, tmp_path):
    """On the 48 x 64, four-frame burst of tests/test_gpu_flow.py (generate_data --flow_motion_path): super_resolution
    --registration=flow ends where the restatement's registration and masked solve of the same frames end (PSNR within
    0.01 dB) and beats --registration=translational by more than 5 dB; --save_flow_path holds the library's fields bit for
    bit and round-trips through --flow_motion_path (with --data_loss=huber, which runs without the masks, to the same PSNR)."""
    import subprocess
    from conftest import ROOT
    from test_gpu_apps import _read_envi, _write_envi
    libdir = os.path.join(ROOT, "super-resolution_amd", "lib")
    gen, srbin = os.path.join(libdir, "generate_data"), os.path.join(libdir, "super_resolution")
    assert os.path.exists(gen) and os.path.exists(srbin), "build() makes the tools"
    C_, H, W, s, K = 1, 48, 64, 2, 4
    rng = np.random.default_rng(21)
    gt = np.clip(0.8 * rr.prototype_ground_truth(C_, H, W) + 0.1 * rng.random((C_, H, W)), 0, 1).astype(np.float32).astype(np.float64)
    gt_cfg = _write_envi(str(tmp_path / "gt"), gt)
    fields = fr.table_fields(H, W, ar.TABLE_SHIFTS[:K])
    flow_in = tmp_path / "flow.bin"
    np.ascontiguousarray(fields, dtype="<f8").tofile(str(flow_in))
    lr_dir = tmp_path / "lr"
    lr_dir.mkdir()
    out = subprocess.run([gen, "--input_image=" + gt_cfg, "--output_image_dir=" + str(lr_dir), "--flow_motion_path=" + str(flow_in),
                          "--blur_radius=3", "--blur_sigma=1.0", "--downsampling_scale=%d" % s, "--number_of_frames=%d" % K],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    frames = np.stack([_read_envi(str(lr_dir / ("low_res_%d" % i)), (C_, H // s, W // s)) for i in range(K)]).astype(np.float64)
    base = [srbin, "--data_path=" + str(lr_dir), "--ground_truth_image=" + gt_cfg, "--upsampling_scale=%d" % s, "--blur_radius=3",
            "--blur_sigma=1.0", "--regularizer=btv", "--btv_scale_range=2", "--regularization_parameter=0.005",
            "--optimization_iterations=5", "--solver_iterations=30", "--evaluators=psnr"]

    def run(*flags):
        o = subprocess.run(base + list(flags), capture_output=True, text=True, timeout=600)
        print(o.stdout, o.stderr)
        assert o.returncode == 0
        return [float(l.split(":")[1]) for l in o.stdout.splitlines() if l.startswith("PSNR score on result")][0], o.stdout

    saved = tmp_path / "estimated_flow.bin"
    ps_flow, text = run("--registration=flow", "--save_flow_path=" + str(saved))
    assert "Estimated flow motion of 4 frames" in text
    ps_trans, _ = run("--registration=translational")
    flow, valid, _ = ctx.register_flow(frames[:, 0], hr_scale=s)
    got = np.fromfile(str(saved), dtype="<f8").reshape(K, 2, H, W)
    assert np.array_equal(got, flow)
    rflow, rvalid, _ = fq.register_flow(frames[:, 0], hr_scale=s)
    assert np.max(np.abs(flow - rflow)) <= 1e-6 and np.array_equal(valid, rvalid)
    o = orc.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = 5, 30
    x0 = rr.bilinear(frames[0], s)
    ref = orc.psnr(gt, rr.irls_solve(fr.gaussian_model(s, rflow, 3, 1.0), frames, x0, reg=(orc.REG_BTV, 0.005, 2, 0.5), options=o,
                                     composed=True, weights=rvalid[:, None])[0])
    print("CLI / restatement: %.4f / %.4f dB with the estimated flow and its masks; CLI with estimated translations %.4f dB"
          % (ps_flow, ref, ps_trans))
    assert abs(ps_flow - ref) <= 0.01
    assert ps_flow >= ps_trans + 5.0
    ps_huber, _ = run("--registration=flow", "--data_loss=huber")
    ps_file, _ = run("--flow_motion_path=" + str(saved), "--data_loss=huber")
    assert ps_huber == ps_file
    ps_unmasked, _ = run("--flow_motion_path=" + str(saved))
    print("the saved fields without the masks: %.4f dB (Huber %.4f dB)" % (ps_unmasked, ps_file))
    assert ps_flow > ps_unmasked


def test_host_facade_returns_what_the_c_call_returns(tmp_path):
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "super-resolution_amd", "lib", "flow_registration_test")
    assert os.path.exists(exe), "build() makes the facade test binary"
    o = subprocess.run([exe, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(o.stdout, o.stderr)
    assert o.returncode == 0 and "FLOW REGISTRATION FACADE TESTS PASSED" in o.stdout
