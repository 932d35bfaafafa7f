"""The blur-kernel bank through the host facade and the two command-line tools, on the GPU: tests/cpp/blur_bank_test.cpp
`gpu` (the model over a bank, IRLSMapSolver::SetBlurBank / FitBlurBank against the C calls, bit for bit) and generate_data /
super_resolution end to end on a 48 x 64, four-frame burst whose frames carry different blurs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blur_bank_restatement as bb  # noqa: E402
import blur_kernel_restatement as bk  # noqa: E402
import robust_restatement as rr  # noqa: E402

pytestmark = pytest.mark.gpu

LIBDIR = os.path.join(ROOT, "super-resolution_amd", "lib")


def test_host_facade_returns_what_the_c_calls_return(tmp_path):
    exe = os.path.join(LIBDIR, "blur_bank_test")
    assert os.path.exists(exe), "build() makes the facade test binary"
    o = subprocess.run([exe, str(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(o.stdout, o.stderr)
    assert o.returncode == 0 and "BLUR BANK FACADE TESTS PASSED" in o.stdout


def test_cli_blur_bank_flags(tmp_path):
    """generate_data --blur_bank_path makes the frames the library makes with that bank; super_resolution
    --fit_blur_bank_from on those frames, started from the guessed Gaussian, saves a bank that matches the generating one
    (up to the float32 files) and ends above the same run without the fit; the saved file drives a run as --blur_bank_path."""
    import srmap
    from test_gpu_apps import _read_envi, _write_envi
    gen, srbin = os.path.join(LIBDIR, "generate_data"), os.path.join(LIBDIR, "super_resolution")
    assert os.path.exists(gen) and os.path.exists(srbin), "build() makes the tools"
    C_, H, W, s, K = 1, 48, 64, 2, 4
    rng = np.random.default_rng(21)
    gt = np.clip(rr.prototype_ground_truth(C_, H, W) + 0.1 * rng.random((C_, H, W)), 0, 1).astype(np.float32).astype(np.float64)
    gt_cfg = _write_envi(str(tmp_path / "gt"), gt)
    bank = np.stack([bb.pad(bk.gaussian_taps(3, 1.0), 5), bb.streak(0), bk.anisotropic_psf(), bb.streak(45)])
    bfile = tmp_path / "bank.txt"
    bfile.write_text("1 5 %d\n" % K + "".join(" ".join(repr(float(v)) for v in row) + "\n" for e in bank for row in e))
    shifts = [[0, 0], [1.25, .75], [.5, 1], [1, .25]]
    motion = tmp_path / "motion.txt"
    motion.write_text("".join("%r %r\n" % (float(a), float(b)) for a, b in shifts))
    lr_dir = tmp_path / "lr"
    lr_dir.mkdir()
    out = subprocess.run([gen, "--input_image=" + gt_cfg, "--output_image_dir=" + str(lr_dir), "--motion_sequence_path=" + str(motion),
                          "--blur_bank_path=" + str(bfile), "--downsampling_scale=%d" % s, "--number_of_frames=%d" % K],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    frames = np.stack([_read_envi(str(lr_dir / ("low_res_%d" % i)), (C_, H // s, W // s)) for i in range(K)])
    p = srmap.Problem(srmap.Context(0), W, H, C_, K, s, shifts, 0, 0.0, srmap.F64)
    p.set_blur_bank(bank, srmap.BLUR_PER_FRAME)
    for k in range(K):
        assert np.allclose(frames[k], p.apply(gt, k), atol=2e-7)
    base = [srbin, "--data_path=" + str(lr_dir), "--ground_truth_image=" + gt_cfg, "--upsampling_scale=%d" % s,
            "--motion_sequence_path=" + str(motion), "--regularizer=btv", "--btv_scale_range=2", "--regularization_parameter=0.001",
            "--optimization_iterations=5", "--solver_iterations=30", "--evaluators=psnr"]

    def run(*flags):
        o = subprocess.run(base + list(flags), capture_output=True, text=True, timeout=600)
        print(o.stdout, o.stderr)
        assert o.returncode == 0
        return [float(l.split(":")[1]) for l in o.stdout.splitlines() if l.startswith("PSNR score on result")][0], o.stdout

    saved = tmp_path / "fitted.txt"
    ps_guess, _ = run("--blur_radius=3", "--blur_sigma=1.0")
    ps_fit, text = run("--blur_radius=3", "--blur_sigma=1.0", "--fit_blur_bank_from=" + gt_cfg, "--fit_blur_bank_mode=frame",
                       "--fit_blur_ksize=5", "--save_blur_bank_path=" + str(saved))
    assert "Fitted a bank of 4 5 x 5 blur kernels (mode frame): 0 degenerate" in text
    vals = [float(v) for v in saved.read_text().split()]
    assert vals[:3] == [1, 5, K] and len(vals) == 3 + K * 25
    err = float(np.max(np.abs(np.array(vals[3:]).reshape(K, 5, 5) - bank)))
    ps_file, _ = run("--blur_bank_path=" + str(saved))
    print("CLI: %.3f dB with the guessed Gaussian, %.3f dB with --fit_blur_bank_from (largest tap error %.2e), %.3f dB from the saved bank"
          % (ps_guess, ps_fit, err, ps_file))
    # the frames are float32 files of noise-free frames: the single-kernel tool test's bars (tests/test_gpu_blur_kernel.py)
    assert err <= 1e-3 and ps_fit > ps_guess + 0.5 and abs(ps_file - ps_fit) <= 1e-6
