"""Host side of the displacement-field motion model (tests/cpp/flow_motion_test.cpp): the raw sequence file and its size
check, index errors, the error for a model given two kinds of motion, ImageModel::Canonical() carrying the field, and the
flag combinations the two tools refuse.  CPU only."""
import os
import subprocess

import pytest


def _exe():
    import __graft_entry__ as ge
    ge.build_lib()
    exe = ge.build_flow_motion_test()
    assert exe and os.path.exists(exe)
    return exe


def test_cpp_flow_motion_cases(tmp_path):
    out = subprocess.run([_exe(), str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "FLOW MOTION HOST TESTS PASSED" in out.stdout


@pytest.mark.parametrize("case,message", [
    ("index", "flow motion index out of range"),
    ("pixel", "flow motion pixel out of range"),
    ("both", "a flow motion sequence and another motion sequence were given"),
    ("wrong_size", "760 bytes are no whole number of frames of 2 x 4 x 6 float64 values (384 bytes each)"),
    ("empty_file", "0 bytes are no whole number of frames"),
    ("missing_file", "Could not open file"),
    ("wrong_geometry", "the flow motion is given for a 6 x 4 high-resolution image, the model is applied at 8 x 4"),
])
def test_cpp_flow_motion_errors_abort_with_a_message(tmp_path, case, message):
    out = subprocess.run([_exe(), str(tmp_path), case], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode != 0
    assert "did not abort" not in out.stdout
    assert "Check failed" in out.stderr and message in out.stderr


def _apps():
    import __graft_entry__ as ge
    ge.build_lib()
    return {os.path.basename(e): e for e in ge.build_apps()}


@pytest.mark.parametrize("other", ["--motion_sequence_path=%s", "--affine_motion_path=%s"])
def test_generate_data_refuses_a_second_motion(tmp_path, other):
    f = tmp_path / "flow.bin"
    f.write_bytes(b"\0" * 64)
    s = tmp_path / "other.txt"
    s.write_text("0 0\n")
    out = subprocess.run([_apps()["generate_data"], "--input_image=x.pgm", "--flow_motion_path=%s" % f, other % s],
                         capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 1
    assert "--flow_motion_path excludes --motion_sequence_path and --affine_motion_path" in out.stderr


@pytest.mark.parametrize("other,name", [
    ("--motion_sequence_path=%s", "--motion_sequence_path"),
    ("--affine_motion_path=%s", "--affine_motion_path"),
    ("--registration=affine", "--registration"),
    ("--registration=translational", "--registration"),
    ("--refine_motion_rounds=2", "--refine_motion_rounds"),
    ("--fit_blur_from=%s", "--fit_blur_from"),
    ("--photometric_rounds=0", "--photometric_rounds"),
])
def test_super_resolution_refuses_what_a_flow_excludes(tmp_path, other, name):
    f = tmp_path / "flow.bin"
    f.write_bytes(b"\0" * 64)
    s = tmp_path / "other.txt"
    s.write_text("0 0\n")
    flag = other % s if "%s" in other else other
    out = subprocess.run([_apps()["super_resolution"], "--data_path=x", "--flow_motion_path=%s" % f, flag],
                         capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 1
    assert "--flow_motion_path and %s exclude each other" % name in out.stderr
