"""Host side of the affine motion model (tests/cpp/affine_motion_test.cpp): the sequence file format, index errors, the
error for a model given both kinds of motion, and ImageModel::Canonical() carrying the matrices.  CPU only."""
import os
import subprocess

import pytest


def _exe():
    import __graft_entry__ as ge
    ge.build_lib()
    exe = ge.build_affine_motion_test()
    assert exe and os.path.exists(exe)
    return exe


def test_cpp_affine_motion_cases(tmp_path):
    out = subprocess.run([_exe(), str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "AFFINE MOTION HOST TESTS PASSED" in out.stdout


@pytest.mark.parametrize("case,message", [
    ("index", "affine motion index out of range"),
    ("both", "both an affine motion sequence and a motion shift sequence were given"),
    ("short_line", "line 2: expected six numbers"),
    ("missing_file", "Could not open file"),
])
def test_cpp_affine_motion_errors_abort_with_a_message(tmp_path, case, message):
    out = subprocess.run([_exe(), str(tmp_path), case], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode != 0
    assert "did not abort" not in out.stdout
    assert "Check failed" in out.stderr and message in out.stderr


@pytest.mark.parametrize("app", ["generate_data", "super_resolution"])
def test_apps_refuse_both_motion_flags(tmp_path, app):
    import __graft_entry__ as ge
    ge.build_lib()
    exes = {os.path.basename(e): e for e in ge.build_apps()}
    a = tmp_path / "affine.txt"
    a.write_text("1 0 0 0 1 0\n")
    s = tmp_path / "shifts.txt"
    s.write_text("0 0\n")
    first = "--input_image=x.pgm" if app == "generate_data" else "--data_path=x"
    out = subprocess.run([exes[app], first, "--affine_motion_path=%s" % a, "--motion_sequence_path=%s" % s],
                         capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 1
    assert "--affine_motion_path and --motion_sequence_path exclude each other" in out.stderr
