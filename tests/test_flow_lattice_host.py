"""Host side of the displacement field on a control lattice (tests/cpp/flow_lattice_test.cpp): the sequence file and its
round trip, the reader's aborts, FlowLatticeSequence::Expand against literals of the numpy restatement, and the flag
combinations the two tools refuse.  CPU only."""
import os
import subprocess

import pytest


def _exe():
    import __graft_entry__ as ge
    ge.build_lib()
    exe = ge.build_flow_lattice_test()
    assert exe and os.path.exists(exe)
    return exe


def test_cpp_flow_lattice_cases(tmp_path):
    out = subprocess.run([_exe(), str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "FLOW LATTICE HOST TESTS PASSED" in out.stdout


@pytest.mark.parametrize("case,message", [
    ("missing_file", "Could not open file"),
    ("bad_header", "the first line is not `step lw lh frames`"),
    ("trailing", "the first line is not `step lw lh frames`"),
    ("bad_step", "a lattice has a step of 1 ... 1024, at least 2 x 2 nodes and at least one frame"),
    ("few_nodes", "a lattice has a step of 1 ... 1024, at least 2 x 2 nodes and at least one frame"),
    ("wrong_size", "376 bytes follow the header, 2 frames of 2 x 3 x 4 float64 nodes are 384"),
    ("empty_expand", "flow lattice: the sequence is empty"),
    ("reach", "4 x 3 nodes at step 3 reach more than a cell beyond the 5 x 8 image"),
    ("shape", "48 values are no whole number of frames of 2 x 3 x 5"),
])
def test_cpp_flow_lattice_errors_abort_with_a_message(tmp_path, case, message):
    out = subprocess.run([_exe(), str(tmp_path), case], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode != 0
    assert "did not abort" not in out.stdout
    assert "Check failed" in out.stderr and message in out.stderr


def _apps():
    import __graft_entry__ as ge
    ge.build_lib()
    return {os.path.basename(e): e for e in ge.build_apps()}


def _files(tmp_path):
    f = tmp_path / "lattice.bin"
    f.write_bytes(b"4 2 2 1\n" + b"\0" * 64)
    s = tmp_path / "other.txt"
    s.write_text("0 0\n")
    return f, s


@pytest.mark.parametrize("other,message", [
    ("--motion_sequence_path=%s", "--flow_lattice_path excludes --motion_sequence_path and --affine_motion_path"),
    ("--affine_motion_path=%s", "--flow_lattice_path excludes --motion_sequence_path and --affine_motion_path"),
    ("--flow_motion_path=%s", "--flow_lattice_path and --flow_motion_path exclude each other"),
])
def test_generate_data_refuses_a_second_motion(tmp_path, other, message):
    f, s = _files(tmp_path)
    out = subprocess.run([_apps()["generate_data"], "--input_image=x.pgm", "--flow_lattice_path=%s" % f, other % s],
                         capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 1
    assert message in out.stderr


@pytest.mark.parametrize("other,name", [
    ("--motion_sequence_path=%s", "--motion_sequence_path"),
    ("--affine_motion_path=%s", "--affine_motion_path"),
    ("--registration=affine", "--registration"),
    ("--registration=translational", "--registration"),
    ("--registration=flow", "--registration"),
    ("--refine_motion_rounds=2", "--refine_motion_rounds"),
    ("--fit_blur_from=%s", "--fit_blur_from"),
    ("--photometric_rounds=0", "--photometric_rounds"),
    ("--flow_motion_path=%s", "--flow_motion_path"),
])
def test_super_resolution_refuses_what_a_lattice_excludes(tmp_path, other, name):
    f, s = _files(tmp_path)
    flag = other % s if "%s" in other else other
    out = subprocess.run([_apps()["super_resolution"], "--data_path=x", "--flow_lattice_path=%s" % f, flag],
                         capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 1
    assert "--flow_lattice_path and %s exclude each other" % name in out.stderr


@pytest.mark.parametrize("flags,message", [
    (["--flow_lattice"], "--flow_lattice needs --registration=flow"),
    (["--registration=affine", "--flow_lattice"], "--flow_lattice needs --registration=flow"),
    (["--save_flow_lattice_path=x.bin"], "--save_flow_lattice_path needs --registration=flow --flow_lattice"),
    (["--registration=flow", "--save_flow_lattice_path=x.bin"], "--save_flow_lattice_path needs --registration=flow --flow_lattice"),
    (["--registration=flow", "--flow_lattice", "--fit_blur_bank_from=x", "--fit_blur_bank_mode=frame"],
     "--fit_blur_bank_from has no sampling leg for a displacement field"),
])
def test_super_resolution_refuses_the_lattice_flags_without_their_registration(flags, message):
    out = subprocess.run([_apps()["super_resolution"], "--data_path=x"] + flags, capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 1
    assert message in out.stderr
