"""Host side of the dense flow registration (tests/cpp/flow_registration_test.cpp): the empty list, the file
--save_flow_path writes, the calls that abort before any device call, and the flag combinations super_resolution refuses
for --registration=flow and --save_flow_path.  CPU only."""
import os
import subprocess

import pytest


def _exe():
    import __graft_entry__ as ge
    ge.build_lib()
    exe = ge.build_flow_registration_test()
    assert exe and os.path.exists(exe)
    return exe


def test_cpp_flow_registration_cases(tmp_path):
    out = subprocess.run([_exe(), str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "FLOW REGISTRATION HOST TESTS PASSED" in out.stdout


@pytest.mark.parametrize("case,message", [
    ("scale", "flow registration: the scale must be at least 1"),
    ("sizes", "registration needs images of one size with at least one channel"),
    ("no_channel", "registration needs images of one size with at least one channel"),
    ("few_initial", "flow registration: fewer initial matrices than images"),
])
def test_cpp_flow_registration_errors_abort_with_a_message(tmp_path, case, message):
    out = subprocess.run([_exe(), str(tmp_path), case], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode != 0
    assert "did not abort" not in out.stdout
    assert "Check failed" in out.stderr and message in out.stderr


def _super_resolution():
    import __graft_entry__ as ge
    ge.build_lib()
    return {os.path.basename(e): e for e in ge.build_apps()}["super_resolution"]


@pytest.mark.parametrize("other,name", [
    ("--motion_sequence_path=%s", "--motion_sequence_path"),
    ("--affine_motion_path=%s", "--affine_motion_path"),
    ("--refine_motion_rounds=2", "--refine_motion_rounds"),
    ("--fit_blur_from=%s", "--fit_blur_from"),
    ("--photometric_rounds=0", "--photometric_rounds"),
])
@pytest.mark.parametrize("generate", [False, True])
def test_super_resolution_refuses_what_a_flow_registration_excludes(tmp_path, other, name, generate):
    s = tmp_path / "other.txt"
    s.write_text("0 0\n")
    flag = other % s if "%s" in other else other
    out = subprocess.run([_super_resolution(), "--data_path=x", "--registration=flow", flag] + (["--generate_lr_images"] if generate else []),
                         capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 1
    assert "--registration=flow and %s exclude each other" % name in out.stderr


def test_super_resolution_flow_flags_that_need_each_other(tmp_path):
    exe = _super_resolution()
    f = tmp_path / "flow.bin"
    f.write_bytes(b"\0" * 64)
    cases = [
        (["--flow_motion_path=%s" % f, "--registration=flow"], "--flow_motion_path and --registration exclude each other"),
        (["--save_flow_path=%s" % f], "--save_flow_path needs --registration=flow"),
        (["--save_flow_path=%s" % f, "--registration=affine"], "--save_flow_path needs --registration=flow"),
        (["--registration=flow", "--save_motion_path=%s" % f], "go to --save_flow_path"),
        (["--registration=dense"], "--registration is 'translational' or 'affine', or 'flow'"),
    ]
    for flags, message in cases:
        out = subprocess.run([exe, "--data_path=x"] + flags, capture_output=True, text=True, timeout=120)
        print(out.stdout[-2000:], out.stderr[-2000:])
        assert out.returncode == 1 and message in out.stderr, flags
    # the help text names the new flags
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    text = out.stdout + out.stderr
    assert "--registration=translational|affine|flow" in text and "--save_flow_path" in text
