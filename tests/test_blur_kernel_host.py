"""Host side of the free-form blur kernel (tests/cpp/blur_kernel_test.cpp): the kernel file format and its round trip, the
errors of the reader, and ImageModel::Canonical() carrying the taps.  CPU only."""
import os
import subprocess

import pytest


def _exe():
    import __graft_entry__ as ge
    ge.build_lib()
    exe = ge.build_blur_kernel_test()
    assert exe and os.path.exists(exe)
    return exe


def test_cpp_blur_kernel_cases(tmp_path):
    out = subprocess.run([_exe(), str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "BLUR KERNEL HOST TESTS PASSED" in out.stdout


@pytest.mark.parametrize("case,message", [
    ("even_size", "expected an odd kernel size first"),
    ("short_file", "expected 9 taps after the size, read 8"),
    ("long_file", "more than 1 taps after the size"),
    ("missing_file", "Could not open file"),
    ("empty_module", "the blur kernel is empty"),
    ("index", "blur kernel index out of range"),
])
def test_cpp_blur_kernel_errors_abort_with_a_message(tmp_path, case, message):
    out = subprocess.run([_exe(), str(tmp_path), case], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode != 0
    assert "did not abort" not in out.stdout
    assert "Check failed" in out.stderr and message in out.stderr


@pytest.mark.parametrize("flags,message", [
    (["--fit_blur_ksize=4", "--fit_blur_from=x.pgm"], "--fit_blur_ksize is 0 or an odd size up to 7"),
    (["--fit_blur_ksize=9", "--fit_blur_from=x.pgm"], "--fit_blur_ksize is 0 or an odd size up to 7"),
    (["--save_blur_kernel_path=k.txt"], "need --fit_blur_from"),
    (["--fit_blur_ksize=5"], "need --fit_blur_from"),
])
def test_super_resolution_refuses_bad_blur_flags(tmp_path, flags, message):
    import __graft_entry__ as ge
    ge.build_lib()
    exes = {os.path.basename(e): e for e in ge.build_apps()}
    out = subprocess.run([exes["super_resolution"], "--data_path=" + str(tmp_path)] + flags, capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 1 and message in out.stderr
