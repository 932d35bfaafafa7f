"""Host side of the blur-kernel bank (tests/cpp/blur_bank_test.cpp): the bank file format and its round trip, the errors of
the reader, ImageModel::Canonical() carrying the bank, and the flag combinations the two tools refuse.  CPU only."""
import os
import subprocess

import pytest


def _exe():
    import __graft_entry__ as ge
    ge.build_lib()
    exe = ge.build_blur_bank_test()
    assert exe and os.path.exists(exe)
    return exe


def test_cpp_blur_bank_cases(tmp_path):
    out = subprocess.run([_exe(), str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "BLUR BANK HOST TESTS PASSED" in out.stdout


@pytest.mark.parametrize("case,message", [
    ("bad_mode", "expected the bank mode 1, 2 or 3 first"),
    ("even_size", "expected an odd kernel size after the mode"),
    ("no_entries", "expected the number of entries after the size"),
    ("short_file", "expected 18 taps after the header, read 12"),
    ("long_file", "more than 2 taps after the header"),
    ("missing_file", "Could not open file"),
    ("empty_module", "the blur bank is empty"),
    ("entry", "blur bank entry out of range"),
    ("both_blurs", "both a blur bank and a blur kernel were given"),
])
def test_cpp_blur_bank_errors_abort_with_a_message(tmp_path, case, message):
    out = subprocess.run([_exe(), str(tmp_path), case], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode != 0
    assert "did not abort" not in out.stdout
    assert "Check failed" in out.stderr and message in out.stderr


@pytest.mark.parametrize("flags,message", [
    (["--blur_bank_path=b.txt", "--blur_kernel_path=k.txt"], "--blur_bank_path and --blur_kernel_path exclude each other"),
    (["--blur_bank_path=b.txt", "--fit_blur_from=x.pgm"], "--blur_bank_path and --fit_blur_from exclude each other"),
    (["--fit_blur_bank_from=x.pgm", "--fit_blur_bank_mode=frame", "--blur_kernel_path=k.txt"], "--fit_blur_bank_from and --blur_kernel_path exclude each other"),
    (["--fit_blur_bank_from=x.pgm", "--fit_blur_bank_mode=frame", "--fit_blur_from=x.pgm"], "--fit_blur_bank_from and --fit_blur_from exclude each other"),
    (["--fit_blur_bank_from=x.pgm"], "needs --fit_blur_bank_mode=frame|channel|frame_channel"),
    (["--fit_blur_bank_from=x.pgm", "--fit_blur_bank_mode=band"], "needs --fit_blur_bank_mode=frame|channel|frame_channel"),
    (["--fit_blur_bank_mode=frame"], "need --fit_blur_bank_from"),
    (["--save_blur_bank_path=b.txt"], "need --fit_blur_bank_from"),
    (["--fit_blur_bank_from=x.pgm", "--fit_blur_bank_mode=frame", "--fit_blur_ksize=4"], "--fit_blur_ksize is 0 or an odd size up to 7"),
    (["--fit_blur_bank_from=x.pgm", "--fit_blur_bank_mode=channel", "--registration=flow"], "no sampling leg for a displacement field"),
])
def test_super_resolution_refuses_bad_bank_flags(tmp_path, flags, message):
    import __graft_entry__ as ge
    ge.build_lib()
    exes = {os.path.basename(e): e for e in ge.build_apps()}
    out = subprocess.run([exes["super_resolution"], "--data_path=" + str(tmp_path)] + flags, capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 1 and message in out.stderr


def test_generate_data_refuses_a_bank_with_a_kernel(tmp_path):
    import __graft_entry__ as ge
    ge.build_lib()
    exes = {os.path.basename(e): e for e in ge.build_apps()}
    out = subprocess.run([exes["generate_data"], "--input_image=x.pgm", "--blur_bank_path=b.txt", "--blur_kernel_path=k.txt"],
                         capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 1 and "--blur_bank_path and --blur_kernel_path exclude each other" in out.stderr
