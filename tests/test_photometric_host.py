"""Host side of the photometric frame model (tests/cpp/photometric_test.cpp): the 'gain bias' file format and its round
trip, the errors of the reader, the plain-C++ per-frame solve against closed forms with its statuses, and the flag
combinations super_resolution refuses.  CPU only."""
import os
import subprocess

import pytest


def _exe():
    import __graft_entry__ as ge
    ge.build_lib()
    exe = ge.build_photometric_test()
    assert exe and os.path.exists(exe)
    return exe


def test_cpp_photometric_cases(tmp_path):
    out = subprocess.run([_exe(), str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "PHOTOMETRIC HOST TESTS PASSED" in out.stdout


@pytest.mark.parametrize("case,message", [
    ("short_line", "short.txt line 2: expected two numbers 'gain bias'"),
    ("long_line", "long.txt line 1: expected two numbers 'gain bias'"),
    ("not_a_number", "nan.txt line 1: expected two numbers 'gain bias'"),
    ("bad_gain", "bad.txt line 3: the gain must be > 0 and both numbers finite"),
    ("missing_file", "Could not open file"),
    ("index", "photometric index out of range"),
])
def test_cpp_photometric_errors_abort_with_a_message(tmp_path, case, message):
    out = subprocess.run([_exe(), str(tmp_path), case], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode != 0
    assert "did not abort" not in out.stdout
    assert "Check failed" in out.stderr and message in out.stderr


@pytest.mark.parametrize("flags,message", [
    (["--save_photometric_path=p.txt"], "--save_photometric_path needs --photometric_path or --photometric_rounds"),
    (["--photometric_path=p.txt", "--photometric_rounds=3"], "they exclude each other"),
    (["--photometric_path=p.txt", "--photometric_rounds=0", "--save_photometric_path=q.txt"], "they exclude each other"),
    (["--photometric_rounds=-2"], "--photometric_rounds is >= 0"),
])
def test_super_resolution_refuses_bad_photometric_flags(tmp_path, flags, message):
    import __graft_entry__ as ge
    ge.build_lib()
    exes = {os.path.basename(e): e for e in ge.build_apps()}
    out = subprocess.run([exes["super_resolution"], "--data_path=" + str(tmp_path)] + flags, capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 1 and message in out.stderr
