"""The host side of the regularisers' gradient mode without a GPU: the mode words of --regularizer_gradient and the
dispatch rule of k_btv_gradient_exact4 (csrc/reg_gradient_host.hpp) through tests/cpp/reg_exact_facade_test.cpp, the
exported entry points, and the command line's refusal of an unknown word before any GPU work."""
import os
import subprocess

from conftest import ROOT

LIBDIR = os.path.join(ROOT, "super-resolution_amd", "lib")


def test_mode_words_and_dispatch_rule():
    import __graft_entry__ as ge
    ge.build_lib()
    exe = ge.build_reg_exact_facade_test()
    o = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(o.stdout, o.stderr)
    assert o.returncode == 0 and "REG EXACT FACADE TESTS PASSED" in o.stdout


def test_entry_points_and_constants():
    import __graft_entry__ as ge
    ge.build_lib()
    import srmap
    lib = srmap.load()
    for name in ("srmap_problem_set_regularizer_gradient", "srmap_problem_get_regularizer_gradient"):
        assert hasattr(lib, name) and name in srmap.EXPORTED_SYMBOLS
    assert (srmap.REG_GRADIENT_REFERENCE, srmap.REG_GRADIENT_EXACT) == (0, 1)
    # a null problem is refused without touching a device
    assert lib.srmap_problem_set_regularizer_gradient(None, 0, 1) == srmap.EINVAL
    assert lib.srmap_problem_get_regularizer_gradient(None, 0, None) == srmap.EINVAL


def test_command_line_refuses_an_unknown_word(tmp_path):
    import __graft_entry__ as ge
    ge.build_lib()
    _, srbin = ge.build_apps()
    for word in ("Exact", "true", "exact,reference"):
        o = subprocess.run([srbin, "--data_path=" + str(tmp_path), "--regularizer_gradient=" + word], capture_output=True, text=True,
                           timeout=60)
        assert o.returncode != 0 and "--regularizer_gradient is reference or exact" in (o.stdout + o.stderr), (word, o.stdout, o.stderr)
