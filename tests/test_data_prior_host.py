"""Host side of the persistent data prior: the flag combinations super_resolution refuses for --flow_valid_prior and its
help text.  CPU only; the facade (IRLSMapSolver::SetDataPrior, RegisterFlow) needs a problem on a device and is run by
tests/test_gpu_data_prior.py through tests/cpp/data_prior_test.cpp."""
import os
import subprocess

import pytest


def _super_resolution():
    import __graft_entry__ as ge
    ge.build_lib()
    return {os.path.basename(e): e for e in ge.build_apps()}["super_resolution"]


@pytest.mark.parametrize("flags", [[], ["--registration=affine"], ["--registration=translational"], ["--data_loss=huber"]])
def test_super_resolution_refuses_the_prior_without_a_flow_registration(flags):
    out = subprocess.run([_super_resolution(), "--data_path=x", "--flow_valid_prior"] + flags, capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 1
    assert "--flow_valid_prior needs --registration=flow" in out.stderr


def test_the_flag_is_known_and_the_help_text_names_it(tmp_path):
    exe = _super_resolution()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    text = out.stdout + out.stderr
    assert "--flow_valid_prior" in text and "--data_loss=huber" in text
    # with --registration=flow the flag passes the flag checks: the run ends at the missing data, not at the flags
    out = subprocess.run([exe, "--data_path=%s" % (tmp_path / "none"), "--registration=flow", "--flow_valid_prior"],
                         capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert "--flow_valid_prior needs" not in out.stderr and "nknown" not in out.stderr.split("\n")[0]


def test_the_facade_test_program_builds():
    import __graft_entry__ as ge
    ge.build_lib()
    exe = ge.build_data_prior_test()
    assert exe and os.path.exists(exe)
