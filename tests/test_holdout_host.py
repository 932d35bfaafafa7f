"""The host arithmetic of hold-out validation (csrc/holdout_host.hpp: the index hash, the threshold of a fraction, the chosen
row and the early stop of the lambda path) in plain C++ against literals: tests/cpp/holdout_test.cpp, which includes that
header alone and links nothing of the library.  No GPU.  The same program compared with the numpy restatement:
tests/test_holdout_cpu.py."""
import subprocess


def _exe():
    import __graft_entry__ as ge
    exe = ge.build_holdout_test()
    assert exe, "tests/cpp/holdout_test.cpp is missing"
    return exe


def test_the_literals_hold_in_plain_cpp():
    r = subprocess.run([_exe()], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def test_the_modes_of_the_program():
    exe = _exe()
    out = subprocess.run([exe, "mask", "35", "0.5", "3"], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["8388608", "10000110011010100111101110110000111"]
    assert subprocess.run([exe, "choose", "3", "1", "1", "nan"], capture_output=True, text=True, check=True).stdout.strip() == "1"
    assert subprocess.run([exe, "stop", "2", "5", "4", "4.5", "4.6", "4.7"], capture_output=True, text=True, check=True).stdout.strip() == "00011"
    assert subprocess.run([exe, "nonsense"], capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe, "triple", "0.08:0.5:8"], capture_output=True, text=True, check=True).stdout.split() == ["0.080000000000000002", "0.5", "8"]
    for bad in ("0.08:0.5", "0.08:1:8", "0:0.5:8", "0.08:0.5:33", "0.08:0.5:8x", ""):
        assert subprocess.run([exe, "triple", bad], capture_output=True, text=True, check=True).stdout.strip() == "refused", bad


def test_the_tool_refuses_bad_flags_before_any_gpu_work(tmp_path):
    """super_resolution answers a malformed --lambda_path, one without --holdout_fraction and a fraction outside (0, 0.5] with
    a message and exit status 1 before it loads a frame or touches a GPU: the data path does not even exist."""
    import os
    import __graft_entry__ as ge
    tools = {os.path.basename(t): t for t in ge.build_apps()}
    srbin = tools["super_resolution"]
    for flags, word in ((["--lambda_path=0.08:0.5:4"], "--lambda_path needs --holdout_fraction."),
                        (["--holdout_fraction=0.1", "--lambda_path=0.08:0.5"], "--lambda_path is <largest>:<ratio>:<count>"),
                        (["--holdout_fraction=0.1", "--lambda_path=0.08:1.0:4"], "--lambda_path is <largest>:<ratio>:<count>"),
                        (["--holdout_fraction=0.1", "--lambda_path=0.08:0.5:40"], "--lambda_path is <largest>:<ratio>:<count>"),
                        (["--holdout_fraction=0.7"], "--holdout_fraction is in (0, 0.5]."),
                        (["--holdout_fraction=-0.1"], "--holdout_fraction is in (0, 0.5]."),
                        (["--holdout_fraction=0.1", "--lambda_path=0.08:0.5:4", "--lambda_patience=-1"], "--lambda_patience is >= 0."),
                        (["--holdout_fraction=0.1", "--holdout_seed=abc"], "--holdout_seed is a non-negative integer"),
                        (["--holdout_fraction=0.1", "--holdout_seed=-1"], "--holdout_seed is a non-negative integer"),
                        (["--holdout_fraction=0.1", "--holdout_seed=1.5"], "--holdout_seed is a non-negative integer"),
                        (["--holdout_fraction=0.1", "--holdout_seed=12345678901234567890"], "--holdout_seed is a non-negative integer"),
                        (["--holdout_seed=3"], "--holdout_seed needs --holdout_fraction."),
                        (["--print_lambda_path"], "need --lambda_path."),
                        (["--lambda_patience=2"], "need --lambda_path."),
                        (["--holdout_fraction=0.1", "--lambda_path=0.08:0.5:4", "--refine_motion_rounds=1"], "runs plain solves")):
        o = subprocess.run([srbin, "--data_path=" + str(tmp_path / "nothing")] + flags, capture_output=True, text=True, timeout=60)
        assert o.returncode == 1 and word in o.stderr, (flags, o.stdout, o.stderr)
