"""The command lines the two host tools refuse before they load anything (host/apps): every such `ERROR:` line of
super_resolution and generate_data in full, its exit code 1, and which refusal wins when several apply -- the order of
the checks is part of the tools' behaviour.  Plus app::Flags itself: an unknown flag and a missing required flag end with
exit code 2 and the message in front of the usage text.  CPU only: every refusal returns before a GPU context exists."""
import os
import subprocess

import pytest

BOTH = "ERROR: %s and %s exclude each other."
FLOW_FILE = "--flow_motion_path=f.bin"
FLOW_REG = "--registration=flow"
BANK_FIT = ["--fit_blur_bank_from=hr.pgm", "--fit_blur_bank_mode=frame"]

SUPER_RESOLUTION = [
    # one row per stanza, in the order of the checks
    (["--affine_motion_path=a.txt", "--motion_sequence_path=m.txt"], BOTH % ("--affine_motion_path", "--motion_sequence_path")),
    ([FLOW_FILE, "--motion_sequence_path=m.txt"], BOTH % ("--flow_motion_path", "--motion_sequence_path")),
    ([FLOW_FILE, "--affine_motion_path=a.txt"], BOTH % ("--flow_motion_path", "--affine_motion_path")),
    ([FLOW_FILE, "--registration=affine"], BOTH % ("--flow_motion_path", "--registration")),
    ([FLOW_FILE, "--refine_motion_rounds=1"], BOTH % ("--flow_motion_path", "--refine_motion_rounds")),
    ([FLOW_FILE, "--refine_motion_rounds=-1"], BOTH % ("--flow_motion_path", "--refine_motion_rounds")),
    ([FLOW_FILE, "--fit_blur_from=hr.pgm"], BOTH % ("--flow_motion_path", "--fit_blur_from")),
    ([FLOW_FILE, "--photometric_rounds=0"], BOTH % ("--flow_motion_path", "--photometric_rounds")),
    (["--registration=rigid"], "ERROR: --registration is 'translational' or 'affine', or 'flow'."),
    ([FLOW_REG, "--motion_sequence_path=m.txt"], BOTH % ("--registration=flow", "--motion_sequence_path")),
    ([FLOW_REG, "--affine_motion_path=a.txt"], BOTH % ("--registration=flow", "--affine_motion_path")),
    ([FLOW_REG, "--refine_motion_rounds=2"], BOTH % ("--registration=flow", "--refine_motion_rounds")),
    ([FLOW_REG, "--fit_blur_from=hr.pgm"], BOTH % ("--registration=flow", "--fit_blur_from")),
    ([FLOW_REG, "--photometric_rounds=1"], BOTH % ("--registration=flow", "--photometric_rounds")),
    ([FLOW_REG, "--save_motion_path=m.txt"],
     "ERROR: --save_motion_path holds matrices; the fields of --registration=flow go to --save_flow_path."),
    (["--save_flow_path=f.bin"], "ERROR: --save_flow_path needs --registration=flow."),
    (["--save_flow_path=f.bin", "--registration=affine"], "ERROR: --save_flow_path needs --registration=flow."),
    (["--flow_valid_prior"], "ERROR: --flow_valid_prior needs --registration=flow."),
    (["--registration=affine", "--motion_sequence_path=m.txt"],
     "ERROR: --registration estimates the motion; it excludes --motion_sequence_path and --affine_motion_path "
     "(except with --generate_lr_images, where the files generate the frames)."),
    (["--registration=translational", "--affine_motion_path=a.txt"],
     "ERROR: --registration estimates the motion; it excludes --motion_sequence_path and --affine_motion_path "
     "(except with --generate_lr_images, where the files generate the frames)."),
    (["--refine_motion_rounds=-1"], "ERROR: --refine_motion_rounds is >= 0 and --refine_motion_dof is 2 or 6."),
    (["--refine_motion_dof=4"], "ERROR: --refine_motion_rounds is >= 0 and --refine_motion_dof is 2 or 6."),
    (["--save_motion_path=m.txt"], "ERROR: --save_motion_path needs --registration or --refine_motion_rounds."),
    (["--fit_blur_ksize=-1"], "ERROR: --fit_blur_ksize is 0 or an odd size up to 7."),
    (["--fit_blur_ksize=4", "--fit_blur_from=hr.pgm"], "ERROR: --fit_blur_ksize is 0 or an odd size up to 7."),
    (["--fit_blur_ksize=9", "--fit_blur_from=hr.pgm"], "ERROR: --fit_blur_ksize is 0 or an odd size up to 7."),
    (["--save_blur_kernel_path=k.txt"],
     "ERROR: --save_blur_kernel_path and --fit_blur_ksize need --fit_blur_from (--fit_blur_ksize also goes with --fit_blur_bank_from)."),
    (["--save_blur_kernel_path=k.txt"] + BANK_FIT,
     "ERROR: --save_blur_kernel_path and --fit_blur_ksize need --fit_blur_from (--fit_blur_ksize also goes with --fit_blur_bank_from)."),
    (["--fit_blur_ksize=3"],
     "ERROR: --save_blur_kernel_path and --fit_blur_ksize need --fit_blur_from (--fit_blur_ksize also goes with --fit_blur_bank_from)."),
    (["--blur_bank_path=b.txt", "--blur_kernel_path=k.txt"], BOTH % ("--blur_bank_path", "--blur_kernel_path")),
    (["--blur_bank_path=b.txt", "--fit_blur_from=hr.pgm"], BOTH % ("--blur_bank_path", "--fit_blur_from")),
    (BANK_FIT + ["--blur_kernel_path=k.txt"], BOTH % ("--fit_blur_bank_from", "--blur_kernel_path")),
    (BANK_FIT + ["--fit_blur_from=hr.pgm"], BOTH % ("--fit_blur_bank_from", "--fit_blur_from")),
    (["--fit_blur_bank_mode=frame"], "ERROR: --fit_blur_bank_mode and --save_blur_bank_path need --fit_blur_bank_from."),
    (["--save_blur_bank_path=b.txt"], "ERROR: --fit_blur_bank_mode and --save_blur_bank_path need --fit_blur_bank_from."),
    (["--fit_blur_bank_from=hr.pgm"], "ERROR: --fit_blur_bank_from needs --fit_blur_bank_mode=frame|channel|frame_channel."),
    (["--fit_blur_bank_from=hr.pgm", "--fit_blur_bank_mode=both"],
     "ERROR: --fit_blur_bank_from needs --fit_blur_bank_mode=frame|channel|frame_channel."),
    (BANK_FIT + [FLOW_FILE],
     "ERROR: --fit_blur_bank_from has no sampling leg for a displacement field: not with --flow_motion_path or --registration=flow."),
    (BANK_FIT + [FLOW_REG],
     "ERROR: --fit_blur_bank_from has no sampling leg for a displacement field: not with --flow_motion_path or --registration=flow."),
    (["--photometric_rounds=-2"], "ERROR: --photometric_rounds is >= 0 (or -1: off)."),
    (["--photometric_path=p.txt", "--photometric_rounds=0"],
     "ERROR: --photometric_path gives the parameters, --photometric_rounds fits them: they exclude each other."),
    (["--save_photometric_path=p.txt"], "ERROR: --save_photometric_path needs --photometric_path or --photometric_rounds."),
    # which refusal wins when several apply
    ([FLOW_FILE, FLOW_REG], BOTH % ("--flow_motion_path", "--registration")),
    (BANK_FIT + ["--blur_kernel_path=k.txt", "--fit_blur_from=hr.pgm"], BOTH % ("--fit_blur_bank_from", "--blur_kernel_path")),
    (["--save_motion_path=m.txt", FLOW_REG],
     "ERROR: --save_motion_path holds matrices; the fields of --registration=flow go to --save_flow_path."),
    ([FLOW_FILE, "--affine_motion_path=a.txt", "--motion_sequence_path=m.txt"], BOTH % ("--affine_motion_path", "--motion_sequence_path")),
    ([FLOW_FILE, "--photometric_rounds=0", "--fit_blur_from=hr.pgm", "--refine_motion_rounds=1"],
     BOTH % ("--flow_motion_path", "--refine_motion_rounds")),
    ([FLOW_FILE, "--registration=rigid"], BOTH % ("--flow_motion_path", "--registration")),
    ([FLOW_REG, "--motion_sequence_path=m.txt", "--save_motion_path=s.txt"], BOTH % ("--registration=flow", "--motion_sequence_path")),
    ([FLOW_REG, "--photometric_rounds=0", "--fit_blur_from=hr.pgm"], BOTH % ("--registration=flow", "--fit_blur_from")),
    (["--registration=rigid", "--save_flow_path=f.bin"], "ERROR: --registration is 'translational' or 'affine', or 'flow'."),
    (["--save_flow_path=f.bin", "--flow_valid_prior"], "ERROR: --save_flow_path needs --registration=flow."),
    (["--flow_valid_prior", "--registration=affine", "--motion_sequence_path=m.txt"], "ERROR: --flow_valid_prior needs --registration=flow."),
    (["--registration=affine", "--motion_sequence_path=m.txt", "--refine_motion_dof=3"],
     "ERROR: --registration estimates the motion; it excludes --motion_sequence_path and --affine_motion_path "
     "(except with --generate_lr_images, where the files generate the frames)."),
    (["--registration=affine", "--motion_sequence_path=m.txt", "--refine_motion_dof=3", "--generate_lr_images"],
     "ERROR: --refine_motion_rounds is >= 0 and --refine_motion_dof is 2 or 6."),
    (["--refine_motion_rounds=-1", "--save_motion_path=m.txt"], "ERROR: --refine_motion_rounds is >= 0 and --refine_motion_dof is 2 or 6."),
    (["--save_motion_path=m.txt", "--fit_blur_ksize=2"], "ERROR: --save_motion_path needs --registration or --refine_motion_rounds."),
    (["--fit_blur_ksize=2", "--save_blur_kernel_path=k.txt"], "ERROR: --fit_blur_ksize is 0 or an odd size up to 7."),
    (["--save_blur_kernel_path=k.txt", "--blur_bank_path=b.txt", "--blur_kernel_path=k.txt"],
     "ERROR: --save_blur_kernel_path and --fit_blur_ksize need --fit_blur_from (--fit_blur_ksize also goes with --fit_blur_bank_from)."),
    (["--blur_bank_path=b.txt", "--fit_blur_bank_from=hr.pgm", "--fit_blur_from=hr.pgm"], BOTH % ("--blur_bank_path", "--fit_blur_from")),
    (["--blur_bank_path=b.txt", "--blur_kernel_path=k.txt", "--save_blur_bank_path=s.txt"], BOTH % ("--blur_bank_path", "--blur_kernel_path")),
    (["--save_blur_bank_path=s.txt", "--photometric_rounds=-2"], "ERROR: --fit_blur_bank_mode and --save_blur_bank_path need --fit_blur_bank_from."),
    (["--fit_blur_bank_from=hr.pgm", FLOW_FILE], "ERROR: --fit_blur_bank_from needs --fit_blur_bank_mode=frame|channel|frame_channel."),
    (BANK_FIT + [FLOW_REG, "--photometric_rounds=-2"],
     "ERROR: --fit_blur_bank_from has no sampling leg for a displacement field: not with --flow_motion_path or --registration=flow."),
    (["--photometric_rounds=-2", "--save_photometric_path=p.txt"], "ERROR: --photometric_rounds is >= 0 (or -1: off)."),
    (["--photometric_path=p.txt", "--photometric_rounds=0", "--save_photometric_path=q.txt"],
     "ERROR: --photometric_path gives the parameters, --photometric_rounds fits them: they exclude each other."),
]

GENERATE_DATA = [
    (["--blur_bank_path=b.txt", "--blur_kernel_path=k.txt"], BOTH % ("--blur_bank_path", "--blur_kernel_path")),
    (["--affine_motion_path=a.txt", "--motion_sequence_path=m.txt"], BOTH % ("--affine_motion_path", "--motion_sequence_path")),
    ([FLOW_FILE, "--motion_sequence_path=m.txt"], "ERROR: --flow_motion_path excludes --motion_sequence_path and --affine_motion_path."),
    ([FLOW_FILE, "--affine_motion_path=a.txt"], "ERROR: --flow_motion_path excludes --motion_sequence_path and --affine_motion_path."),
    # which refusal wins when several apply
    (["--affine_motion_path=a.txt", "--motion_sequence_path=m.txt", "--blur_bank_path=b.txt", "--blur_kernel_path=k.txt"],
     BOTH % ("--blur_bank_path", "--blur_kernel_path")),
    ([FLOW_FILE, "--affine_motion_path=a.txt", "--motion_sequence_path=m.txt"], BOTH % ("--affine_motion_path", "--motion_sequence_path")),
]

# the flag a tool requires, which every refused command line above carries (its file is never opened)
REQUIRED = {"super_resolution": "data_path", "generate_data": "input_image"}

REFUSALS = [("super_resolution", flags, line) for flags, line in SUPER_RESOLUTION] + \
           [("generate_data", flags, line) for flags, line in GENERATE_DATA]

# app::Flags: the message, then the usage text, exit code 2
FLAG_ERRORS = [
    ("super_resolution", ["--data_path=frames", "--no_such_flag=1"], "unknown flag --no_such_flag"),
    ("super_resolution", ["--upsampling_scale=2"], "Required argument 'data_path' is missing"),
    ("generate_data", ["--input_image=hr.pgm", "--unheard_of"], "unknown flag --unheard_of"),
    ("generate_data", ["--output_image_dir=out"], "Required argument 'input_image' is missing"),
]


@pytest.fixture(scope="module")
def apps():
    import __graft_entry__ as ge
    ge.build_lib()
    return {os.path.basename(e): e for e in ge.build_apps()}


def _run(exe, flags, cwd):
    out = subprocess.run([exe] + flags, capture_output=True, text=True, timeout=120, cwd=str(cwd))
    print(out.stdout[-2000:], out.stderr[-2000:])
    return out


@pytest.mark.parametrize("app,flags,line", REFUSALS, ids=["%s-%s" % (a, " ".join(f)) for a, f, _ in REFUSALS])
def test_refused_command_line(apps, tmp_path, app, flags, line):
    out = _run(apps[app], ["--%s=%s" % (REQUIRED[app], tmp_path / "missing")] + flags, tmp_path)
    assert out.returncode == 1
    assert out.stderr == line + "\n"
    assert out.stdout == ""


@pytest.mark.parametrize("app,flags,message", FLAG_ERRORS, ids=["%s-%s" % (a, " ".join(f)) for a, f, _ in FLAG_ERRORS])
def test_flag_errors_print_the_message_before_the_usage(apps, tmp_path, app, flags, message):
    out = _run(apps[app], flags, tmp_path)
    assert out.returncode == 2
    lines = out.stderr.splitlines()
    assert lines[0] == message
    assert lines[1].startswith(app + " --" + REQUIRED[app] + "=") and len(lines) > 2
    assert out.stdout == ""
