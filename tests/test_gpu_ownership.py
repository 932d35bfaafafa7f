"""Device-memory ownership (csrc/dev_mem.hpp): srmap_live_allocations() around create / evaluate / destroy, every model
setter as set -> refused -> cleared, every motion and blur replaced by another and then cleared, re-plan churn, and
every call with scratch of its own.

The counts are read in ONE fresh child process (tests/ownership_worker.py, which lists the scenarios): in the pytest
process they depend on when Python collects the problems of other tests.  Every test here reads the record of its
scenario; a scenario asserts only equalities of counts, so there is no tolerance to choose.
"""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

# The worker takes 2.3 s on an MI355X, most of it the start of torch and of the HIP runtime
# (profiles/r17_device_ownership.txt); the limit leaves room for the start of a process on a busy machine.
WORKER_LIMIT_S = 60

DT = ("f64", "f32")
SCENARIOS = (
    ["create_eval_destroy[%s,%s]" % (k, t) for t in DT for k in ("integer", "subpixel", "rounding_tie", "direct")]
    + ["setter[%s,%s]" % (k, t) for t in DT
       for k in ("affine", "flow", "blur", "photometric", "prior_then_weights", "huber_then_prior")]
    + ["replacement[%s,%s]" % (k, t) for t in DT for k in ("motion", "blur")]
    + ["churn[%s,%s]" % (k, t) for t in DT for k in ("regularizers", "data_loss")]
    + ["scratch[%s,%s]" % (k, t) for t in DT
       for k in ("solve_cg", "solve_lbfgs", "solve_split_channels", "cg_trace", "lbfgs_trace", "fit_blur", "fit_photometric",
                 "refine_motion", "fit_blur_refused_under_flow", "fit_photometric_refused_under_flow", "register_flow_problem")]
    + ["scratch[%s]" % k for k in ("register_translational", "register_affine", "register_flow_host",
                                   "register_flow_host_single_image", "register_flow_device",
                                   "register_flow_device_single_image", "register_flow_device_non_finite_pixel",
                                   "channel_map", "pca")]
    + ["end"])


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ownership") / "results.jsonl")
    worker = os.path.join(ROOT, "tests", "ownership_worker.py")
    try:
        done = subprocess.run([sys.executable, worker, out], capture_output=True, text=True, timeout=WORKER_LIMIT_S)
        log = "exit code %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    except subprocess.TimeoutExpired:
        log = "the worker did not finish within %d s" % WORKER_LIMIT_S
    recs = {}
    if os.path.exists(out):
        with open(out) as f:
            for line in f:
                r = json.loads(line)
                recs[r["name"]] = r
    return recs, log


@pytest.mark.parametrize("name", SCENARIOS)
def test_live_allocations(records, name):
    recs, log = records
    assert "worker" not in recs, recs["worker"]["error"]
    assert name in recs, "no record of this scenario: %s" % log
    wrong = [c for c in recs[name]["checks"] if c[1] != c[2]]
    assert not wrong, "[label, got, want]: %s" % wrong
