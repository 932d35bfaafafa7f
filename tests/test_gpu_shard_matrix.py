"""The sharded evaluation and the sharded solve (srmap_eval_sharded_device, srmap_solve_sharded: csrc/shard_eval.hip,
csrc/comm.hip) over 2, 3, 4 and 6 ranks on ONE GPU, against the CPU oracle of the whole problem: ranks with neighbours on
both sides, uneven row bands / channel blocks / frame shards, the regulariser's clipped and empty band of frame mode,
f32 halos and gradients, sub-pixel shifts and the rounding-tie refusal of row mode, term subsets and optional outputs,
reg_rank != 0, and the overlap decision at a halo of exactly the tile kernel's reach and below it.

tests/shard_matrix.py is the case table, tests/shard_matrix_worker.py one rank.  A launch starts its ranks once and runs
all cases of its world over one communicator; every test reads the record of its case.
"""
import json
import os
import socket
import subprocess
import sys
import time

import pytest

import shard_matrix as sm
from conftest import ROOT
from parity_log import note

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-12, "f32": 2e-5}  # test_gpu_bands.py's; a band is tiled at another alignment than the whole image, so
BAR = 10                           # the summation order differs: 10 x, as there

# Wall time of every launch on an MI355X (profiles/shard_matrix.txt), ranks sharing the GPU, start of the processes and
# of the communicator included:
#   host, 2 ranks 2.9 s    host, 3 ranks 2.8 s    host, 4 ranks 3.0 s    host, 6 ranks 3.4 s    rccl, 3 ranks 6.6 s
# The limit is four times the slowest (26.4 s), rounded up to the next 30 s: process start and RCCL's socket set-up vary
# by that much on a busy machine.  (The first runs had the existing test's 300 s.)
LAUNCH_LIMIT_S = 30

_state = {"hung": None}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _launch(backend, world, outdir):
    """Starts the ranks once and waits for them.  The first rank that exits non-zero, or the time limit, ends all of
    them; nothing is started again.  Returns {"error": text} or the parsed results."""
    if _state["hung"]:
        return {"error": "an earlier launch hung (%s): this one was not started" % _state["hung"]}
    os.makedirs(outdir)
    port = _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    worker = os.path.join(ROOT, "tests", "shard_matrix_worker.py")
    outs = [open(os.path.join(outdir, "rank%d.log" % r), "w") for r in range(world)]
    t0 = time.monotonic()
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(port), backend, outdir], env=env,
                              stdout=outs[r], stderr=subprocess.STDOUT) for r in range(world)]
    why = None
    while why is None:
        codes = [p.poll() for p in procs]
        if all(c is not None for c in codes):
            break
        if any(c not in (None, 0) for c in codes):
            why = "a rank exited with %s" % [c for c in codes if c not in (None, 0)]
        elif time.monotonic() - t0 > LAUNCH_LIMIT_S:
            why = "time limit of %d s" % LAUNCH_LIMIT_S
            _state["hung"] = "%s, %d ranks: %s" % (backend, world, why)
        else:
            time.sleep(0.05)
    codes = [p.poll() for p in procs]  # before the others are ended
    for p in procs:
        if p.poll() is None:
            p.kill()
    for p, o in zip(procs, outs):
        p.wait()
        o.close()
    wall = time.monotonic() - t0
    if any(c is not None and c < 0 for c in codes):
        _state["hung"] = "%s, %d ranks: a rank was ended by signal %s" % (backend, world, [-c for c in codes if c is not None and c < 0])
    logs = [open(os.path.join(outdir, "rank%d.log" % r)).read() for r in range(world)]
    text = "\n".join("---- rank %d (exit %s)\n%s" % (r, codes[r], logs[r][-3000:]) for r in range(world))
    if why is None and all(c == 0 for c in codes):
        with open(os.path.join(outdir, "results.json")) as f:
            res = json.load(f)
        res["wall_s"] = wall
        return res
    if backend == "rccl" and not _state["hung"] and not all("RCCL_COMM_OK" in o for o in logs):
        # the communicator itself did not come up (no loopback interface, sockets forbidden ...): the environment cannot
        # host this launch; a failure AFTER the communicator exists is the library's
        return {"skip": "RCCL could not create a %d-rank communicator over loopback here:\n%s" % (world, text)}
    return {"error": "%s launch, %d ranks: %s after %.0f s\n%s" % (backend, world, why or "exit codes %s" % codes, wall, text)}


def _launch_fixture(backend, world):
    @pytest.fixture(scope="module", name="launch_%s_%d" % (backend, world))
    def fx(tmp_path_factory):
        res = _launch(backend, world, str(tmp_path_factory.mktemp("shards") / ("%s%d" % (backend, world))))
        if "wall_s" in res:
            print("launch %s %d ranks: %.1f s" % (backend, world, res["wall_s"]))
        return res
    return fx


# one module-scoped fixture per launch, created in the order the launches run
launch_host_2, launch_host_3, launch_host_4, launch_host_6, launch_rccl_3 = (_launch_fixture(b, w) for b, w in sm.LAUNCHES)

_PARAMS = {kind: [pytest.param(b, r, id="%s-%s" % (b, r["key"])) for b, w in sm.LAUNCHES for r in sm.runs_of(b, w) if r["kind"] == kind]
           for kind in ("eval", "solve", "refuse")}


def _record(request, backend, run):
    world = sm.CASES[run["case"]]["world"]
    res = request.getfixturevalue("launch_%s_%d" % (backend, world))
    if "skip" in res:
        pytest.skip(res["skip"])
    assert "error" not in res, res["error"]
    assert res["launch"]["backend"].startswith("rccl " if backend == "rccl" else "host")
    assert run["key"] in res["runs"], "no record of %s: %s" % (run["key"], sorted(res["runs"]))
    rec = res["runs"][run["key"]]
    print(run["key"], rec)
    return res, rec


def test_launch_wall_times(request):
    """Every launch's wall time, logged (SRMAP_PARITY_LOG) -- the figures LAUNCH_LIMIT_S is set from."""
    for b, w in sm.LAUNCHES:
        res = request.getfixturevalue("launch_%s_%d" % (b, w))
        assert any(k in res for k in ("wall_s", "skip", "error"))
        if "wall_s" in res:
            note(res["wall_s"], "launch %s %d ranks wall s" % (b, w))


@pytest.mark.parametrize("backend,run", _PARAMS["eval"])
def test_sharded_eval(request, backend, run):
    """Cost (the global one, on every rank) and the stitched gradient against the oracle of the whole problem, relative to
    max(1, |ref|); frame and grid replicas bit-equal.  The unsharded GPU evaluation's own error is in the record."""
    res, rec = _record(request, backend, run)
    case = sm.CASES[run["case"]]
    bar = BAR * TOL[run["dt"]]
    assert rec["status"] == [0] * case["world"]
    if case["id"] in ("F1", "F2", "R1", "R2", "R3"):
        assert rec["impl"] == [2] * case["world"]     # SRMAP_IMPL_TILED: band split / overlap decision are reached
    if case["id"].startswith("R4"):
        assert rec["impl"] == [1] * case["world"]     # the direct kernels
    if run["want_cost"]:
        assert rec["cost_err"] <= bar
        if case["mode"] == "frames":
            assert rec["replica_costs_equal"]
    if run["want_grad"]:
        assert rec["grad_err"] <= bar
        assert rec["replicas_equal"]


@pytest.mark.parametrize("backend,run", _PARAMS["solve"])
def test_sharded_solve(request, backend, run):
    """2 IRLS rounds x 6 CG iterations: the same decisions on every rank and as the unsharded solve, iterates equal up to
    the reduction order."""
    res, rec = _record(request, backend, run)
    assert all(c == rec["counts_unsharded"] for c in rec["counts"]), rec
    assert rec["solve_err"] <= 1e-9
    assert rec["replicas_equal"]


@pytest.mark.parametrize("backend,run", _PARAMS["refuse"])
def test_row_shard_refusal(request, backend, run):
    """A dy on a rounding tie under row shards: SRMAP_EUNSUPPORTED on every rank, before any communication -- the same
    communicator evaluates the next case (R4 over two ranks) correctly, so nothing was left half-posted."""
    res, rec = _record(request, backend, run)
    assert rec["status"] == [sm.EUNSUPPORTED] * sm.CASES[run["case"]]["world"], rec
    assert all("rounding tie" in m for m in rec["messages"])
    nxt = res["runs"]["R4w2-f64"]
    assert nxt["status"] == [0, 0] and nxt["cost_err"] <= BAR * TOL["f64"] and nxt["grad_err"] <= BAR * TOL["f64"]
