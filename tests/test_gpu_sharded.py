"""Multi-GPU paths of the C ABI on ONE GPU: the sharded evaluation and the sharded IRLS/CG solve
(srmap_eval_sharded_device, srmap_solve_sharded) with 2 ranks sharing GPU 0 over the host-callback communicator
(gloo) AND over the RCCL communicator (loopback sockets: each rank names itself its own host), for frame, row-band and
channel (+ 3-D TV halo plane) shards, against the single-process result; the RCCL backend with a one-rank
communicator; and the CG trajectory against ALGLIB's / the oracle's mincg."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import oracle as orc
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("backend", ["host", "rccl"])
@pytest.mark.parametrize("mode", ["frames", "frames2", "frames_mixed", "rows", "rows_overlap", "channels", "grid"])
def test_two_ranks_on_one_gpu(tmp_path, mode, backend):
    """2 ranks (grid: 4 = 2 channel blocks x 2 frame groups, the frames x channels sharding of BASELINE configs[4]).
    frames: the regulariser split over the ranks by row band; frames2: two regularisers, evaluated on reg_rank;
    frames_mixed: rank 1 forced to the direct kernels -- the band split is a collective decision (all ranks fall back to
    reg_rank), otherwise the regulariser would be counted one and a half times; rows_overlap: the halo exchange posted
    on the side stream under the interior tile rows.
    backend "rccl": the same over the RCCL communicator -- ncclCommInitRank with N = 2 / 4, ncclAllReduce, the grouped
    ncclSend / ncclRecv halo exchange and ncclCommSplit (grid) -- every rank posing as a host of its own so that RCCL
    accepts the shared GPU and runs its socket transport over loopback (tests/dist_gpu_worker.py)."""
    world, port = (4 if mode == "grid" else 2), _free_port()
    out = str(tmp_path / "res.json")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_gpu_worker.py"), str(r), str(world),
                               str(port), mode, out, backend], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True)
             for r in range(world)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    if backend == "rccl" and any(p.returncode != 0 for p in procs) and not all("RCCL_COMM_OK" in o for o in logs):
        # the communicator itself did not come up (no loopback interface, sockets forbidden ...): the environment cannot
        # host this test; a failure AFTER the communicator exists is the library's and fails below
        pytest.skip("RCCL could not create a %d-rank communicator over loopback here:\n%s" % (world, "\n".join(o[-600:] for o in logs)))
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    res = json.load(open(out))
    print(res)
    assert res["backend"].startswith("rccl " if backend == "rccl" else "host")
    assert res["cost_err"] <= 1e-12 and res["grad_err"] <= 1e-11
    # same decisions on every rank and as the single-process solve; iterates equal up to reduction order
    assert len(set(res["cg"])) == 1 and len(set(res["irls"])) == 1 and len(set(res["evals"])) == 1
    assert res["solve_err"] <= 1e-9
    if mode in ("frames", "frames2", "frames_mixed", "grid"):
        assert res["replicas_equal"]


@pytest.mark.parametrize("shard,how", [("rows", "--test-single-device"), ("channels", "--test-single-device"),
                                       ("rows", "--test-rccl-loopback")])
def test_bench_spawns_its_ranks(shard, how):
    """`python bench.py --gpus 2` as a bare subprocess (no launcher, no WORLD_SIZE): the bench re-executes itself under
    torch.distributed.run, one rank per process; here both ranks share GPU 0 over the host-callback communicator, or over
    RCCL itself on loopback sockets (the path the driver's N > 1 run takes, minus xGMI).  --full: the frames variant and
    the configs[2] block are part of the line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    rccl = how == "--test-rccl-loopback"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", how, "--full", "--watchdog-s", "240",
                        "--steps", "5", "--warmup", "2", "--clock-ramp-ms", "0", "--min-timed-ms", "0", "--hr", "512",
                        "--shard", shard],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if rccl and r.returncode != 0 and r.stderr.count("RCCL communicator up") < 2:
        pytest.skip("RCCL could not create a 2-rank communicator over loopback here:\n" + r.stderr[-1500:])
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 5 and out["value"] > 0
    assert out["config"]["shard"] == shard
    if shard == "rows":
        assert out["scaling"] == "strong" and out["config"]["comm_ranks"] == 2
        # the labels say what ran
        if rccl:
            assert out["config"]["comm_backend"].startswith("rccl over loopback") and out["config"]["comm_library"].startswith("rccl ")
            assert out["frames_variant"]["value"] > 0 and "ncclAllReduce" in out["frames_variant"]["collective_per_step"]
            assert "ncclSend/ncclRecv" in out["config"]["collective_per_step"]
        else:
            assert out["config"]["comm_backend"].startswith("host") and out["config"]["comm_library"] == "host callbacks"
            assert out["frames_variant"]["value"] > 0 and "host-callback all-reduce" in out["frames_variant"]["collective_per_step"]
            assert "host-callback send/recv" in out["config"]["collective_per_step"]
        # the configs[2] block: rows strong scaling with its own N = 1 time from the same run
        c3 = out["cfg3"]
        assert c3["shard"] == "rows" and c3["scaling"] == "strong" and c3["value"] > 0
        assert c3["n1_reference_ms_per_step"] > 0 and c3["speedup_vs_n1_in_this_run"] > 0
        assert "configs[2]" in c3["workload"]
    else:
        assert out["scaling"] == "weak" and out["config"]["collective_per_step"].startswith("none")


def test_rccl_backend_world_one():
    """The RCCL code path (dlopen, ncclCommInitRank, ncclAllReduce on the stream) with a one-rank communicator."""
    import torch
    import srmap
    ctx = srmap.Context(0)
    uid = srmap.Comm.unique_id(ctx)
    assert len(uid) == 128
    comm = srmap.Comm(ctx, 0, 1, backend="rccl", unique_id=uid)
    # the communicator names the collective library it resolved (a process may carry several librccl copies)
    what = comm.describe().split()
    assert what[0] == "rccl" and int(what[1]) > 0 and "rccl" in what[2]
    assert comm.info() == (0, 1, 1)
    comm.set_overlap(True)   # opt-in of the halo-exchange overlap (row shards); a no-op for this one-rank solve
    t = torch.arange(1000, dtype=torch.float64, device="cuda")
    comm.allreduce(t.data_ptr(), t.numel(), srmap.F64, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), torch.arange(1000, dtype=torch.float64))
    comm.allreduce(t.data_ptr(), t.numel(), srmap.F64, 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), torch.arange(1000, dtype=torch.float64))
    # a one-rank communicator leaves the solve untouched
    rng = np.random.default_rng(1)
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    p = srmap.Problem(ctx, 48, 32, 1, 4, 2, shifts, 3, 1.0, srmap.F64)
    p.set_observations(rng.random((4, 1, 16, 24)))
    p.add_regularizer(srmap.REG_TV, 0.01)
    x0 = rng.random((1, 32, 48))
    sd = srmap.ShardDesc()
    sd.mode = srmap.SHARD_FRAMES
    xa, ra = p.solve(x0)
    xb, rb = p.solve(x0, comm=comm, shard=sd)
    assert np.array_equal(xa, xb) and ra.evaluations == rb.evaluations


@pytest.mark.parametrize("blur", [0, 3])
def test_cg_trajectory_matches_mincg(blur):
    """run_cg (csrc/solver.hip) against ALGLIB's mincg (oracle/_ref when built, else the restatement, which is
    bit-exact against it) on the SMOOTH data term: same iteration count, evaluation count and termination type, the
    cost of every accepted iterate to 1e-11."""
    import srmap
    ctx = srmap.Context(0)
    rng = np.random.default_rng(9)
    s, K, h, w = 2, 4, 20, 28
    H, W = h * s, w * s
    shifts = [[0, 0], [1, 1], [0, 1], [1, 0]]
    model = orc.ImageModel(scale=s, shifts=shifts, blur_ksize=blur, blur_sigma=1.0 if blur else 0.0)
    gt = rng.random((1, H, W))
    lr = np.stack([model.apply(gt, k) for k in range(K)]) + 0.01 * rng.standard_normal((K, 1, h, w))
    ref = orc.Problem(model, lr)
    x0 = orc.resize_nearest(lr[0, 0], W, H)[None]
    eps = 1e-6 * x0.size * 0.0 + 1e-7
    trace = []
    x_ref, rep_ref = orc.mincg(lambda x: (lambda fg: (fg[0], fg[1].ravel()))(ref.objective(x.reshape(1, H, W))),
                               x0, eps, eps, eps, 40, use_alglib=orc.have_ref(), trace=trace)
    p = srmap.Problem(ctx, W, H, 1, K, s, shifts, blur, 1.0 if blur else 0.0, srmap.F64)
    p.set_observations(lr)
    x, its, nfev, term, ftrace = p.cg_trace(x0, eps, eps, eps, 40)
    print("iterations %d/%d nfev %d/%d termination %d/%d" % (its, rep_ref.iterations, nfev, rep_ref.nfev, term,
                                                              rep_ref.termination_type))
    assert (its, nfev, term) == (rep_ref.iterations, rep_ref.nfev, rep_ref.termination_type)
    assert len(ftrace) == nfev
    # ALGLIB reports the accepted point of every iteration (xrep): its cost must appear in the GPU's evaluation log
    f_iter = [f for _, f in trace]
    for f in f_iter[1:]:
        assert np.min(np.abs(ftrace - f) / max(1.0, abs(f))) <= 1e-11
    assert abs(ftrace[-1] - rep_ref.f) <= 1e-11 * max(1.0, abs(rep_ref.f)) or \
        np.min(np.abs(ftrace - rep_ref.f)) <= 1e-11 * max(1.0, abs(rep_ref.f))
    assert np.max(np.abs(x - x_ref.reshape(1, H, W))) <= 1e-8
