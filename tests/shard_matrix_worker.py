"""One rank of a launch of the sharded-evaluation matrix (tests/test_gpu_shard_matrix.py over tests/shard_matrix.py).

    python shard_matrix_worker.py <rank> <world> <port> <backend> <outdir>

Every rank shares GPU 0.  The rank initialises as tests/dist_gpu_worker.py does (torch, then gloo, then the host-callback
or the RCCL communicator; RCCL with every rank posing as a host of its own over loopback sockets) and then runs every
case of the table for its world over that ONE communicator: its shard through srmap_eval_sharded_device or
srmap_solve_sharded, the owned parts gathered on rank 0, compared there with the CPU oracle of the whole problem and
with the unsharded GPU evaluation, one record per run appended to <outdir>/results.json.

A rank left alone in a collective fails after 60 s (the gloo timeout) instead of waiting; a rank that meets an
unexpected error writes it to <outdir>/rank<r>.err and exits non-zero at once, without entering the next case.
"""
import json
import os
import sys
import traceback
from datetime import timedelta

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "super-resolution_amd", "python"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import shard_matrix as sm  # noqa: E402
from parity_log import note  # noqa: E402


def _err(a, ref):
    """max |a - ref| / max(1, |ref|), the suite's per-element measure (parity_log.relerr, without its log line)."""
    a, ref = np.asarray(a, dtype=float).ravel(), np.asarray(ref, dtype=float).ravel()
    return float(np.max(np.abs(a - ref) / np.maximum(1.0, np.abs(ref)))) if a.size else 0.0


class Rank:
    def __init__(self, rank, world, port, backend, outdir):
        self.rank, self.world, self.backend, self.outdir = rank, world, backend, outdir
        if backend == "rccl":  # before anything loads librccl
            os.environ["NCCL_HOSTID"] = "srmap-test-host-%d" % rank
            os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
            os.environ.setdefault("NCCL_IB_DISABLE", "1")
        torch.cuda.init()
        torch.zeros(1, device="cuda")  # torch's HIP runtime first (see tests/conftest.py)
        import oracle
        import srmap
        self.sr, self.orc = srmap, oracle
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world,
                                timeout=timedelta(seconds=60))
        self.ctx = srmap.Context(0)
        if backend == "rccl":
            box = [srmap.Comm.unique_id(self.ctx) if rank == 0 else None]
            dist.broadcast_object_list(box, src=0)
            self.comm = srmap.Comm(self.ctx, rank, world, backend="rccl", unique_id=box[0])
            print("RCCL_COMM_OK rank %d" % rank, flush=True)  # past this line a failure is the library's, not the environment's
        else:
            self.comm = srmap.Comm(self.ctx, rank, world, backend="host", dist=dist)
        self.frame_comms = {}   # frame groups -> the communicator of this rank's channel block (grid mode)
        self.results = {"launch": {"backend": self.comm.describe(), "world": world}, "runs": {}}
        self._ref = {}

    # ------------------------------------------------------------------ problems
    def problem(self, geom, lr, regs, weights, dtype):
        sr = self.sr
        p = sr.Problem(self.ctx, geom["W"], geom["H"], geom["C"], geom["K"], geom["s"], geom["shifts"], geom["blur"],
                       geom["sigma"], dtype)
        p.set_observations(lr)
        for r, w in zip(regs, weights):
            i = p.add_regularizer(*r)
            if w is not None:
                p.set_irls_weights(i, w)
        return p

    def whole(self, case, inp, dtype, weighted=True):
        x, lr, wts = inp
        geom = dict(W=case["W"], H=case["H"], C=case["C"], K=case["K"], s=case["s"], shifts=case["shifts"],
                    blur=case["blur"], sigma=case["sigma"])
        return self.problem(geom, lr, case["regs"], wts if weighted else [None] * len(wts), dtype)

    def oracle(self, case, inp, terms):
        """(f, g) of the whole problem by the CPU oracle."""
        key = (case["id"], terms)
        if key not in self._ref:
            x, lr, wts = inp
            orc = self.orc
            model = orc.ImageModel(scale=case["s"], shifts=case["shifts"], blur_ksize=case["blur"], blur_sigma=case["sigma"])
            ref = orc.Problem(model, lr)
            for r, w in zip(case["regs"], wts):
                ref.set_irls_weights(ref.add_regularizer(*r), w)
            if terms == sm.TERM_ALL:
                f, g = ref.objective(x)
            else:
                f, g = 0.0, np.zeros_like(x)
                if terms & sm.TERM_DATA:
                    fd, gd = ref.data_term(x)
                    f, g = f + fd, g + np.asarray(gd).reshape(x.shape)
                if terms & sm.TERM_REG:
                    for i in range(len(case["regs"])):
                        fr, gr = ref.reg_term(i, x)
                        f, g = f + fr, g + np.asarray(gr).reshape(x.shape)
            self._ref[key] = (float(f), np.asarray(g).reshape(x.shape))
        return self._ref[key]

    def descriptor(self, case, sh):
        sr = self.sr
        sd = sr.ShardDesc()
        for k, v in sh["desc"].items():
            setattr(sd, k, v)
        if case["mode"] == "grid":
            fgs = case["frame_groups"]
            if fgs not in self.frame_comms:
                nblocks = self.world // fgs
                if self.backend == "rccl":
                    fc = self.comm.split(sh["block"], sh["group"], sh["group"], fgs)
                else:  # collective: every rank creates every group, in the same order
                    groups = [dist.new_group([b * fgs + f for f in range(fgs)]) for b in range(nblocks)]
                    fc = sr.Comm(self.ctx, sh["group"], fgs, backend="host", dist=dist, group=groups[sh["block"]],
                                 group_ranks=[sh["block"] * fgs + f for f in range(fgs)])
                self.frame_comms[fgs] = fc
            sd.frame_comm = self.frame_comms[fgs]._h
        return sd

    # ------------------------------------------------------------------ runs
    def run(self, run):
        case = sm.CASES[run["case"]]
        os.environ["PYTEST_CURRENT_TEST"] = sm.node_id(self.backend, run) + " (call)"  # the node parity_log names
        inp = sm.inputs(case)
        sh = sm.shard(case, self.rank, inp)
        rec = {"case": case["id"], "kind": run["kind"]}
        if run["overlap"] is not None:
            self.comm.set_overlap(run["overlap"])
        if run["kind"] == "solve":
            self.solve(run, case, inp, sh, rec)
        else:
            self.evaluate(run, case, inp, sh, rec)
        if self.rank == 0:
            self.results["runs"][run["key"]] = rec
            tmp = os.path.join(self.outdir, "results.json.tmp")
            with open(tmp, "w") as f:
                json.dump(self.results, f)
            os.replace(tmp, os.path.join(self.outdir, "results.json"))

    def gather(self, obj):
        box = [None] * self.world
        dist.all_gather_object(box, obj)
        return box

    def evaluate(self, run, case, inp, sh, rec):
        sr, dtype = self.sr, run["dtype"]
        tdt = torch.float64 if dtype == sr.F64 else torch.float32
        p = self.problem(sh["geom"], sh["lr"], case["regs"], sh["weights"], dtype)
        if sh["cost_rows"]:
            p.set_cost_rows(*sh["cost_rows"])
        sd = self.descriptor(case, sh)
        xd = torch.from_numpy(sh["x"]).to(tdt).cuda()
        gd = torch.full_like(xd, 3.0) if run["want_grad"] else None  # not zero: a part nobody writes shows
        status, message, f = 0, "", None
        torch.cuda.synchronize()  # the library evaluates on its own stream: torch's fills must be behind us first
        try:
            f = p.eval_sharded_device(self.comm, sd, xd.data_ptr(), gd.data_ptr() if gd is not None else 0,
                                      run["terms"], want_cost=run["want_cost"])
        except sr.SrmapError as e:
            status, message = e.status, str(e)
        torch.cuda.synchronize()
        if status != 0 and run["kind"] != "refuse":
            raise RuntimeError("%s: rank %d: %s" % (run["key"], self.rank, message))
        g_own = gd.cpu().numpy().astype(np.float64)[sh["own_local"]] if gd is not None and status == 0 else None
        mine = dict(status=status, message=message, cost=f, g=g_own, impl=p.active_impl())
        everyone = self.gather(mine)
        if self.rank != 0:
            return
        rec.update(status=[m["status"] for m in everyone], messages=[m["message"] for m in everyone],
                   impl=[m["impl"] for m in everyone], dtype=run["dt"])
        if run["kind"] == "refuse":
            return
        f_ref, g_ref = self.oracle(case, inp, run["terms"])
        full = self.whole(case, inp, dtype)
        f_gpu, g_gpu = full.eval(inp[0], run["terms"])
        what = "%s %s" % (case["mode"], run["dt"])
        rec["gpu_cost_err"] = note(abs(f_gpu - f_ref) / max(1.0, abs(f_ref)), "unsharded cost " + what)
        rec["gpu_grad_err"] = note(_err(g_gpu, g_ref), "unsharded grad " + what)
        if run["want_cost"]:  # the global cost, on every rank
            rec["cost_err"] = note(max(abs(m["cost"] - f_ref) for m in everyone) / max(1.0, abs(f_ref)), "sharded cost " + what)
            rec["cost_vs_gpu"] = max(abs(m["cost"] - f_gpu) for m in everyone) / max(1.0, abs(f_gpu))
        if run["want_grad"]:
            g_all = sm.assemble(case, [m["g"] for m in everyone])
            rec["grad_err"] = note(_err(g_all, g_ref), "sharded grad " + what)
            rec["grad_vs_gpu"] = _err(g_all, g_gpu)
            # where the worst element sits, and how many miss the f32 tolerance: a wrong band shows as rows, a swapped
            # neighbour as a halo's worth of them
            e = np.abs(g_all - g_ref) / np.maximum(1.0, np.abs(g_ref))
            at = np.unravel_index(int(np.argmax(e)), e.shape)
            rec["grad_worst"] = [int(i) for i in at] + [float(g_all[at]), float(g_ref[at])]
            rec["grad_off"] = int(np.sum(e > 2e-5))
            rec["replicas_equal"] = all(np.array_equal(everyone[s[0]]["g"], everyone[r]["g"])
                                        for s in sm.replica_sets(case) for r in s[1:])
        if run["want_cost"] and case["mode"] == "frames":
            rec["replica_costs_equal"] = len({m["cost"] for m in everyone}) == 1

    def solve(self, run, case, inp, sh, rec):
        sr = self.sr
        opts = sr.default_irls_options()
        opts.max_num_irls_iterations = 2
        opts.max_num_solver_iterations = 6
        none = [None] * len(case["regs"])  # the solve computes its own IRLS weights
        p = self.problem(sh["geom"], sh["lr"], case["regs"], none, sr.F64)
        if sh["cost_rows"]:
            p.set_cost_rows(*sh["cost_rows"])
        sd = self.descriptor(case, sh)
        x_sol, rep = p.solve(sh["x"], opts, comm=self.comm, shard=sd)
        mine = dict(x=x_sol[sh["own_local"]], counts=[rep.irls_rounds, rep.cg_iterations, rep.evaluations],
                    final_cost=rep.final_cost)
        everyone = self.gather(mine)
        if self.rank != 0:
            return
        x_ref, rep_ref = self.whole(case, inp, sr.F64, weighted=False).solve(inp[0], opts)
        rec.update(counts=[m["counts"] for m in everyone], final_cost=[m["final_cost"] for m in everyone], dtype="f64",
                   counts_unsharded=[rep_ref.irls_rounds, rep_ref.cg_iterations, rep_ref.evaluations],
                   final_cost_unsharded=rep_ref.final_cost,
                   solve_err=note(_err(sm.assemble(case, [m["x"] for m in everyone]), x_ref), "sharded solve " + case["mode"]),
                   replicas_equal=all(np.array_equal(everyone[s[0]]["x"], everyone[r]["x"])
                                      for s in sm.replica_sets(case) for r in s[1:]))


def main():
    rank, world, port, backend, outdir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    try:
        me = Rank(rank, world, port, backend, outdir)
        for run in sm.runs_of(backend, world):
            me.run(run)
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:  # not into the next case: the launcher ends the other ranks when this one is gone
        with open(os.path.join(outdir, "rank%d.err" % rank), "w") as f:
            traceback.print_exc(file=f)
        traceback.print_exc()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(3)


if __name__ == "__main__":
    main()
