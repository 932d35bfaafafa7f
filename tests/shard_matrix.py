"""The case table of the multi-rank sharded-evaluation matrix (tests/test_gpu_shard_matrix.py runs it on the GPU through
tests/shard_matrix_worker.py; tests/test_shard_matrix_cpu.py checks the table itself with the oracle alone).

Imports without a GPU: numpy and srmap_dist only (the inputs come from error_bars, imported when they are asked for).

Every case is one whole problem and one way of cutting it over `world` ranks; shard(case, rank, inputs) returns what one
rank holds: the geometry of its sub-problem, its slice of the observations, of x and of the IRLS weights, the fields of
its srmap_shard_desc and the part of the gradient it owns.  A RUN is a case with a dtype and the arguments of one
srmap_eval_sharded_device / srmap_solve_sharded call.

The shapes are the smallest at which the named edge exists.  None had to be moved for the tile planner
(ztile_plan.hip plans a band when W, H > 4 E + 2 S, E the largest shift): the smallest band here is R3's last one,
12 + 3 rows against 4 * 1 + 2 * 3 = 10.  R4 is the other way round: it is there for the direct kernels, and at
BAND_CASES[4]'s width of 32 the sub-pixel plan (W, H > 4 Dr + 2 S = 28, Dr = 2 + 2 + 1) takes the taller bands, so its
width is 28, at which no band is planned.

R5's y shift: a shift of an exact odd multiple of 1/64 px is a quantisation tie that double arithmetic resolves the same
way in every row, so its warp table is uniform and a row shard evaluates it correctly -- nothing is refused.  The
refusal belongs to a dy within floating-point rounding of such a tie, (16.5 + 1e-10) / 1024 here, whose rounding
direction depends on the row index (model_tables.hpp make_warp: the per-row table).  test_shard_matrix_cpu.py asserts with
the oracle's warp tables that every band of R5 really has a non-uniform table, forward and transposed.
"""
import numpy as np

import srmap_dist

# include/srmap.h (test_shard_matrix_cpu.py compares them with the binding's)
F64, F32 = 0, 1
REG_TV, REG_TV3D, REG_BTV = 0, 1, 2
TERM_DATA, TERM_REG, TERM_ALL = 1, 2, 3
SHARD_FRAMES, SHARD_ROWS, SHARD_CHANNELS, SHARD_GRID = 1, 2, 3, 4
EUNSUPPORTED = 4
MODES = {"frames": SHARD_FRAMES, "rows": SHARD_ROWS, "channels": SHARD_CHANNELS, "grid": SHARD_GRID}
DT = {"f64": F64, "f32": F32}
# srmap_shard_desc without frame_comm, which is the worker's to make
ShardFields = ("mode", "own_row0", "own_row1", "send_up_rows", "send_down_rows", "own_ch0", "own_ch1", "reg_rank", "frame_groups")

LAMBDA = 2.0 ** -6  # error_bars.LAMBDA: dyadic, like the decays 0.5 and 0.625
STALE = -7.0        # what every halo row / plane of a rank's x holds before the library refreshes it

_INT4 = [[k % 4, (k * 3) % 4] for k in range(8)]                       # integer shifts < 4 (the existing worker's)
_INT1 = [[0, 0], [1, 1], [-1, 0], [0, -1], [1, -1]]                    # |shift| <= 1
_SUBPIX = [[0.5, 0.25], [-1.25, 1.5], [2.0, -0.75]]                    # test_gpu_bands.BAND_CASES[4]: off the 1/32 ties
_TIE = [[0.5, 0.0161132812500001], [-1.25, 1.5], [2.0, -0.75]]         # frame 0: dy on a rounding tie (module docstring)
_BTV3 = (REG_BTV, LAMBDA, 3, 0.5)
_TV = (REG_TV, LAMBDA, 0, 0.0)
_TV3D = (REG_TV3D, LAMBDA, 0, 0.0)


def _case(cid, mode, world, s, blur, shifts, regs, C, W, h, seed, **kw):
    c = dict(id=cid, mode=mode, world=world, s=s, blur=blur, sigma=1.0 if blur else 0.0, shifts=[list(map(float, v)) for v in shifts],
             regs=list(regs), C=C, K=len(shifts), W=W, H=h * s, seed=seed, halo=0, reach=0, reg_rank=0, frame_groups=1)
    c.update(kw)
    return c


CASES = {c["id"]: c for c in [
    # ---- rows: LR rows split 9/9/8, 8/8/7, 5/5/5/4, 5/4/4; halo = srmap_dist.band_halo(s, blur, max |shift|, reach)
    _case("R1", "rows", 3, 4, 3, _INT4, [_BTV3], 2, 80, 26, 11, halo=8, reach=3),
    _case("R2", "rows", 3, 2, 3, _INT1, [_TV], 1, 74, 23, 12, halo=4, reach=1),
    _case("R3", "rows", 4, 3, 0, _INT1[:4], [(REG_BTV, LAMBDA, 2, 0.625)], 1, 75, 19, 13, halo=3, reach=2),
    _case("R4", "rows", 3, 4, 3, _SUBPIX, [_TV], 1, 28, 13, 14, halo=8, reach=1),
    _case("R4w2", "rows", 2, 4, 3, _SUBPIX, [_TV], 1, 28, 13, 14, halo=8, reach=1),
    _case("R5", "rows", 2, 4, 3, _TIE, [_TV], 1, 28, 13, 14, halo=8, reach=1),
    # ---- frames: the regulariser split by bands of whole tile rows (F1, F2) or left to reg_rank (F3)
    _case("F1", "frames", 3, 4, 3, _INT4, [_BTV3], 2, 80, 26, 21),
    _case("F2", "frames", 4, 4, 3, _INT4[:5], [_BTV3], 2, 80, 10, 22),
    _case("F3", "frames", 3, 4, 3, _INT4, [_BTV3, _TV], 2, 80, 26, 23, reg_rank=2),
    # ---- channels: BTV + 3-D TV couple neighbouring planes (one halo plane per neighbour); C3 has no coupling
    _case("C1", "channels", 3, 4, 3, _INT4[:4], [_BTV3, _TV3D], 5, 80, 12, 31),
    _case("C2", "channels", 4, 4, 3, _INT4[:4], [_BTV3, _TV3D], 4, 80, 12, 32),
    _case("C3", "channels", 3, 4, 3, _INT4[:4], [_BTV3], 3, 80, 12, 33),
    # ---- grid: rank = channel block * frame_groups + frame group; 3 blocks (2/2/1 channels) x 2 groups (3 / 2 frames)
    _case("G1", "grid", 6, 4, 3, _INT4[:5], [_BTV3, _TV3D], 5, 80, 12, 41, frame_groups=2),
]}


def _run(case, dt, kind="eval", name="", overlap=None, terms=TERM_ALL, cost=True, grad=True, rccl=False):
    key = "-".join(v for v in (case, dt, name) if v)
    return dict(key=key, case=case, dtype=DT[dt], dt=dt, kind=kind, overlap=overlap, terms=terms, want_cost=cost,
                want_grad=grad, backends=("host", "rccl") if rccl else ("host",))


_FRAME_VARIANTS = [("all", TERM_ALL, True, True), ("data", TERM_DATA, True, True), ("reg", TERM_REG, True, True),
                   ("nocost", TERM_ALL, False, True), ("nograd", TERM_ALL, True, False)]

# In the order a launch runs them.  The RCCL launch (world 3) runs R1, F1 and C1 only.
RUNS = (
    # world 2: the refusal first, then the same communicator must still evaluate
    [_run("R5", "f64", kind="refuse", overlap=False), _run("R4w2", "f64", overlap=False), _run("R4w2", "f32", overlap=False)] +
    # world 3
    [_run("R1", dt, name="ovl%d" % o, overlap=bool(o), rccl=True) for dt in ("f64", "f32") for o in (0, 1)] +
    [_run("R2", "f32", name="ovl1", overlap=True)] +
    [_run("R4", dt, overlap=False) for dt in ("f64", "f32")] +
    [_run(f, dt, name=n, terms=t, cost=c, grad=g, rccl=f == "F1") for f in ("F1", "F3") for dt in ("f64", "f32")
     for n, t, c, g in _FRAME_VARIANTS] +
    [_run("C1", dt, rccl=True) for dt in ("f64", "f32")] + [_run("C3", dt) for dt in ("f64", "f32")] +
    [_run(c, "f64", kind="solve", name="solve", rccl=True) for c in ("R1", "F1", "C1")] +
    # world 4
    [_run("R3", "f64", name="ovl1", overlap=True)] +
    [_run("F2", dt, name=n, terms=t, cost=c, grad=g) for dt in ("f64", "f32") for n, t, c, g in _FRAME_VARIANTS] +
    [_run("C2", dt) for dt in ("f64", "f32")] +
    # world 6
    [_run("G1", dt) for dt in ("f64", "f32")] + [_run("G1", "f64", kind="solve", name="solve")]
)

LAUNCHES = [("host", 2), ("host", 3), ("host", 4), ("host", 6), ("rccl", 3)]  # run strictly one after the other


def runs_of(backend, world):
    return [r for r in RUNS if CASES[r["case"]]["world"] == world and backend in r["backends"]]


def node_id(backend, run):
    """The pytest node that reads this run's record (the worker logs its errors under it: parity_log)."""
    test = {"eval": "test_sharded_eval", "solve": "test_sharded_solve", "refuse": "test_row_shard_refusal"}[run["kind"]]
    return "tests/test_gpu_shard_matrix.py::%s[%s-%s]" % (test, backend, run["key"])


def inputs(case):
    """(x [C][H][W], lr [K][C][h][w], [IRLS weights per regulariser]) on dyadic grids: exact in f32, so the oracle sees
    the numbers the GPU sees.  The weights differ from ones and from each other."""
    import error_bars as eb
    rng = np.random.default_rng(7000 + case["seed"])
    x, lr = eb.dyadic_inputs(rng, case["K"], case["C"], case["H"], case["W"], case["s"])
    wts = [eb.dyadic_weights(rng, case["C"], case["H"], case["W"]) for _ in case["regs"]]
    return x, lr, wts


def row_bands(case):
    return [srmap_dist.row_band(case["H"], case["s"], case["world"], r, case["halo"]) for r in range(case["world"])]


def reg_band(H, world, rank):
    """shard_eval.hip's regulariser band of frame mode, restated: whole tile rows (8 HR rows), ceil(tiles / world) per
    rank; returns the unclamped [rr0, rr1) and the band clamped to the image as eval_typed clamps it."""
    tiles = (H + 7) // 8
    per = (tiles + world - 1) // world
    rr0, rr1 = rank * per * 8, (rank + 1) * per * 8
    return (rr0, rr1), (min(rr0, H), min(rr1, H))


def shard(case, rank, inp):
    """What `rank` holds of `case`.  desc: the srmap_shard_desc fields (frame_comm is the worker's to make);
    own: index into a global [C][H][W] array of what the rank owns; own_local: the same part inside its local arrays;
    cost_rows: the argument of srmap_problem_set_cost_rows (row shards)."""
    x, lr, wts = inp
    mode, world, s = case["mode"], case["world"], case["s"]
    C, K, W, H = case["C"], case["K"], case["W"], case["H"]
    desc = dict(mode=MODES[mode], own_row0=0, own_row1=0, send_up_rows=0, send_down_rows=0, own_ch0=0, own_ch1=0,
                reg_rank=case["reg_rank"], frame_groups=0)
    frames, rows, chans = list(range(K)), (0, H), (0, C)   # global frames, rows and channels of the local problem
    out = dict(cost_rows=None, block=None, group=None)
    if mode == "frames":
        frames = srmap_dist.frame_shard(K, world, rank)
        own, own_local = (slice(None), slice(None)), (slice(None), slice(None))
    elif mode == "rows":
        bands = row_bands(case)
        (r0, r1), (e0, e1) = bands[rank]
        rows = (e0, e1)
        desc["own_row0"], desc["own_row1"] = r0 - e0, r1 - e0
        if rank + 1 < world:   # my last owned rows fill the lower neighbour's top halo
            (n0, _), (ne0, _) = bands[rank + 1]
            desc["send_down_rows"] = n0 - ne0
        if rank > 0:           # my first owned rows fill the upper neighbour's bottom halo
            (_, u1), (_, ue1) = bands[rank - 1]
            desc["send_up_rows"] = ue1 - u1
        out["cost_rows"] = (r0 - e0, r1 - e0)
        own, own_local = (slice(None), slice(r0, r1)), (slice(None), slice(r0 - e0, r1 - e0))
    else:
        fgs = case["frame_groups"] if mode == "grid" else 1
        block, group = srmap_dist.grid_coords(world, rank, fgs)
        c0, c1 = srmap_dist.channel_shard(C, world // fgs, block)
        coupled = any(r[0] == REG_TV3D for r in case["regs"])
        lo, hi = (1 if coupled and c0 > 0 else 0), (1 if coupled and c1 < C else 0)
        chans = (c0 - lo, c1 + hi)
        desc["own_ch0"], desc["own_ch1"] = lo, lo + (c1 - c0)
        if mode == "grid":
            frames = srmap_dist.frame_shard(K, fgs, group)
            desc["frame_groups"] = fgs
        out["block"], out["group"] = block, group
        own, own_local = (slice(c0, c1), slice(None)), (slice(lo, lo + c1 - c0), slice(None))
    cut = (slice(chans[0], chans[1]), slice(rows[0], rows[1]))
    x_true = np.ascontiguousarray(x[cut])
    x_loc = np.full_like(x_true, STALE)          # halo rows and planes start stale
    x_loc[own_local] = x_true[own_local]
    out.update(
        geom=dict(W=W, H=rows[1] - rows[0], C=chans[1] - chans[0], K=len(frames), s=s, shifts=[case["shifts"][k] for k in frames],
                  blur=case["blur"], sigma=case["sigma"]),
        frames=frames, rows=rows, chans=chans, desc=desc, own=own, own_local=own_local, x=x_loc, x_true=x_true,
        lr=np.ascontiguousarray(lr[frames][:, chans[0]:chans[1], rows[0] // s:rows[1] // s, :]),
        weights=[np.ascontiguousarray(w[cut]) for w in wts])
    return out


def assemble(case, parts):
    """The whole [C][H][W] array from the ranks' owned parts (frame and grid replicas: the first of each)."""
    mode = case["mode"]
    if mode == "frames":
        return np.asarray(parts[0])
    if mode == "rows":
        return np.concatenate(parts, axis=1)
    fgs = case["frame_groups"] if mode == "grid" else 1
    return np.concatenate(parts[0::fgs], axis=0)


def replica_sets(case):
    """Groups of ranks whose owned results must be bit-equal."""
    world, mode = case["world"], case["mode"]
    if mode == "frames":
        return [list(range(world))]
    if mode == "grid":
        fgs = case["frame_groups"]
        return [list(range(b * fgs, (b + 1) * fgs)) for b in range(world // fgs)]
    return []
