"""tests/shard_matrix.py checked without the code under test: the descriptors tile every problem and satisfy what
shard_exchange_x demands, the halos of the row cases suffice (oracle band problems reassemble the oracle's whole
objective), frame mode's regulariser bands partition the image with the empty and the clipped band where the table says
they are, R5's bands really carry a non-uniform warp table, and srmap_dist.band_halo rounds a fractional shift up."""
import math

import numpy as np
import pytest

import oracle as orc
import shard_matrix as sm
import srmap_dist

ALL = sorted(sm.CASES)
ROWS = [c for c in ALL if sm.CASES[c]["mode"] == "rows"]


@pytest.fixture(scope="module")
def inputs():
    cache = {}

    def get(cid):
        if cid not in cache:
            cache[cid] = sm.inputs(sm.CASES[cid])
            for a in (cache[cid][0], cache[cid][1]) + tuple(cache[cid][2]):
                a.setflags(write=False)
        return cache[cid]
    return get


def test_constants_match_the_binding():
    import srmap
    assert (sm.F64, sm.F32, sm.REG_TV, sm.REG_TV3D, sm.REG_BTV) == (srmap.F64, srmap.F32, srmap.REG_TV, srmap.REG_TV3D, srmap.REG_BTV)
    assert (sm.TERM_DATA, sm.TERM_REG, sm.TERM_ALL, sm.EUNSUPPORTED) == (srmap.TERM_DATA, srmap.TERM_REG, srmap.TERM_ALL, srmap.EUNSUPPORTED)
    assert (sm.SHARD_FRAMES, sm.SHARD_ROWS, sm.SHARD_CHANNELS, sm.SHARD_GRID) == \
        (srmap.SHARD_FRAMES, srmap.SHARD_ROWS, srmap.SHARD_CHANNELS, srmap.SHARD_GRID)
    assert sorted(sm.ShardFields) == sorted(n for n, _ in srmap.ShardDesc._fields_ if n != "frame_comm")
    assert (orc.REG_TV, orc.REG_TV3D, orc.REG_BTV) == (sm.REG_TV, sm.REG_TV3D, sm.REG_BTV)


def test_the_table_holds_the_edges_it_names():
    """The splits the matrix exists for, restated from the helpers: a wrong shape would silently drop the edge."""
    def heights(cid):
        return [b[0][1] - b[0][0] for b in sm.row_bands(sm.CASES[cid])]
    assert heights("R1") == [36, 36, 32] and heights("R2") == [16, 16, 14] and heights("R3") == [15, 15, 15, 12]
    assert (sm.CASES["R1"]["halo"], sm.CASES["R2"]["halo"], sm.CASES["R3"]["halo"]) == (8, 4, 3)  # kReach = 4: above, at, below
    frames = lambda cid: [len(srmap_dist.frame_shard(sm.CASES[cid]["K"], sm.CASES[cid]["world"], r)) for r in range(sm.CASES[cid]["world"])]
    assert frames("F1") == [3, 3, 2] and frames("F2") == [2, 1, 1, 1] and sm.CASES["F3"]["reg_rank"] == 2
    blocks = lambda cid, n: [np.diff(srmap_dist.channel_shard(sm.CASES[cid]["C"], n, r))[0] for r in range(n)]
    assert blocks("C1", 3) == [2, 2, 1] and blocks("C2", 4) == [1, 1, 1, 1] and blocks("G1", 3) == [2, 2, 1]
    g = sm.CASES["G1"]
    assert [len(srmap_dist.frame_shard(g["K"], 2, f)) for f in range(2)] == [3, 2]
    for c in sm.CASES.values():
        if c["mode"] in ("frames", "grid"):   # a rank without frames is not part of the matrix
            assert c["K"] >= (c["world"] if c["mode"] == "frames" else c["frame_groups"])
    # every run belongs to exactly one launch, and the launches cover the table
    assert {(b, sm.CASES[r["case"]]["world"]) for r in sm.RUNS for b in r["backends"]} == set(sm.LAUNCHES)
    assert len({r["key"] for r in sm.RUNS}) == len(sm.RUNS)
    assert {r["case"] for r in sm.RUNS} == set(sm.CASES)
    assert {r["case"] for r in sm.runs_of("rccl", 3)} == {"R1", "F1", "C1"}
    keys2 = [r["key"] for r in sm.runs_of("host", 2)]
    assert keys2.index("R5-f64") + 1 == keys2.index("R4w2-f64")   # the refusal, then the same communicator evaluates


@pytest.mark.parametrize("cid", ALL)
def test_descriptors_tile_the_problem(cid, inputs):
    case = sm.CASES[cid]
    world, mode = case["world"], case["mode"]
    shards = [sm.shard(case, r, inputs(cid)) for r in range(world)]
    x, lr, wts = inputs(cid)
    # the owned parts partition the whole: every element of a [C][H][W] array is owned once per replica set
    count = np.zeros(x.shape, dtype=int)
    for sh in shards:
        count[sh["own"]] += 1
        # the local arrays are the global ones' cuts; owned x is authoritative, everything else starts stale
        assert np.array_equal(sh["x"][sh["own_local"]], x[sh["own"]])
        stale = np.ones(sh["x"].shape, dtype=bool)
        stale[sh["own_local"]] = False
        assert np.all(sh["x"][stale] == sm.STALE)
        g = sh["geom"]
        assert sh["x"].shape == (g["C"], g["H"], g["W"]) and sh["lr"].shape == (g["K"], g["C"], g["H"] // g["s"], g["W"] // g["s"])
        assert all(w.shape == sh["x"].shape for w in sh["weights"]) and len(sh["weights"]) == len(case["regs"])
        assert set(sh["desc"]) == set(sm.ShardFields) and sh["desc"]["mode"] == sm.MODES[mode]
    replicas = {"frames": world, "grid": case["frame_groups"]}.get(mode, 1)
    assert np.all(count == replicas)
    assert sm.assemble(case, [x[sh["own"]] for sh in shards]).shape == x.shape
    assert np.array_equal(sm.assemble(case, [x[sh["own"]] for sh in shards]), x)
    if mode in ("frames", "grid"):
        groups = case["frame_groups"] if mode == "grid" else world
        first = shards[:groups]   # the frame shards of one channel block
        assert sorted(k for sh in first for k in sh["frames"]) == list(range(case["K"]))
    if mode == "rows":
        for r, sh in enumerate(shards):
            d, H = sh["desc"], sh["geom"]["H"]
            own = d["own_row1"] - d["own_row0"]
            assert d["own_row0"] % case["s"] == 0 and d["own_row1"] % case["s"] == 0 and own > 0
            assert sh["cost_rows"] == (d["own_row0"], d["own_row1"])
            # shard_exchange_x's three conditions: a neighbour means halo rows here, no more rows are sent than are
            # owned, and every neighbour gets at least one
            if r > 0:
                up = shards[r - 1]["desc"]
                assert d["own_row0"] > 0 and 0 < d["send_up_rows"] <= own
                assert d["send_up_rows"] == shards[r - 1]["geom"]["H"] - up["own_row1"]   # its bottom halo
                # ... and those are the rows below the neighbour's owned ones in the joint image
                assert shards[r - 1]["rows"][0] + up["own_row1"] == sh["rows"][0] + d["own_row0"]
            else:
                assert d["own_row0"] == 0 and d["send_up_rows"] == 0
            if r + 1 < world:
                dn = shards[r + 1]["desc"]
                assert H - d["own_row1"] > 0 and 0 < d["send_down_rows"] <= own
                assert d["send_down_rows"] == dn["own_row0"]                               # its top halo
            else:
                assert d["own_row1"] == H and d["send_down_rows"] == 0
    if mode in ("channels", "grid"):
        fgs = case["frame_groups"] if mode == "grid" else 1
        coupled = any(r[0] == sm.REG_TV3D for r in case["regs"])
        for r, sh in enumerate(shards):
            d, Cl = sh["desc"], sh["geom"]["C"]
            assert (d["own_ch0"] > 0) == (coupled and r - fgs >= 0)          # a halo plane per channel neighbour
            assert (d["own_ch1"] < Cl) == (coupled and r + fgs < world)
            assert d["own_ch0"] in (0, 1) and Cl - d["own_ch1"] in (0, 1) and d["own_ch1"] > d["own_ch0"]
            if r + fgs < world and coupled:   # my last owned plane is the lower neighbour's halo plane
                assert sh["chans"][0] + d["own_ch1"] - 1 == shards[r + fgs]["chans"][0]
            assert d["frame_groups"] == (fgs if mode == "grid" else 0)
    if cid == "C3":
        assert all(sh["desc"]["own_ch0"] == 0 and sh["desc"]["own_ch1"] == sh["geom"]["C"] for sh in shards)
    if cid in ("C1", "C2", "G1"):   # a middle rank with both halo planes
        assert any(sh["desc"]["own_ch0"] == 1 and sh["desc"]["own_ch1"] < sh["geom"]["C"] for sh in shards)


def _oracle_problem(geom, lr, regs, weights):
    model = orc.ImageModel(scale=geom["s"], shifts=geom["shifts"], blur_ksize=geom["blur"], blur_sigma=geom["sigma"])
    p = orc.Problem(model, lr)
    for r, w in zip(regs, weights):
        p.set_irls_weights(p.add_regularizer(*r), w)
    return model, p


def _bands_reassemble(case, inp):
    """Oracle band problems with their halos taken from x, one after the other: (sum of the owned costs, stitched owned
    gradients) -- what the row shards compute when the halo traffic is right."""
    x, lr, wts = inp
    s = case["s"]
    f, g = 0.0, np.zeros_like(x)
    for r in range(case["world"]):
        sh = sm.shard(case, r, inp)
        model, p = _oracle_problem(sh["geom"], sh["lr"], case["regs"], sh["weights"])
        xb = sh["x_true"]
        _, gb = p.objective(xb)
        a, b = sh["cost_rows"]   # the cost of the owned rows only (srmap_problem_set_cost_rows)
        f += sum(float(np.sum((model.apply(xb, k) - sh["lr"][k])[:, a // s:b // s, :] ** 2)) for k in range(case["K"])) * s * s
        for (kind, lam, R, decay), w in zip(case["regs"], sh["weights"]):
            rv = orc.reg_values(kind, xb, R, decay)
            f += lam * float(np.sum((w * rv * rv)[:, a:b, :]))
        g[sh["own"]] = np.asarray(gb).reshape(xb.shape)[sh["own_local"]]
    return f, g


@pytest.mark.parametrize("cid", [c for c in ROWS if c != "R5"])   # R5's bands cannot reassemble: that is why it is refused
def test_row_case_halos_suffice(cid, inputs):
    """A row case that fails here has an input problem, not a kernel problem."""
    case = sm.CASES[cid]
    x, lr, wts = inputs(cid)
    geom = dict(s=case["s"], shifts=case["shifts"], blur=case["blur"], sigma=case["sigma"])
    _, whole = _oracle_problem(geom, lr, case["regs"], wts)
    f_ref, g_ref = whole.objective(x)
    f, g = _bands_reassemble(case, inputs(cid))
    assert f == pytest.approx(f_ref, rel=1e-12)
    assert np.allclose(g, np.asarray(g_ref).reshape(x.shape), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("cid", ROWS)
def test_row_case_halo_is_band_halo(cid):
    """The documented way to size a halo gives the halo of every row case -- R4's from a fractional shift, whose bands
    test_row_case_halos_suffice reassembles with the oracle."""
    case = sm.CASES[cid]
    amax = float(np.max(np.abs(case["shifts"])))
    assert srmap_dist.band_halo(case["s"], case["blur"], amax, case["reach"]) == case["halo"]


def test_band_halo_rounds_a_fractional_shift_up():
    hb = 1
    for s in (2, 3, 4):
        for shift in (0.25, 1.0, 1.5, 2.0, 2.03125, 2.75):
            need = 2 * math.ceil(shift) + 2 * hb
            assert srmap_dist.band_halo(s, 3, shift, 1) == -(-need // s) * s
            assert srmap_dist.band_halo(s, 3, -shift, 1) == srmap_dist.band_halo(s, 3, shift, 1)
    assert srmap_dist.band_halo(2, 3, 1.5, 1) == 6 and srmap_dist.band_halo(2, 3, 1, 1) == 4   # 1.5 no longer counts as 1
    assert srmap_dist.band_halo(4, 3, 3, 3) == 8 and srmap_dist.band_halo(3, 0, 1, 2) == 3      # integers as before


def test_fractional_shift_needs_the_rounded_up_halo(inputs):
    """Where rounding down was wrong: shifts of half a pixel, no blur, no regulariser.  2 * int(0.5) gave a halo of 0
    rows, although the bilinear taps of the warp read the neighbouring row; rounded up the halo is one scale step and the
    oracle's bands reassemble the whole objective.  (With a blur or a regulariser the 2 * |shift| of the formula is
    generous enough to hide the difference, which is why no caller has met it.)"""
    import error_bars as eb
    rng = np.random.default_rng(5)
    base = dict(sm.CASES["R4"], s=2, blur=0, sigma=0.0, shifts=[[0.0, 0.5], [0.5, -0.5]], regs=[], K=2, W=16, H=48, C=1, world=3)
    x, lr = eb.dyadic_inputs(rng, 2, 1, 48, 16, 2)
    inp = (x, lr, [])
    _, whole = _oracle_problem(base, lr, [], [])
    f_ref, g_ref = whole.objective(x)
    g_ref = np.asarray(g_ref).reshape(x.shape)
    good = dict(base, halo=srmap_dist.band_halo(2, 0, 0.5, 0))
    f, g = _bands_reassemble(good, inp)
    assert good["halo"] == 2 and f == pytest.approx(f_ref, rel=1e-12) and np.allclose(g, g_ref, rtol=1e-12, atol=1e-13)
    f, g = _bands_reassemble(dict(base, halo=0), inp)   # what 2 * int(0.5) gave
    assert not np.allclose(g, g_ref, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("cid", ["F1", "F2", "F3"])
def test_frame_mode_regulariser_bands(cid):
    case = sm.CASES[cid]
    H, world = case["H"], case["world"]
    raw = [sm.reg_band(H, world, r)[0] for r in range(world)]
    bands = [sm.reg_band(H, world, r)[1] for r in range(world)]
    assert all(a % 8 == 0 and b % 8 == 0 for a, b in raw)
    assert bands[0][0] == 0 and bands[-1][1] == H
    assert all(bands[r][1] == bands[r + 1][0] for r in range(world - 1)) and all(a <= b for a, b in bands)
    rows = np.zeros(H, dtype=int)
    for a, b in bands:
        rows[a:b] += 1
    assert np.all(rows == 1)
    if cid == "F1":   # tiles 13, per 5: the last band is clipped, none is empty
        assert raw == [(0, 40), (40, 80), (80, 120)] and bands[-1] == (80, 104)
    if cid == "F2":   # tiles 5, per 2: rank 2's band is clipped, rank 3's starts beyond the image and is empty
        assert raw == [(0, 16), (16, 32), (32, 48), (48, 64)] and bands[2] == (32, 40) and bands[3] == (40, 40)
    if cid == "F3":   # two regularisers: the tile kernel alone does not produce them, reg_rank evaluates both
        assert len(case["regs"]) == 2 and case["reg_rank"] == world - 1


def test_r5_bands_carry_a_per_row_warp_table():
    """The refusal is decided from problem->d_ytabs, which make_warp fills when the warpAffine y table of THIS problem's
    height is not uniform: true on every rank of R5 (forward or transposed warp), on none of R4's."""
    def nonuniform(case, rank):
        (_, _), (e0, e1) = sm.row_bands(case)[rank]
        out = False
        for dx, dy in case["shifts"]:
            for sign in (1.0, -1.0):
                _, Y = orc.warp_tables(case["W"], e1 - e0, sign * dx, sign * dy)
                out = out or not np.all(np.diff(Y) == 32)
        return out
    assert all(nonuniform(sm.CASES["R5"], r) for r in range(2))
    assert not any(nonuniform(sm.CASES["R4w2"], r) for r in range(2))
    assert not any(nonuniform(sm.CASES["R4"], r) for r in range(3))
    # an exact odd multiple of 1/64 px is resolved the same way in every row: nothing to refuse
    _, Y = orc.warp_tables(32, 52, 0.0, 17 / 64)
    assert np.all(np.diff(Y) == 32)
