"""csrc/ztile_tables.hpp, the host arithmetic of the tile plan (tests/cpp/ztile_tables_test.cpp), CPU only, by brute force:
the tables are not compared with a second restatement of their construction but with what they have to MEAN, enumerated
observation by observation and pixel by pixel.

Integer plan: the thread that owns HR pixel p evaluates the residual of every observation (frame k, LR row i, LR column j)
whose z position (S i + oy_k, S j + ox_k) is p, and finds it through the slot (row phase, column phase, round) of p's
phase: LR pixel (p_row div S + io, p_col div S + jo) of frame k, at element off relative to its own cell.
Sub-pixel plan: per row phase the (frame, vertical tap) pairs of the transpose warp with a weight that land on the LR grid.
Ring rectangles: every pixel within the per-side reach of the shift range lies in exactly one of the six."""
import os
import subprocess

import numpy as np
import pytest

import tile_matrix

SCALES = (2, 3, 4)


def _run(lines):
    import __graft_entry__ as ge
    exe = ge.build_ztile_tables_test()
    assert exe and os.path.exists(exe)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stdout[-500:], out.stderr[-500:])
    rows = out.stdout.rstrip("\n").split("\n")
    assert len(rows) == len(lines)
    return [r.split() for r in rows]


def _consts():
    chunk, null, tab, maxshift = (int(t) for t in _run(["kk"])[0])
    return chunk, null, tab, maxshift


def _shift_sets(S):
    """K = 1, the S^2 phases with both signs (as tile_matrix.phase_shifts draws them), K = 17."""
    rng = np.random.default_rng(100 + S)
    return [[[-1, 2]], tile_matrix.phase_shifts(S, S, rng), [[int(v) for v in rng.integers(-S, S + 1, 2)] for _ in range(17)]]


def _sizes(S, shifts):
    """(w, h) LR: the smallest image the plan takes (W, H > 4 E + 2 S) and a few tiles (3 column tiles of 64 cells, 2 - 6 row
    tiles of 8 HR rows); H = S h is no multiple of 8 in either."""
    E = max(abs(v) for s in shifts for v in s)
    n0 = (4 * E + 2 * S) // S + 1
    while (n0 * S) % 8 == 0:
        n0 += 1
    out = [(n0, n0), (130, 11)]
    assert all((h * S) % 8 != 0 and w * S > 4 * E + 2 * S and h * S > 4 * E + 2 * S for w, h in out)
    return out


def _offsets(shifts):
    return " ".join("%d %d" % (ox, oy) for ox, oy in shifts)


class _Frame:
    """The output of `ft`, unpacked."""

    def __init__(self, S, row):
        v = [int(t) for t in row]
        assert v[0] == 1
        self.MS, self.n_ent = v[1], v[2]
        pos = [3]

        def take(n):
            a = np.array(v[pos[0]:pos[0] + n], dtype=np.int64)
            assert a.size == n
            pos[0] += n
            return a
        MS = self.MS
        self.hdr = take(S * S * 2).reshape(S, S, 2)
        self.ent = take(self.n_ent * 4).reshape(self.n_ent, 4)
        self.cnt = take(S * 8).reshape(S, 8)
        self.off = take(MS * S * S).reshape(MS, S, S)
        self.aux = take(MS * S * S * 4).reshape(MS, S, S, 4)
        self.cnt0 = take(32).reshape(4, 8)
        self.off0 = take(16).reshape(4, 4)
        self.aux0 = take(64).reshape(4, 4, 4)
        assert pos[0] == len(v)


@pytest.mark.parametrize("S", SCALES)
def test_every_in_image_observation_is_named_by_exactly_one_slot(S):
    C = 2
    cases = [(shifts, w, h) for shifts in _shift_sets(S) for w, h in _sizes(S, shifts)]
    rows = _run(["ft %d %d %d %d %d %s" % (S, C, w, h, len(shifts), _offsets(shifts)) for shifts, w, h in cases])
    for (shifts, w, h), row in zip(cases, rows):
        t = _Frame(S, row)
        W, H = S * w, S * h
        ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        named = np.zeros((len(shifts), h, w), dtype=np.int64)     # slots that name observation (k, i, j) from an in-image pixel
        at_z = np.zeros((len(shifts), h, w), dtype=np.int64)      # ... from the pixel at its z position
        for pr in range(S):
            for pc in range(S):
                n = t.cnt[pr, pc]
                assert 0 <= n <= t.MS
                for r in range(n):
                    k, io, jo, oyx = (int(x) for x in t.aux[r, pr, pc])
                    ox, oy = shifts[k]
                    assert oyx & 0xffffffff == ((oy << 16) & 0xffffffff) | (ox & 0xffff)   # the forward offset, packed
                    assert t.off[r, pr, pc] == k * C * w * h + io * w + jo
                    # the pixels of phase (pr, pc): (S rc + pr, S cell + pc) names LR pixel (rc + io, cell + jo) of frame k
                    pi, pj = S * (ii - io) + pr, S * (jj - jo) + pc   # the pixel that names observation (i, j) through this slot
                    inside = (pi >= 0) & (pi < H) & (pj >= 0) & (pj < W)
                    named[k] += inside
                    at_z[k] += inside & (pi == S * ii + oy) & (pj == S * jj + ox)
        for k, (ox, oy) in enumerate(shifts):
            zi, zj = S * ii + oy, S * jj + ox
            z_inside = (zi >= 0) & (zi < H) & (zj >= 0) & (zj < W)
            assert np.array_equal(named[k], z_inside.astype(np.int64)), (S, k, w, h)
            assert np.array_equal(at_z[k], named[k]), (S, k, w, h)
        # the counts' maximum and minimum over the column phases, the flat table of the border blocks, the by-value copies
        for pr in range(S):
            assert t.cnt[pr, S] == t.cnt[pr, :S].max() and t.cnt[pr, S + 1] == t.cnt[pr, :S].min()
            for pc in range(S):
                n, first = t.hdr[pr, pc]
                assert n == t.cnt[pr, pc]
                assert np.array_equal(t.ent[first:first + n], t.aux[:n, pr, pc])
        assert t.MS == max(1, t.cnt[:, :S].max()) and t.hdr[:, :, 0].sum() == len(shifts) == t.n_ent
        assert np.array_equal(t.cnt0[:S], t.cnt) and not t.cnt0[S:].any()
        assert np.array_equal(t.off0[:S, :S], t.off[0]) and np.array_equal(t.aux0[:S, :S], t.aux[0])


def test_the_frame_table_refuses_more_entries_than_the_border_blocks_stage():
    tab = _consts()[2]
    for K, want in ((tab, "1"), (tab + 1, "0")):
        row = _run(["ft 2 1 8 8 %d %s" % (K, _offsets([[0, 0]] * K))])[0]
        assert row[0] == want


def _warps(S, K, rng):
    """Transpose warps as problem creation leaves them: integer offsets, bilinear weights in 1/32 px; frames with one tap
    (an integer shift), with a zero x or y fraction (two taps with weight), and with four."""
    out = []
    for k in range(K):
        ox, oy = (int(v) for v in rng.integers(-S - 1, S + 2, 2))
        fx, fy = ((0, 0), (0, 7), (13, 0), (5, 29))[k % 4]
        tx, ty = fx / 32.0, fy / 32.0
        w = [(1 - ty) * (1 - tx), (1 - ty) * tx, ty * (1 - tx), ty * tx]
        out.append((ox, oy, 1 if (fx, fy) == (0, 0) else 4, w))
    return out


@pytest.mark.parametrize("S", SCALES)
def test_source_table_holds_the_weighted_taps_on_the_lr_grid_padded_with_null_records(S):
    chunk, null = _consts()[:2]
    rng = np.random.default_rng(200 + S)
    cases = [(hb, _warps(S, K, rng)) for hb in (0, 1) for K in (1, 2 * S * S, 17)]
    rows = _run(["st %d %d %d %s" % (S, hb, len(ws), " ".join("%d %d %d %s" % (ox, oy, nt, " ".join(float(x).hex() for x in w)) for ox, oy, nt, w in ws))
                 for hb, ws in cases])
    for (hb, ws), row in zip(cases, rows):
        spmax, spn = int(row[0]), [int(t) for t in row[1:5]]
        rec = [row[5 + 6 * n:11 + 6 * n] for n in range(S * spmax)]
        assert len(row) == 5 + 6 * S * spmax and spmax % chunk == 0 and spmax == max([chunk] + spn) and spn[S:] == [0] * (4 - S)
        for pr in range(S):
            want = []
            for k, (ox, oy, nt, w) in enumerate(ws):
                live = [w[t] if t < nt else 0.0 for t in range(4)]
                for dy in (0, 1):
                    w0, w1 = live[2 * dy], live[2 * dy + 1]
                    if (w0 != 0.0 or w1 != 0.0) and (pr + oy + dy) % S == 0:
                        # residual column of pixel column c (relative to the cell's first pixel) through tap dx:
                        # cell + q + e with S e = c + dx - a; the first e a cell's S + 2 hb pixels reach
                        a = (-ox) % S
                        es = [(c + dx - a) // S for c in range(-hb, S + hb) for dx in (0, 1) if (c + dx - a) % S == 0]
                        assert (ox + a) % S == 0 and min(es) in (-1, 0)
                        want.append((k, (pr + oy + dy) // S, (ox + a) // S, a | ((min(es) + 1) << 8), w0, w1))
            got = [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), float.fromhex(r[4]), float.fromhex(r[5])) for r in rec[pr * spmax:(pr + 1) * spmax]]
            assert got[:len(want)] == want, (S, hb, pr)
            assert spn[pr] == -(-len(want) // chunk) * chunk
            assert all(g[3] == null and g[4] == 0.0 and g[5] == 0.0 for g in got[len(want):]), (S, hb, pr)


@pytest.mark.parametrize("S", SCALES)
def test_every_pixel_within_the_reach_lies_in_exactly_one_ring_rectangle(S):
    cases = [(B, shifts, w * S, h * S) for B in (1, 3) for shifts in _shift_sets(S) + [[[0, 0]], [[S, S]], [[-S, -S]]]
             for w, h in _sizes(S, shifts)[:1] + [(23, 9)]]
    rows = _run(["rr %d %d %d %d %d %s" % (S, B, W, H, len(shifts), _offsets(shifts)) for B, shifts, W, H in cases])
    for (B, shifts, W, H), row in zip(cases, rows):
        ti, li, to, bo, lo, ro, count = (int(t) for t in row)
        xs, ys = [0] + [s[0] for s in shifts], [0] + [s[1] for s in shifts]
        # the reach per side, from the shift range: inside (corrections; they need a blur tap) top / left, outside top / bottom / left / right
        assert (ti, li) == ((max(ys), max(xs)) if B > 1 else (0, 0))
        assert (to, bo, lo, ro) == (max(0, -min(ys)), max(0, max(ys) - S + 1), max(0, -min(xs)), max(0, max(xs) - S + 1))
        m = max(to, bo, lo, ro) + 1
        hits = np.zeros((H + 2 * m, W + 2 * m), dtype=np.int64)   # pixel (r, c) at [r + m, c + m]
        for r0, r1, c0, c1 in ((0, ti, 0, W), (ti, H, 0, li), (-to, 0, -lo, W + ro), (H, H + bo, -lo, W + ro), (0, H, -lo, 0), (0, H, W, W + ro)):
            hits[r0 + m:r1 + m, c0 + m:c1 + m] += 1
        rr, cc = np.meshgrid(np.arange(-m, H + m), np.arange(-m, W + m), indexing="ij")
        inside = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
        within = np.where(inside, (rr < ti) | (cc < li), (rr >= -to) & (rr < H + bo) & (cc >= -lo) & (cc < W + ro))
        assert np.array_equal(hits, within.astype(np.int64)), (S, B, shifts, W, H)
        assert count == hits.sum()


def test_size_tests_of_the_plan():
    maxshift = _consts()[3]
    assert maxshift == 4096
    cases = [(W, H, reach, S) for S in SCALES for reach in (0, 1, S, 7) for W, H in
             ((4 * reach + 2 * S, 99), (4 * reach + 2 * S + 1, 4 * reach + 2 * S + 1), (99, 4 * reach + 2 * S), (99, 4 * reach + 2 * S + 1))]
    rows = _run(["ff %d %d %d %d" % c for c in cases])
    for (W, H, reach, S), row in zip(cases, rows):
        assert int(row[0]) == int(W > 4 * reach + 2 * S and H > 4 * reach + 2 * S), (W, H, reach, S)
    k1 = np.array([0.25, 0.5, 0.25])
    k2 = np.outer(k1, k1)
    lines = ["b3 %s %s" % (" ".join(float(v).hex() for v in k2.ravel()), " ".join(float(v).hex() for v in k1))]
    for i in range(9):
        if i != 4:   # the centre is free; any other tap off by one ulp breaks the symmetry
            bad = k2.ravel().copy()
            bad[i] = np.nextafter(bad[i], 1.0)
            lines.append("b3 %s %s" % (" ".join(float(v).hex() for v in bad), " ".join(float(v).hex() for v in k1)))
    lines.append("b3 %s %s" % (" ".join(float(v).hex() for v in k2.ravel()), " ".join(float(v).hex() for v in (0.25, 0.5, 0.26))))
    assert [int(r[0]) for r in _run(lines)] == [1] + [0] * 9
