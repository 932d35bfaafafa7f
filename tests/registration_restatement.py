"""numpy restatement of the translational registration (include/srmap.h: srmap_register_translational_ex) -- the checker
of tests/test_registration_cpu.py and tests/test_gpu_registration_parity.py, written from the definition in the header
comment of csrc/registration.hip and in srmap.h, not from the kernels.

For every frame i >= 1 the shift d_i with I_i(p + d_i) ~= I_0(p) (MotionShift's convention); frame 0 gets (0, 0).

  pyramid   2 x 2 box means (an odd last row / column dropped), a level added while min(w, h) > 64, at most 12 levels
  search    coarse to fine, integer u: R0 = max(4, min(16, min side of the coarsest level / 4)) around 0 at the coarsest
            level, +-1 around twice the coarser answer on every finer one; figure of merit: the mean of
            (I_i(p + u) - I_0(p))^2 over the overlap; candidates with fewer than 0.25 w h overlapping pixels are left
            out; the first minimum in row-major candidate order wins; separation from the coarsest table
  refine    at most 20 passes at full resolution from d = the integer answer s: margin = ceil(max(|dx|, |dy|)) + 2, stop
            before a pass with fewer than 4 rows or columns inside the margin; e = I_i(p + d) - I_0(p) (bilinear at
            floor + fraction), g = central differences of I_0; S = sum (gx^2, gx gy, gy^2, gx e, gy e, e^2);
            rms = sqrt(S5 / count); det = S0 S2 - S1^2, stop unless det > 1e-12 (S0 S2 + 1e-300);
            u = -(S2 S3 - S1 S4, S0 S4 - S1 S3) / det, refused when not finite (finite pixels whose products overflow);
            d <- clamp(d + u, s - 1, s + 1); stop at |ux|, |uy| < 1e-5
  quality   (separation, rms of the last pass evaluated, -1 when none ran)

The rows of a level are summed in the library's row chunks (min(64, max(1, h / 16)) chunks of ceil(h / chunks) rows, the
trailing ones possibly empty), chunk by chunk.  `order` ("rows", "cols", "reversed") changes the order in which EVERY sum
is accumulated -- sequentially (np.cumsum; np.sum is pairwise and nearly order-blind) -- so that the restatement measures
its own summation-order sensitivity, the yardstick of the GPU bars.

The module also holds the frame generator (bilinear warp with zero border, out(q) = img(q - d): what MotionModule does)
and the case table both test files use.
"""
import functools

import numpy as np

from affine_registration_restatement import RegistrationError, down2, search_radius, search_separation  # noqa: F401

MAX_LEVELS = 12
MAX_PASSES = 20
MAX_CHUNKS = 64
MIN_OVERLAP = 0.25
TEXTURE_RTOL = 1e-12
STOP = 1e-5
ORDERS = ("rows", "cols", "reversed")


# ------------------------------------------------------------------------------------------- sums
def _seq(v, order):
    """Sequential sum of a vector, back to front for "reversed"."""
    if v.size == 0:
        return 0.0
    return float(np.cumsum(v[::-1] if order == "reversed" else v)[-1])


def total(a, order):
    """Sum of a 2-D array, every addition in sequence: row by row ("rows"), column by column ("cols"), or row by row from
    the last entry back ("reversed")."""
    if a.size == 0:
        return 0.0
    if order == "rows":
        return _seq(np.cumsum(a, axis=1)[:, -1], order)
    if order == "cols":
        return _seq(np.cumsum(a, axis=0)[-1, :], order)
    if order == "reversed":
        return _seq(np.cumsum(a[:, ::-1], axis=1)[:, -1], order)
    raise ValueError(order)


# ------------------------------------------------------------------------------------------- pyramid
def level_sizes(w, h):
    """[(w, h)] fine to coarse."""
    out = [(w, h)]
    while min(out[-1]) > 64 and len(out) < MAX_LEVELS:
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


def pyramid(img):
    out = [np.ascontiguousarray(img, dtype=np.float64)]
    for _ in level_sizes(img.shape[1], img.shape[0])[1:]:
        out.append(down2(out[-1]))
    return out


def coarsest_radius(w, h):
    return search_radius(*level_sizes(w, h)[-1])


def largest_shift(w, h):
    """The largest shift the search covers on both axes: R0 2^(L-1)."""
    return coarsest_radius(w, h) * 2 ** (len(level_sizes(w, h)) - 1)


def row_chunks(h):
    """[(r0, r1)] of the search's row chunks; r1 <= r0 for an empty trailing chunk."""
    chunks = min(MAX_CHUNKS, max(1, h // 16))
    rpc = (h + chunks - 1) // chunks
    return [(k * rpc, min(h, (k + 1) * rpc)) for k in range(chunks)]


# ------------------------------------------------------------------------------------------- integer search
def candidate_sums(a, b, ux, uy, order="rows"):
    """(sum of (b(p + u) - a(p))^2, number of pixels p with p and p + u inside), chunk by chunk."""
    h, w = a.shape
    c_lo, c_hi = max(0, -ux), min(w, w - ux)
    s, n = [], []
    for r0, r1 in row_chunks(h):
        lo, hi = max(r0, -uy), min(r1, h - uy)
        if hi <= lo or c_hi <= c_lo:
            s.append(0.0)
            n.append(0.0)
            continue
        d = b[lo + uy:hi + uy, c_lo + ux:c_hi + ux] - a[lo:hi, c_lo:c_hi]
        s.append(total(d * d, order))
        n.append(float(d.size))
    return _seq(np.array(s), order), _seq(np.array(n), order)


def search_level(a, b, cx, cy, R, order="rows"):
    """(index of the winner, msd [n1][n1] with -1 where the overlap is too small, counts [n1][n1]) of the candidates
    (cx - R + ix, cy - R + iy)."""
    h, w = a.shape
    n1 = 2 * R + 1
    msd, cnt = np.full((n1, n1), -1.0), np.zeros((n1, n1))
    best, bi = 0.0, -1
    for c in range(n1 * n1):
        iy, ix = divmod(c, n1)
        s, n = candidate_sums(a, b, cx - R + ix, cy - R + iy, order)
        cnt[iy, ix] = n
        if n < MIN_OVERLAP * w * h:
            continue
        m = s / n
        msd[iy, ix] = m
        if bi < 0 or m < best:
            best, bi = m, c
    if bi < 0:
        raise RegistrationError("Could not determine motion shift between images.")
    return bi, msd, cnt


def integer_shift(ref_pyr, img_pyr, order="rows"):
    """((sx, sy), separation, [per level, coarse to fine: dict(size, centre, R, best, second, msd, counts)])."""
    L = len(ref_pyr)
    sx = sy = 0
    sep, levels = 0.0, []
    for l in range(L - 1, -1, -1):
        a, b = ref_pyr[l], img_pyr[l]
        R = search_radius(a.shape[1], a.shape[0]) if l == L - 1 else 1
        if l != L - 1:
            sx, sy = 2 * sx, 2 * sy
        bi, msd, cnt = search_level(a, b, sx, sy, R, order)
        n1 = 2 * R + 1
        if l == L - 1:
            sep = search_separation(msd, bi)
        flat = msd.ravel()
        others = np.delete(flat, bi)
        others = others[others >= 0]
        levels.append(dict(size=a.shape, centre=(sx, sy), R=R, winner=bi, best=float(flat[bi]),
                           second=float(np.min(others)) if others.size else np.inf, msd=msd, counts=cnt))
        sx, sy = sx - R + bi % n1, sy - R + bi // n1
    return (sx, sy), sep, levels


# ------------------------------------------------------------------------------------------- refinement
def lk_sums(a, b, dx, dy, margin, order="rows"):
    """S [6] over the pixels at least `margin` from every edge."""
    h, w = a.shape
    m = margin
    ix, iy = int(np.floor(dx)), int(np.floor(dy))
    tx, ty = dx - np.floor(dx), dy - np.floor(dy)
    A = a[m:h - m, m:w - m]
    gx = 0.5 * (a[m:h - m, m + 1:w - m + 1] - a[m:h - m, m - 1:w - m - 1])
    gy = 0.5 * (a[m + 1:h - m + 1, m:w - m] - a[m - 1:h - m - 1, m:w - m])

    def tap(oy, ox):
        return b[m + iy + oy:h - m + iy + oy, m + ix + ox:w - m + ix + ox]

    v = (1.0 - ty) * ((1.0 - tx) * tap(0, 0) + tx * tap(0, 1)) + ty * ((1.0 - tx) * tap(1, 0) + tx * tap(1, 1))
    e = v - A
    return [total(t, order) for t in (gx * gx, gx * gy, gy * gy, gx * e, gy * e, e * e)]


def refine(a, b, sx, sy, order="rows"):
    """((dx, dy), rms, [per pass: dict(at, margin_arg, u, det_ratio, unclamped, clamped)])."""
    h, w = a.shape
    dx, dy, rms, passes = float(sx), float(sy), -1.0, []
    for _ in range(MAX_PASSES):
        arg = max(abs(dx), abs(dy))
        margin = int(np.ceil(arg)) + 2
        rows, cols = h - 2 * margin, w - 2 * margin
        if rows < 4 or cols < 4:
            break
        S = lk_sums(a, b, dx, dy, margin, order)
        rms = float(np.sqrt(S[5] / (float(rows) * cols)))
        det = S[0] * S[2] - S[1] * S[1]
        ratio = det / (S[0] * S[2] + 1e-300)
        rec = dict(at=(dx, dy), margin_arg=arg, u=None, det_ratio=ratio, unclamped=None, clamped=False)
        passes.append(rec)
        if not det > TEXTURE_RTOL * (S[0] * S[2] + 1e-300):
            break
        ux, uy = -(S[2] * S[3] - S[1] * S[4]) / det, -(S[0] * S[4] - S[1] * S[3]) / det
        if not (np.isfinite(ux) and np.isfinite(uy)):  # finite pixels whose products overflow
            raise RegistrationError("Could not determine motion shift between images.")
        nx, ny = dx + ux, dy + uy
        dx, dy = min(max(nx, sx - 1.0), sx + 1.0), min(max(ny, sy - 1.0), sy + 1.0)
        rec.update(u=(ux, uy), unclamped=(nx, ny), clamped=(dx != nx or dy != ny))
        if abs(ux) < STOP and abs(uy) < STOP:
            break
    return (dx, dy), rms, passes


# ------------------------------------------------------------------------------------------- whole runs
def register_translational(images, order="rows", with_trace=False):
    """images [n][H][W] -> (shifts [n][2], quality [n][2]) (and the trace: per frame dict(integer, levels, passes), None
    for frame 0)."""
    images = np.asarray(images, dtype=np.float64)
    n = images.shape[0]
    out, q, trace = np.zeros((n, 2)), np.zeros((n, 2)), [None] * n
    if n == 0:
        return (out, q, trace) if with_trace else (out, q)
    if images.shape[1] < 8 or images.shape[2] < 8:
        raise RegistrationError("registration needs images of at least 8 x 8")
    for k in range(n):
        if not np.all(np.isfinite(images[k])):
            raise RegistrationError("registration: image %d is not finite" % k)
    q[0] = [1.0, 0.0]
    ref_pyr = pyramid(images[0])
    for k in range(1, n):
        img_pyr = pyramid(images[k])
        (sx, sy), sep, levels = integer_shift(ref_pyr, img_pyr, order)
        d, rms, passes = refine(ref_pyr[0], img_pyr[0], sx, sy, order)
        out[k], q[k] = d, [sep, rms]
        trace[k] = dict(integer=(sx, sy), levels=levels, passes=passes)
    return (out, q, trace) if with_trace else (out, q)


# ------------------------------------------------------------------------------------------- frames
def texture(rng, H, W, cell=4):
    """Band-limited random texture (bilinear blow-up of a random grid of `cell` px) + two sinusoids."""
    coarse = rng.random((H // cell + 2, W // cell + 2))
    r, c = np.arange(H) / float(cell), np.arange(W) / float(cell)
    r0, c0 = r.astype(int), c.astype(int)
    a, b = (c - c0)[None, :], (r - r0)[:, None]
    g = (1 - b) * ((1 - a) * coarse[r0][:, c0] + a * coarse[r0][:, c0 + 1]) + b * ((1 - a) * coarse[r0 + 1][:, c0] + a * coarse[r0 + 1][:, c0 + 1])
    yy, xx = np.mgrid[0:H, 0:W]
    return 0.6 * g + 0.2 + 0.1 * np.sin(0.21 * xx) * np.cos(0.17 * yy)


def warp(img, d):
    """out(q) = img(q - d), bilinear, zero outside the image (MotionModule: warpAffine with a constant zero border)."""
    H, W = img.shape
    dx, dy = float(d[0]), float(d[1])
    P = int(np.ceil(max(abs(dx), abs(dy)))) + 2
    pad = np.zeros((H + 2 * P, W + 2 * P))
    pad[P:P + H, P:P + W] = img
    fx, fy = np.floor(-dx), np.floor(-dy)
    tx, ty = -dx - fx, -dy - fy
    y0, x0 = P + int(fy), P + int(fx)

    def tap(oy, ox):
        return pad[y0 + oy:y0 + oy + H, x0 + ox:x0 + ox + W]

    return (1.0 - ty) * ((1.0 - tx) * tap(0, 0) + tx * tap(0, 1)) + ty * ((1.0 - tx) * tap(1, 0) + tx * tap(1, 1))


def shifted_stack(img, shifts, noise=0.0, rng=None):
    st = np.stack([warp(img, d) for d in shifts])
    return st + noise * rng.standard_normal(st.shape) if noise else st


# ------------------------------------------------------------------------------------------- the case table
SIZES = (  # (H, W, why)
    (8, 8, "the minimum size: R0 = 4, any |d| >= 1 ends without a refinement pass"),
    (9, 11, "small and odd"),
    (12, 16, "the first size that refines a shift of 1-2"),
    (17, 23, "under one wave wide"),
    (33, 47, "small and odd"),
    (64, 64, "the level rule: one level, R0 = 16"),
    (65, 65, "the level rule: two levels, R0 = 8"),
    (70, 129, "two levels, odd halves"),
    (130, 257, "three levels, width one stride + 1"),
    (31, 255, "stride - 1, one chunk"),
    (32, 256, "one stride, two chunks"),
    (33, 257, "stride + 1, two chunks"),
    (1030, 16, "the 64-chunk cap: 17 rows per chunk, three empty trailing chunks, one level"),
    (16, 600, "three strides per row, one chunk"),
)
NOISY_SIZES = ((33, 47), (65, 65), (130, 257))
NOISE_SIGMA = 0.01
INTEGER_SHIFTS = ((0, 0), (1, 0), (0, -1), (2, -1))
SUBPIXEL_SHIFTS = ((0.5, -0.25), (-1.75, 1.5), (-3.125, 0.875), (1.25, 0.75))


def shifts_of(H, W):
    """Frame 0, the four integer shifts, the largest shift the search covers (opposite signs), the four sub-pixel ones."""
    m = largest_shift(W, H)
    return ((0, 0),) + INTEGER_SHIFTS + ((m, -m),) + SUBPIXEL_SHIFTS


def case_ids():
    return ["%dx%d" % s[:2] for s in SIZES] + ["%dx%d-noise" % s for s in NOISY_SIZES]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(H, W, noise, shifts [n][2], exact [n] (frames that are exact integer translations), stack [n][H][W]); the
    stack is built once and shared: leave it unchanged."""
    size, _, tail = name.partition("-")
    H, W = (int(v) for v in size.split("x"))
    noise = NOISE_SIGMA if tail == "noise" else 0.0
    rng = np.random.default_rng(1000 * H + W)
    img = texture(rng, H, W)
    shifts = np.array(shifts_of(H, W), dtype=np.float64)
    stack = shifted_stack(img, shifts, noise, rng)
    stack.setflags(write=False)
    exact = np.array([noise == 0.0 and float(dx).is_integer() and float(dy).is_integer() for dx, dy in shifts])
    return dict(name=name, H=H, W=W, noise=noise, shifts=shifts, exact=exact, stack=stack)


@functools.lru_cache(maxsize=None)
def restated(name):
    """{order: (shifts, quality, trace)} of a table case or a special stack, computed once."""
    stack = special(name) if name in SPECIAL else case(name)["stack"]
    return {order: register_translational(stack, order, with_trace=True) for order in ORDERS}


def sensitivity(name):
    """(shift [n], separation [n], rms [n]): the largest change of each output between the three summation orders."""
    r = restated(name)
    base = r["rows"]
    ds = np.max([np.max(np.abs(r[o][0] - base[0]), axis=1) for o in ORDERS[1:]], axis=0)
    dq = np.max([np.abs(r[o][1] - base[1]) for o in ORDERS[1:]], axis=0)
    return ds, dq[:, 0], dq[:, 1]


# ------------------------------------------------------------------------------------------- other stacks
FIVE_SHIFTS = ((0, 0), (1.25, 0.75), (-3, 2), (0.5, -0.25), (-1.75, 1.5))
FIVE_PERMUTATION = (0, 3, 1, 4, 2)
SPECIAL = ("five", "flat", "periodic", "clamp")


@functools.lru_cache(maxsize=None)
def special(name):
    if name == "five":  # one stack of 5 frames at 33 x 47
        st = shifted_stack(texture(np.random.default_rng(5), 33, 47), FIVE_SHIFTS)
    elif name == "flat":
        st = np.full((2, 64, 64), 0.5)
    elif name == "periodic":
        # period 16 px in x and y, shift (3, 2), cropped to 64 x 80 so that no zero border anchors the search.  The factors
        # come from one table per period: the frame repeats bit for bit, so candidates a period apart tie at exactly 0
        yy, xx = np.mgrid[0:128, 0:144]
        s = np.sin(2 * np.pi * np.arange(16) / 16.0)
        per = 0.5 + 0.4 * s[xx % 16] * s[yy % 16]
        st = shifted_stack(per, [(0, 0), (3, 2)])[:, 32:-32, 32:-32].copy()
    elif name == "clamp":
        # not a translation: a ramp of 0.02 per pixel under the texture and frame 1 brighter by 0.6 -- 30 px worth of ramp.
        # The search ends at the corner of its range and every refinement step wants more than a pixel beyond it: the clamp
        # to the integer answer +-1 acts in every pass, on both axes, and the pass limit ends the run
        img = texture(np.random.default_rng(0), 33, 47) + 0.02 * np.arange(47)[None, :]
        st = np.stack([img, img + 0.6])
    elif name == "overflow":
        # finite pixels, a step that is not: gradients of 1e9 against a residual of 1e300 overflow every product gx e, to
        # +inf and to -inf with the sign of gx, so S3 and S4 are NaN in any summation order while S0, S1, S2 are finite
        img = 1e10 * texture(np.random.default_rng(7), 33, 47)
        st = np.stack([img, img + 1e300])
    else:
        raise KeyError(name)
    st.setflags(write=False)
    return st
