"""CPU checks of the dense flow registration (include/srmap.h: srmap_register_flow) through its numpy restatement
(tests/flow_registration_restatement.py): exact recovery of a translation, the table input of tests/flow_restatement.py
(endpoint errors, acceptance by the flow model, the solves with the estimated fields and the validity mask), a rotation
beyond the zero start's range, the restatement's own invariants, and the new symbols.

The pinned figures below are the restatement's, with the reference's ALGLIB (oracle/_ref) as the inner minimiser of the
solves; tests/test_gpu_flow_registration.py compares the GPU against them."""
import os
import re
import sys

import numpy as np
import pytest

import oracle as orc

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_registration_restatement as rg  # noqa: E402
import affine_restatement as ar  # noqa: E402
import flow_registration_restatement as fq  # noqa: E402
import flow_restatement as fr  # noqa: E402
import robust_restatement as rr  # noqa: E402

# mean endpoint error (HR px, >= 8 HR px from the border, frames 1...5) and the solves of fr.table_inputs():
# PSNR dB (IRLS rounds, CG iterations, evaluations)
PINNED = {
    "epe_translations": 1.420,
    "epe_clean": 0.109,
    "epe_noisy": 0.210,
    "off_margin0": 0.0375,
    "off_margin3": 0.20703125,
    "solve_l2": (32.095, (7, 136, 196)),
    "solve_huber": (34.284, (7, 169, 230)),
    "solve_mask0": (36.469, (7, 109, 161)),
    "solve_mask3": (37.863, (6, 117, 177)),
}


# ------------------------------------------------------------------------------------------- inputs
def texture(seed, H, W):
    """Smooth texture: a few sinusoids of wavelengths 9 ... 40 px with random phases and directions."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.full((H, W), 0.5)
    for lam in (9.0, 13.0, 21.0, 40.0):
        th, ph = rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        out += 0.1 * np.sin(2 * np.pi * (np.cos(th) * xx + np.sin(th) * yy) / lam + ph)
    return out


def warp_by_field(img, field):
    """I_k(q) = I_0(q + u(q)), four-tap bilinear, 0 where a tap is outside."""
    m, sx, sy = fq.inside(np.asarray(field, dtype=np.float64))
    return fq.sample((img,), m, sx, sy)[0]


def deformed_stack(H, W, n):
    """Frame 0 and n - 1 frames deformed by a sub-pixel shift plus a smooth sinusoid of amplitude 0.6 px."""
    img = texture(H * 100 + W, H, W)
    frames = [img]
    for k in range(1, n):
        f = fr.sinusoid(H, W, 0.6, 31.0 + 6 * k, offset=(0.7 * k - 1.0, 0.45 - 0.3 * k), phase=0.4 * k)
        frames.append(warp_by_field(img, f))
    return np.stack(frames)


@pytest.fixture(scope="module")
def table():
    return fr.table_inputs()


@pytest.fixture(scope="module")
def estimates(table):
    """The restatement's answers on the table's frames: noise-free, noisy (margin 3), noisy (margin 0)."""
    T = table
    clean = np.stack([T["model"].apply(T["gt"], k) for k in range(T["K"])])
    return dict(clean=fq.register_flow(clean[:, 0], hr_scale=T["s"]),
                noisy=fq.register_flow(T["y"][:, 0], hr_scale=T["s"]),
                noisy_margin0=fq.register_flow(T["y"][:, 0], hr_scale=T["s"], valid_margin=0))


# ------------------------------------------------------------------------------------------- the interface
def test_library_exports_and_header_declares_the_flow_registration():
    import __graft_entry__ as ge
    ge.build_lib()
    import srmap
    lib = srmap.load()
    text = open(os.path.join(ROOT, "include", "srmap.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+srmap_register_flow\s*\(\s*srmap_ctx\s*\*\s*ctx\s*,\s*int\s+num_images\s*,\s*int\s+width\s*,"
                     r"\s*int\s+height\s*,\s*const\s+double\s*\*\s*images_host\s*,\s*const\s+srmap_flow_registration_options\s*\*"
                     r"\s*options\s*,\s*double\s*\*\s*flow_out\s*,\s*double\s*\*\s*valid_out\s*,\s*double\s*\*\s*quality_out\s*\)", code)
    for field in ("struct_size", "hr_scale", "warps", "window_radius", "damping", "smooth_radius", "valid_margin", "max_levels",
                  "initial_affine_2x3"):
        assert field in code[code.index("srmap_affine_registration_options;"):code.index("} srmap_flow_registration_options;")]
        assert field in dict(srmap.FlowRegistrationOptions._fields_)
    for name in ("srmap_register_flow", "srmap_flow_registration_options_default"):
        assert hasattr(lib, name) and name in srmap.EXPORTED_SYMBOLS
    assert callable(getattr(srmap.Context, "register_flow", None))
    o = srmap.FlowRegistrationOptions()
    lib.srmap_flow_registration_options_default(srmap.C.byref(o))
    assert o.struct_size == srmap.C.sizeof(o)
    got = {k: getattr(o, k) for k in fq.DEFAULTS}
    assert got == fq.DEFAULTS and o.hr_scale == 1 and not o.initial_affine_2x3
    at = text.index("/* Dense flow registration")
    comment = text[at:text.index("*/", at)]
    for word in ("no reference counterpart", "NOT", "occlusion", "ONE plane", "srmap_refine_motion", "SRMAP_EINVAL", "bit-identical"):
        assert word in comment, word


# ------------------------------------------------------------------------------------------- the restatement itself
def test_window_sum_and_box_mean_against_their_definitions():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((11, 14))
    for r in (1, 2):
        direct = np.zeros_like(a)
        for y in range(a.shape[0]):
            for x in range(a.shape[1]):
                for dy in range(-2 * r, 2 * r + 1):
                    for dx in range(-2 * r, 2 * r + 1):
                        if 0 <= y + dy < a.shape[0] and 0 <= x + dx < a.shape[1]:
                            direct[y, x] += (2 * r + 1 - abs(dy)) * (2 * r + 1 - abs(dx)) * a[y + dy, x + dx]
        for order in ("stated", "permuted"):
            assert np.max(np.abs(fq.window_sum(a, r, order) - direct)) <= 1e-12 * (2 * r + 1) ** 4
    v = rng.standard_normal((2, 7, 9))
    for R in (0, 1, 3):
        direct = np.zeros_like(v)
        for y in range(7):
            for x in range(9):
                box = v[:, max(0, y - R):y + R + 1, max(0, x - R):x + R + 1]
                direct[:, y, x] = box.reshape(2, -1).mean(axis=1)
        assert np.max(np.abs(fq.box_mean(v, R) - direct)) <= 1e-14
    assert np.array_equal(fq.box_mean(v, 0), v)


def test_levels_transfer_and_output():
    assert [fq.num_levels(w, h) for w, h in ((16, 16), (31, 200), (32, 32), (47, 33), (129, 70), (1024, 1024))] == [1, 1, 2, 2, 3, 7]
    assert fq.num_levels(1024, 1024, 3) == 3 and fq.num_levels(1 << 20, 1 << 20) == fq.MAX_LEVELS
    # a linear field transfers exactly away from the clamped border: u_fine(q) = 2 u_coarse((q - 1/2) / 2)
    h, w = 9, 12
    qy, qx = fq.grid(h, w)
    u = np.stack([0.25 * qx - 0.5 * qy + 1.0, 0.125 * qy + 0.5])
    fine = fq.to_finer(u, 2 * h + 1, 2 * w)
    fy, fx = fq.grid(2 * h + 1, 2 * w)
    cx, cy = (fx - 0.5) / 2, (fy - 0.5) / 2
    expect = np.stack([2 * (0.25 * cx - 0.5 * cy + 1.0), 2 * (0.125 * cy + 0.5)])
    assert np.max(np.abs(fine - expect)[:, 1:2 * h - 1, 1:2 * w - 1]) <= 1e-13
    assert np.array_equal(fq.to_output(u, 1), u)
    U = fq.to_output(u, 3)
    assert U.shape == (2, 27, 36) and np.array_equal(U[:, ::3, ::3], 3 * u)


def test_exact_recovery_of_a_translation():
    """A constant translation on noise-free smooth texture, frame 1 sampled from frame 0's (larger) canvas with the model's
    own bilinear taps, so that e = 0 at the true field and the true field is a fixed point of the pass: interior error
    <= 1e-6 px.  The pass count is fixed and the passes converge linearly (the error falls by about 0.77 per pass on this
    texture: 8.6e-4 px after the default 8 passes per level, 1.5e-6 after 32, 1e-9 after 64), so the case runs 48."""
    H, W, pad = 64, 80, 8
    canvas = texture(3, H + 2 * pad, W + 2 * pad)
    t = np.array([1.3, -0.8])
    moved = warp_by_field(canvas, np.broadcast_to(t[:, None, None], (2,) + canvas.shape))
    stack = np.stack([canvas[pad:-pad, pad:-pad], moved[pad:-pad, pad:-pad]])
    flow, valid, q = fq.register_flow(stack, warps=48)
    err = np.max(np.abs(flow[1] - t[:, None, None])[:, 16:-16, 16:-16])
    print("largest interior error %.2e px, residual %.2e" % (err, q[1, 0]))
    assert err <= 1e-6


def test_the_table_input(table, estimates):
    T = table
    trans = fr.from_shifts(T["shifts"], T["H"], T["W"])
    K = T["K"]
    e_tr = np.mean([fq.endpoint_error(trans[k], T["fields"][k]) for k in range(1, K)])
    per = {name: [fq.endpoint_error(estimates[name][0][k], T["fields"][k]) for k in range(1, K)] for name in ("clean", "noisy")}
    print("translations %.3f, noise-free %.3f, noisy %.3f (per frame %s)" %
          (e_tr, np.mean(per["clean"]), np.mean(per["noisy"]), " ".join("%.2f" % e for e in per["noisy"])))
    assert abs(e_tr - PINNED["epe_translations"]) <= 1e-3
    assert abs(np.mean(per["clean"]) - PINNED["epe_clean"]) <= 1e-3
    assert abs(np.mean(per["noisy"]) - PINNED["epe_noisy"]) <= 1e-3
    assert np.mean(per["clean"]) <= 0.15 and np.mean(per["noisy"]) <= 0.30
    assert np.mean(per["noisy"]) <= 0.25 * e_tr
    assert abs(1 - np.mean(estimates["noisy"][1][1:]) - PINNED["off_margin3"]) <= 1e-12
    assert abs(1 - np.mean(estimates["noisy_margin0"][1][1:]) - PINNED["off_margin0"]) <= 1e-3
    assert np.array_equal(estimates["noisy"][0], estimates["noisy_margin0"][0])


def test_the_flow_model_accepts_every_estimated_field(table, estimates):
    T = table
    for name in ("clean", "noisy"):
        flow, _, q = estimates[name]
        for k in range(T["K"]):
            assert fr.classify(flow[k], T["W"], T["H"]) == "ok", (name, k)
            assert abs(q[k, 2] - sum(fr.neighbour_differences(flow[k]))) <= 1e-15
        print("%s: largest dx + dy %.3f" % (name, np.max(q[:, 2])))
        assert np.max(q[:, 2]) <= fr.NEIGHBOUR_BOUND


def test_summation_order_sensitivity_is_small(table):
    T = table
    y = T["y"][:2, 0]
    a = fq.register_flow(y, hr_scale=T["s"])
    b = fq.register_flow(y, hr_scale=T["s"], order="permuted")
    sens = float(np.max(np.abs(a[0] - b[0])))
    print("whole-run summation-order sensitivity %.2e px" % sens)
    assert sens <= 1e-8 and np.array_equal(a[1], b[1])


def _solve(T, model, **kw):
    x, rep, _ = rr.irls_solve(model, T["y"], rr.bilinear(T["y"][0], T["s"]), reg=T["reg"], composed=True, **kw)
    return orc.psnr(T["gt"], x), (rep.irls_rounds, rep.cg_iterations, rep.nfev)


def test_the_solves_with_the_estimated_fields(table, estimates):
    """Re-derives PINNED's solves.  The counts and the last digits are pinned for the reference's ALGLIB (oracle/_ref); with
    the oracle's own mincg the pins are compared at 0.05 dB and the three conditions still hold."""
    T = table
    flow, valid3, _ = estimates["noisy"]
    valid0 = estimates["noisy_margin0"][1]
    model = fr.gaussian_model(T["s"], flow, *T["blur"])
    got = {"solve_l2": _solve(T, model),
           "solve_huber": _solve(T, model, loss="huber", delta=T["delta"]),
           "solve_mask0": _solve(T, model, weights=valid0[:, None]),
           "solve_mask3": _solve(T, model, weights=valid3[:, None])}
    for name, (ps, counts) in got.items():
        print("%-12s %.3f dB %s (pinned %.3f dB %s)" % (name, ps, counts, PINNED[name][0], PINNED[name][1]))
    alglib = orc.have_ref()
    for name, (ps, counts) in got.items():
        assert abs(ps - PINNED[name][0]) <= (0.002 if alglib else 0.05), name
        if alglib:
            assert counts == PINNED[name][1], name
    masked = got["solve_mask3"][0]
    assert masked >= fr.TABLE["translation_l2"][0] + 12.0
    assert abs(masked - 38.10) <= 0.5 and abs(fr.TABLE["flow_l2"][0] - 38.10) <= 0.005
    assert masked >= got["solve_l2"][0] + 3.0


def random_texture(seed, H, W):
    """Aperiodic texture: bilinear interpolation of a random grid with nodes 8 px apart, plus a slow sinusoid."""
    rng = np.random.default_rng(seed)
    coarse = rng.random((H // 8 + 2, W // 8 + 2))
    r, c = np.arange(H) / 8.0, np.arange(W) / 8.0
    r0, c0 = r.astype(int), c.astype(int)
    a, b = (c - c0)[None, :], (r - r0)[:, None]
    g = (1 - b) * ((1 - a) * coarse[r0][:, c0] + a * coarse[r0][:, c0 + 1]) + b * ((1 - a) * coarse[r0 + 1][:, c0] + a * coarse[r0 + 1][:, c0 + 1])
    yy, xx = np.mgrid[0:H, 0:W]
    return 0.6 * g + 0.2 + 0.1 * np.sin(0.21 * xx) * np.cos(0.17 * yy)


def test_a_rotation_needs_the_affine_start():
    """4 degrees about the centre and a shift of (9.5, -6.75) px at 64 x 96, plus a 0.5 px deformation: two levels of +-1 px
    steps from u = 0 do not follow it (endpoint error above 1 px).  Started from the affine registration's matrices the
    field ends with a lower residual than the affine field alone, and than the zero start."""
    H, W = 64, 96
    img = random_texture(11, H, W)
    M = ar.rotation_about_centre(4.0, (9.5, -6.75), W, H)
    truth = fr.from_affine([M], H, W)[0] + fr.sinusoid(H, W, 0.5, 37.0)
    stack = np.stack([img, warp_by_field(img, truth)])
    mats = rg.register_affine(stack)

    def residual(field):
        valid = fq.valid_mask(field, 3)
        m, sx, sy = fq.inside(field)
        e = (fq.sample((img,), m, sx, sy)[0] - stack[1])[valid]
        return float(np.sqrt(np.mean(e * e)))

    affine_only = residual(fr.from_affine(mats, H, W)[1])
    started, _, q, _ = fq.register_pair(stack[0], stack[1], init=mats[1])
    zero, _, q0, _ = fq.register_pair(stack[0], stack[1])
    e_started, e_zero = fq.endpoint_error(started, truth), fq.endpoint_error(zero, truth)
    print("RMS residual: affine field alone %.2e, flow from the affine start %.2e, flow from zero %.2e; endpoint error %.3f / %.3f px"
          % (affine_only, q[0], q0[0], e_started, e_zero))
    assert abs(q[0] - residual(started)) <= 1e-15
    assert q[0] < affine_only
    assert q[0] < q0[0] and e_zero > 1.0
    assert e_started <= 0.1


def test_errors():
    pair = deformed_stack(16, 20, 2)
    assert fq.register_flow(np.zeros((0, 16, 16)))[0].shape == (0, 2, 16, 16)
    for kw in (dict(hr_scale=0), dict(warps=0), dict(window_radius=0), dict(window_radius=9), dict(smooth_radius=-1),
               dict(damping=-1.0), dict(valid_margin=-1), dict(max_levels=-1),
               dict(init=np.stack([ar.translation(0, 0), ar.rotation_about_centre(20.0, (0, 0), 20, 16)]))):
        with pytest.raises(fq.FlowRegistrationError):
            fq.register_flow(pair, **kw)
    with pytest.raises(fq.FlowRegistrationError):
        fq.register_flow(np.zeros((2, 15, 40)))
    bad = pair.copy()
    bad[1, 2, 3] = np.inf
    with pytest.raises(fq.FlowRegistrationError):
        fq.register_flow(bad)
