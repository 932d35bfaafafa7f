"""CPU checks of the persistent prior on the data weights (include/srmap.h: srmap_set_data_prior) through its numpy
restatement (tests/data_prior_restatement.py): a validity mask that holds under a Huber loss, on the table input of
tests/flow_restatement.py with the fields and masks of tests/flow_registration_restatement.py, and the new symbols.

The pinned figures are the restatement's, with the reference's ALGLIB (oracle/_ref) as the inner minimiser, at the precision
tests/test_flow_registration_cpu.py uses; tests/test_gpu_data_prior.py and tests/test_gpu_flow_device.py compare the GPU
against them."""
import os
import re
import sys

import numpy as np
import pytest

import oracle as orc

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import data_prior_restatement as dp  # noqa: E402
import flow_registration_restatement as fq  # noqa: E402
import flow_restatement as fr  # noqa: E402
import robust_restatement as rr  # noqa: E402
import test_flow_registration_cpu as cpu  # noqa: E402

# PSNR dB (IRLS rounds, CG iterations, evaluations): m .* huber(r) on fr.table_inputs() with the estimated fields
PINNED = {
    "huber_mask0": (36.910, (7, 113, 166)),
    "huber_mask3": (37.908, (7, 139, 209)),
}

NEW_SYMBOLS = ("srmap_set_data_prior", "srmap_set_data_prior_device", "srmap_get_data_prior", "srmap_register_flow_device",
               "srmap_problem_register_flow")


@pytest.fixture(scope="module")
def table():
    return fr.table_inputs()


@pytest.fixture(scope="module")
def estimate(table):
    T = table
    flow, valid3, _ = fq.register_flow(T["y"][:, 0], hr_scale=T["s"])
    valid0 = fq.register_flow(T["y"][:, 0], hr_scale=T["s"], valid_margin=0)[1]
    return flow, valid0, valid3


def _solve(T, model, m):
    x, rep, w = dp.irls_solve(model, T["y"], rr.bilinear(T["y"][0], T["s"]), m, reg=T["reg"], delta=T["delta"])
    return orc.psnr(T["gt"], x), (rep.irls_rounds, rep.cg_iterations, rep.nfev), w


def test_the_masks_hold_under_huber(table, estimate):
    """Re-derives PINNED.  The counts and the last digits are pinned for the reference's ALGLIB (oracle/_ref); with the
    oracle's own mincg the pins are compared at 0.05 dB and the conditions still hold."""
    T = table
    flow, valid0, valid3 = estimate
    model = fr.gaussian_model(T["s"], flow, *T["blur"])
    got = {"huber_mask0": _solve(T, model, valid0[:, None]), "huber_mask3": _solve(T, model, valid3[:, None])}
    alglib = orc.have_ref()
    for name, (ps, counts, w) in got.items():
        print("%-12s %.3f dB %s (pinned %.3f dB %s)" % (name, ps, counts, PINNED[name][0], PINNED[name][1]))
    for name, (ps, counts, w) in got.items():
        assert abs(ps - PINNED[name][0]) <= (0.002 if alglib else 0.05), name
        if alglib:
            assert counts == PINNED[name][1], name
    # the mask holds: what it removes is still removed after the last re-weighting
    assert np.all(got["huber_mask0"][2][np.broadcast_to(valid0[:, None] == 0, T["y"].shape)] == 0)
    assert np.all(got["huber_mask3"][2][np.broadcast_to(valid3[:, None] == 0, T["y"].shape)] == 0)
    m0, m3 = got["huber_mask0"][0], got["huber_mask3"][0]
    print("mask0 x Huber - mask0 L2 %+.3f dB, - Huber alone %+.3f dB" %
          (m0 - cpu.PINNED["solve_mask0"][0], m0 - cpu.PINNED["solve_huber"][0]))
    assert m0 >= cpu.PINNED["solve_mask0"][0] + 0.2
    assert m0 >= cpu.PINNED["solve_huber"][0] + 2.0
    assert abs(m3 - 38.10) <= 0.5


def test_a_prior_of_ones_is_the_huber_solve_bit_for_bit():
    P = rr.prototype_inputs()
    y = P["inputs"][1][1][:, :, :24, :32]
    model = orc.ImageModel(scale=P["s"], shifts=P["shifts"], blur_ksize=3, blur_sigma=1.0)
    x0 = rr.bilinear(y[0], P["s"])
    o = orc.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = 3, 10
    a = rr.irls_solve(model, y, x0, reg=P["reg"], loss="huber", delta=P["delta"], options=o)
    b = dp.irls_solve(model, y, x0, np.ones_like(y), reg=P["reg"], delta=P["delta"], options=o)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert (a[1].irls_rounds, a[1].cg_iterations, a[1].nfev, a[1].final_cost) == (b[1].irls_rounds, b[1].cg_iterations, b[1].nfev, b[1].final_cost)
    # and a mask changes it
    m = np.ones_like(y)
    m[2] = 0.0
    c = dp.irls_solve(model, y, x0, m, reg=P["reg"], delta=P["delta"], options=o)
    assert not np.array_equal(a[0], c[0]) and np.all(c[2][2] == 0)


def test_effective_weights_and_the_plane_rule():
    rng = np.random.default_rng(3)
    m, w, r = rng.random((2, 3, 4, 5)), rng.random((2, 3, 4, 5)), rng.standard_normal((2, 3, 4, 5)) * 0.05
    assert np.array_equal(dp.effective_weights(m), m) and np.array_equal(dp.effective_weights(m, w), m * w)
    assert np.array_equal(dp.huber_prior_weights(m, r, 0.02), m * rr.huber_weights(r, 0.02))
    y = rng.random((2, 3, 4, 5))
    assert np.array_equal(dp.plane_of(y, 1), y[:, 1])
    assert np.array_equal(dp.plane_of(y, -1), ((y[:, 0] + y[:, 1]) + y[:, 2]) / 3.0)
    assert np.array_equal(dp.plane_of(y[:, :1], -1), y[:, 0])


def test_library_exports_and_header_declares_the_new_calls():
    import __graft_entry__ as ge
    ge.build_lib()
    import srmap
    lib = srmap.load()
    text = open(os.path.join(ROOT, "include", "srmap.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in srmap.EXPORTED_SYMBOLS, name
    assert re.search(r"int\s+srmap_set_data_prior\s*\(\s*srmap_problem\s*\*\s*p\s*,\s*const\s+double\s*\*\s*m_host\s*\)", code)
    assert re.search(r"int\s+srmap_problem_register_flow\s*\(\s*srmap_problem\s*\*\s*p\s*,\s*int\s+channel\s*,\s*const\s+"
                     r"srmap_flow_registration_options\s*\*\s*options\s*,\s*int\s+install_prior\s*,\s*double\s*\*\s*quality_out\s*\)", code)
    for name in ("set_data_prior", "data_prior", "register_flow"):
        assert callable(getattr(srmap.Problem, name, None)), name
    assert "a mask combined with Huber is not supported" not in text and "srmap_set_data_prior below" in text
    assert "srmap_refine_motion is future work" not in text


# ------------------------------------------------------------------------------------------- the tools' burst
def burst():
    """The 48 x 64, four-frame burst of tests/test_gpu_flow.py (generate_data --flow_motion_path), with the frames rounded
    to the float32 the tool writes: (ground truth, frames [K][1][h][w], scale)."""
    import affine_restatement as ar
    C_, H, W, s, K = 1, 48, 64, 2, 4
    rng = np.random.default_rng(21)
    gt = np.clip(0.8 * rr.prototype_ground_truth(C_, H, W) + 0.1 * rng.random((C_, H, W)), 0, 1).astype(np.float32).astype(np.float64)
    model = fr.gaussian_model(s, fr.table_fields(H, W, ar.TABLE_SHIFTS[:K]), 3, 1.0)
    frames = np.stack([model.apply(gt, k) for k in range(K)]).astype(np.float32).astype(np.float64)
    return gt, frames, s


def burst_solve(gt, frames, s, prior):
    """super_resolution --registration=flow --data_loss=huber [--flow_valid_prior] restated: 5 rounds of 30 iterations."""
    flow, valid, _ = fq.register_flow(frames[:, 0], hr_scale=s)
    o = orc.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = 5, 30
    model = fr.gaussian_model(s, flow, 3, 1.0)
    x0, reg = rr.bilinear(frames[0], s), (orc.REG_BTV, 0.005, 2, 0.5)
    if prior:
        x = dp.irls_solve(model, frames, x0, valid[:, None], reg=reg, delta=0.02, options=o)[0]
    else:
        x = rr.irls_solve(model, frames, x0, reg=reg, loss="huber", delta=0.02, options=o, composed=True)[0]
    return orc.psnr(gt, x)


# PSNR dB of the burst: Huber with the masks as prior, Huber alone
BURST_PINNED = {"huber_prior": 31.765, "huber": 31.189}


def test_the_burst_of_the_tools():
    gt, frames, s = burst()
    got = {"huber_prior": burst_solve(gt, frames, s, True), "huber": burst_solve(gt, frames, s, False)}
    print("burst: Huber x masks %.4f dB, Huber alone %.4f dB" % (got["huber_prior"], got["huber"]))
    for name, ps in got.items():
        assert abs(ps - BURST_PINNED[name]) <= (0.002 if orc.have_ref() else 0.05), name
    assert got["huber_prior"] >= got["huber"]
