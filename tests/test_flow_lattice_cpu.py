"""CPU checks of the displacement field on a control lattice (include/srmap.h: srmap_problem_set_flow_lattice) through its
numpy restatement (tests/flow_lattice_restatement.py): the interpolation against the registration's output rule, the
node-difference rule, the clamp, the degenerate forms, the single rounding, the ADMISSION of the lattices the GPU tests use
(tests/test_gpu_flow_lattice.py tests the library, not its inputs), the table input, the binding's own expand, and the new
symbols.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_lattice_restatement as fl  # noqa: E402
import flow_registration_restatement as fq  # noqa: E402
import flow_restatement as fr  # noqa: E402


def smooth_u(rng, h, w, amplitude=0.8):
    return np.stack([fr.smooth_random(rng, h, w, amplitude, spacing=6)[c] + off for c, off in ((0, 0.3), (1, -1.7))])


# ------------------------------------------------------------------------------------------- the interface
def test_library_exports_and_header_declares_the_lattice_calls():
    import srmap
    names = ["srmap_problem_set_flow_lattice", "srmap_problem_set_flow_lattice_device", "srmap_problem_get_flow_lattice",
             "srmap_problem_register_flow_lattice"]
    header = open(os.path.join(ROOT, "include", "srmap.h")).read()
    for n in names:
        assert n in srmap.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % n, header), n
    for attr in ("set_flow_lattice", "flow_lattice", "register_flow_lattice"):
        assert hasattr(srmap.Problem, attr)
    assert callable(srmap.flow_lattice_expand)


# ------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("scale", [1, 2, 3, 4])
def test_expand_is_the_registrations_output_rule(scale):
    """expand(s u) against to_output(u, s): the same arrays where s is a power of two (the product commutes with every
    rounding), within 1e-14 at s = 3."""
    rng = np.random.default_rng(scale)
    h, w = 19, 27
    u = smooth_u(rng, h, w)
    dense = fq.to_output(u, scale)
    mine = fl.expand(fl.nodes_from_registration(u, scale), scale, scale * h, scale * w)
    err = float(np.max(np.abs(mine - dense)))
    print("scale %d: max |expand(s u) - to_output(u, s)| = %.3e" % (scale, err))
    if scale == 3:
        assert err <= 1e-14
    else:
        assert np.array_equal(mine, dense)


@pytest.mark.parametrize("step,form", [(1, "covering"), (2, "covering"), (3, "covering"), (4, "registration"), (8, "covering")])
def test_node_difference_rule(step, form):
    """(largest node difference along x + along y) / step against max_neighbour_sum of the expanded field, to 1e-12, for
    lattices that cover the image."""
    rng = np.random.default_rng(10 + step)
    h, w, scale = 17, 23, 4
    H, W = h * scale, w * scale
    lw, lh = fl.lattice_size(form, step, h, w, scale)
    nodes = fl.random_nodes(rng, 1, lw, lh, step, [(1.5, -0.25)])[0]
    if form == "covering" and (W - 1) % step:
        # only the nodes inside the image decide the field's differences exactly; damp the overhanging ones to their neighbours
        nodes[:, :, -1] = nodes[:, :, -2]
        nodes[:, -1, :] = nodes[:, -2, :]
    got, ref = fl.node_difference_sum(nodes, step), fq.max_neighbour_sum(fl.expand(nodes, step, H, W))
    print("step %d: nodes %.15g field %.15g" % (step, got, ref))
    assert abs(got - ref) <= 1e-12


def test_the_clamp_region_is_constant():
    rng = np.random.default_rng(3)
    H, W, step, lw, lh = 40, 50, 4, 6, 5  # the last node sits at x = 20, y = 16
    nodes = fl.random_nodes(rng, 1, lw, lh, step, [(0.5, 0.5)])[0]
    U = fl.expand(nodes, step, H, W)
    x1, y1 = (lw - 1) * step, (lh - 1) * step
    assert np.array_equal(U[:, :, x1:], np.repeat(U[:, :, x1:x1 + 1], W - x1, axis=2))
    assert np.array_equal(U[:, y1:, :], np.repeat(U[:, y1:y1 + 1, :], H - y1, axis=1))
    assert np.array_equal(U[:, y1, x1], nodes[:, -1, -1])


def test_step_one_is_the_identity_and_a_step_beyond_the_image():
    rng = np.random.default_rng(4)
    H, W = 11, 14
    dense = rng.standard_normal((2, H, W))
    assert np.array_equal(fl.expand(dense, 1, H, W), dense)
    nodes = rng.standard_normal((2, 2, 2))
    U = fl.expand(nodes, 64, H, W)
    x, y = 5, 9
    fx, fy = x / 64.0, y / 64.0
    ref = (1 - fy) * ((1 - fx) * nodes[:, 0, 0] + fx * nodes[:, 0, 1]) + fy * ((1 - fx) * nodes[:, 1, 0] + fx * nodes[:, 1, 1])
    assert np.array_equal(U[:, y, x], ref)
    assert np.array_equal(U[:, 0, 0], nodes[:, 0, 0])


def test_f32_rounding_happens_once_at_the_end():
    rng = np.random.default_rng(5)
    H, W, step = 24, 30, 4
    lw, lh = fl.covering_size(W, H, step)
    nodes = fl.random_nodes(rng, 1, lw, lh, step, [(0.123456789, -3.3333333)])[0]
    d64 = fl.expand(nodes, step, H, W)
    d32 = fl.expand(nodes, step, H, W, np.float32)
    assert np.array_equal(d32, d64.astype(np.float32).astype(np.float64))
    early = fl.expand(nodes.astype(np.float32).astype(np.float64), step, H, W, np.float32)
    assert not np.array_equal(d32, early)  # rounding the nodes first is another field


def test_the_domain():
    for step, lw, lh in ((0, 4, 4), (1025, 2, 2), (4, 1, 4), (4, 4, 1), (4, 9, 4), (4, 4, 8)):
        with pytest.raises(fl.LatticeError):
            fl.check_domain(step, lw, lh, 28, 20)  # (lw - 1) step < W + step: lw <= 8, lh <= 6
    for step, lw, lh in ((4, 8, 6), (1, 28, 20), (1024, 2, 2), (4, 2, 2)):
        fl.check_domain(step, lw, lh, 28, 20)
    assert fl.covering_size(28, 20, 4) == (8, 6) and fl.covering_size(258, 140, 3) == (87, 48)


def test_the_bindings_expand_is_the_restatements():
    import srmap
    rng = np.random.default_rng(6)
    for step, H, W in ((1, 9, 11), (3, 20, 31), (8, 20, 31), (64, 20, 31)):
        lw, lh = fl.covering_size(W, H, step)
        nodes = rng.standard_normal((3, 2, lh, lw))
        for dt, npdt in ((srmap.F64, np.float64), (srmap.F32, np.float32)):
            assert np.array_equal(srmap.flow_lattice_expand(nodes, step, H, W, dt), fl.expand(nodes, step, H, W, npdt))


# ------------------------------------------------------------------------------------------- admission of the GPU tests' inputs
@pytest.mark.parametrize("case", fl.CASES, ids=lambda c: "%dx%d-s%d-step%d-%s" % c[:5])
def test_every_lattice_of_the_gpu_table_is_accepted_by_the_flow_model(case):
    h, w, scale, step, form, _, _, K = case
    H, W = h * scale, w * scale
    nodes = fl.case_nodes(h, w, scale, step, form, K)
    fl.check_domain(step, nodes.shape[3], nodes.shape[2], W, H)
    for dtype in (np.float64, np.float32):
        U = fl.expand(nodes, step, H, W, dtype)
        for k in range(K):
            assert fr.classify(U[k], W, H) == "ok", (case, k)
    # the last frame is pushed partly outside: some pixel's taps all miss the image
    sx = np.arange(W)[None, :] + fl.expand(nodes, step, H, W)[K - 1, 0]
    assert np.any(sx >= W) and np.any(sx < W - 1)


@pytest.mark.parametrize("name", sorted(fl.REFUSALS))
def test_every_refusal_case_is_refused_for_its_reason(name):
    h, w, scale, step, K = fl.REFUSAL_GEOMETRY
    H, W = h * scale, w * scale
    lw, lh = fl.covering_size(W, H, step)
    nodes = fl.refusal_nodes(name, K, lw, lh, step, W, H)
    U = fl.expand(nodes, step, H, W)
    got = [fr.classify(U[k], W, H) for k in range(K)]
    assert got == ["ok", fl.REFUSALS[name]] + ["ok"] * (K - 2), (name, got)
    if name == "steep":
        assert abs(fl.node_difference_sum(nodes[1], step) - 1.8) <= 1e-12
    if name == "huge":
        assert np.sum(np.abs(U[1]) > fr.MAX_DISPLACEMENT) >= 1


# ------------------------------------------------------------------------------------------- the table input
def test_the_registrations_lattice_on_the_table_input_is_the_dense_estimate():
    """register_pair's input-level u as a lattice (nodes = 2 u, step 2 on the LR grid) expands to the dense field the
    registration returns, bit for bit, in both dtypes: the solve figures tests/test_flow_registration_cpu.py pins for the
    dense fields are the lattice's."""
    T = fr.table_inputs()
    s = T["s"]
    for k in (1, T["K"] - 1):
        U, _, q, u = fq.register_pair(T["y"][0, 0], T["y"][k, 0], s)
        nodes = fl.nodes_from_registration(u, s)
        for dtype in (np.float64, np.float32):
            assert np.array_equal(fl.expand(nodes, s, T["H"], T["W"], dtype), fr.stored(U, dtype))
        assert abs(fl.node_difference_sum(nodes, s) - q[2]) <= 1e-12
