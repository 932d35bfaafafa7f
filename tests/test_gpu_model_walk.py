"""The model-state walk on the GPU (tests/model_walk.py: the alphabet, the state model, the twin builder, the anchor): a
long-lived problem taken through sequences of its model setters (include/srmap.h: motion, blur, photometric parameters,
observations, hold-out, data weights and loss, lambdas, implementation, cost rows, and the fits and registrations that
install a model through their apply leg) against a FRESH problem that is handed the net state once.

After EVERY step: the getters equal the Python model bit for bit and the fresh twin's; srmap_eval (TERM_ALL, TERM_DATA),
srmap_apply and srmap_apply_transpose (frames 0 and K - 1) give the twin's bits, or the same SRMAP_EUNSUPPORTED exactly
where the model says the tile family does not cover the state under SRMAP_IMPL_TILED.  A refused call answers the status
include/srmap.h documents, leaves a message that names the call, and leaves the evaluation's bits as they were.

Bars.  Bits everywhere (the kernels are fixed-order and atomic-free; an apply leg returns the doubles it installs) but in
test_the_fresh_twin_of_every_net_state_against_the_anchor: the numpy anchor at the bars of tests/test_gpu_affine.py,
test_gpu_blur_kernel.py and test_gpu_blur_bank.py, 1e-12 (f64) and 2e-5 (f32) relative to max(1, |reference|).

Shapes: LR 17 x 23, scale 2, K = 4, C = 2 (HR 34 x 46), both bases of model_walk.BASES, both dtypes.  961 ordered pairs per
base and dtype in 31 tests of 31 pairs; 17 fixed sequences; 3 seeded walks of 60 steps per base and dtype
(SRMAP_WALK_STEPS lengthens them)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_walk as mw  # noqa: E402
from parity_log import relerr  # noqa: E402

pytestmark = pytest.mark.gpu

WALK_STEPS = int(os.environ.get("SRMAP_WALK_STEPS", "60"))
WALK_SEEDS = [11, 12, 13]


@pytest.fixture(autouse=True)
def collected():
    """srmap_live_allocations() counts the whole process: problems of earlier test modules that wait in reference cycles
    (a pytest.raises record holds its frame) are collected HERE, not in the middle of a sequence that counts allocations."""
    import gc
    gc.collect()


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    c = sr.Context(0)
    p = mw.create(sr, c, "tile", sr.F32, mw.payload("tile"))  # the context's pinned staging exists from here on
    mw.destroy(sr, p)
    return c


@pytest.fixture(scope="module")
def payloads():
    import torch
    return {base: mw.device_payload(mw.payload(base), torch) for base in mw.BASES}


# ------------------------------------------------------------------------------------------- 1. pairs
@pytest.mark.parametrize("first", mw.PAIR_LETTERS)
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("base", sorted(mw.BASES))
def test_every_ordered_pair_of_setters(sr, ctx, payloads, base, dtype, first):
    for a, b in mw.PAIRS:
        if a == first:
            mw.run_sequence(sr, ctx, base, dtype, [a, b], payloads[base], tag="pair")


# ------------------------------------------------------------------------------------------- 2. fixed sequences
@pytest.mark.parametrize("name", list(mw.FIXED))
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("base", sorted(mw.BASES))
def test_fixed_sequences(sr, ctx, payloads, base, dtype, name):
    mw.run_sequence(sr, ctx, base, dtype, mw.FIXED[name], payloads[base], solves=True, tag=name)


# ------------------------------------------------------------------------------------------- 3. seeded random walks
@pytest.mark.parametrize("seed", WALK_SEEDS)
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("base", sorted(mw.BASES))
def test_seeded_random_walks(sr, ctx, payloads, base, dtype, seed):
    """A regression test, not a lottery: the letters of a seed are the same in every run."""
    rng = np.random.default_rng(seed * 1000 + 10 * len(base) + dtype)
    seq = [mw.ALPHABET[int(i)] for i in rng.integers(0, len(mw.ALPHABET), WALK_STEPS)]
    mw.run_sequence(sr, ctx, base, dtype, seq, payloads[base], tag="walk %d" % seed)


# ------------------------------------------------------------------------------------------- 4. the anchor
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("base", sorted(mw.BASES))
def test_the_fresh_twin_of_every_net_state_against_the_anchor(sr, ctx, payloads, base, dtype):
    """Twin and walked problem must not be wrong alike: the fresh twin of every distinct net state the fixed sequences
    reach against the numpy anchor.  The states are collected by walking the sequences (the doors' values are the
    library's); a state whose evaluation SRMAP_IMPL_TILED refuses is evaluated under SRMAP_IMPL_AUTO, which the model
    says runs the same direct kernels."""
    import copy
    import test_model_walk_cpu as cpu
    P = payloads[base]
    states = {}
    for name, seq in mw.FIXED.items():
        p = mw.create(sr, ctx, base, dtype, P)
        st = mw.State(base, dtype)
        for i, letter in enumerate(seq):
            mw.step(sr, p, st, letter, P, "%s step %d" % (name, i))
            net = copy.deepcopy(st)
            if net.tiled_refused():
                net.impl = mw.IMPL_AUTO
            states.setdefault(net.key(), net)
        mw.destroy(sr, p)
    assert 40 <= len(states) <= cpu.NET_STATES, len(states)  # equal fits from equal states coincide, as do TILED and AUTO where refused
    worst = {"cost": 0.0, "gradient": 0.0, "apply": 0.0, "apply_transpose": 0.0}
    for st in states.values():
        ref, model = mw.anchor(st, P)
        q = mw.twin(sr, ctx, st, P)
        for terms in (mw.TERM_ALL, mw.TERM_DATA):
            f, g = q.eval(P["x"], terms)
            worst["cost"] = max(worst["cost"], abs(f - ref[terms][0]) / max(1.0, abs(ref[terms][0])))
            worst["gradient"] = max(worst["gradient"], relerr(g, ref[terms][1]))
        for k in (0, mw.K - 1):
            worst["apply"] = max(worst["apply"], relerr(q.apply(P["x"], k), model.apply(P["x"], k)))
            worst["apply_transpose"] = max(worst["apply_transpose"], relerr(q.apply_transpose(P["r"], k), model.apply_transpose(P["r"], k)))
        mw.destroy(sr, q)
        assert max(worst.values()) <= mw.BAR[dtype], (st.motion[0], st.blur[0], st.photo is not None, st.hold, st.huber, st.lam, st.rows, st.impl, worst)
    print("%s f%d: %d net states; largest deviation from the anchor: %s (bar %.0e)"
          % (base, 32 if dtype else 64, len(states), " ".join("%s %.2e" % kv for kv in worst.items()), mw.BAR[dtype]))


# ------------------------------------------------------------------------------------------- 5. refusals
# (the state the call is made in, the call)
REFUSED_IN = [([], "xAdom"), (["Mf"], "xAdom"), ([], "xAnan"), (["Ma", "B5"], "xAnan"), ([], "xFfold"), (["Ma"], "xFfold"),
              (["Ml"], "xFnan"), ([], "xFnan"), ([], "xB9"), (["Kf"], "xB9"), (["B5"], "xB4"), ([], "xBinf"), (["Kc"], "xBinf"),
              ([], "xKmode"), (["B3"], "xKmode"), (["Kf"], "Fb"), (["Kfc", "P"], "Fb"), (["Mf", "Kfc"], "Fb"), (["Mf"], "Fm"), (["Mf"], "Fb"), (["Mg"], "Fp"),
              (["Ml"], "Fm"), (["Ml"], "Fb"), (["Ml", "H+"], "Fp")]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("base", sorted(mw.BASES))
def test_refusals_answer_the_documented_status_and_change_nothing(sr, ctx, payloads, base, dtype):
    """model_walk.step makes the three checks of a refusal (status, a message that names the call, the evaluation's bits);
    here every refusal is made in a state of its own and the getters and the twin are compared after it."""
    P = payloads[base]
    seen = set()
    for head, letter in REFUSED_IN:
        st = mw.walk_model(base, dtype, head, placeholder=False)[0]
        assert letter in mw.REFUSALS or st.door_refused(letter) is not None, (head, letter)
        seen.add(letter if letter in mw.REFUSALS else st.door_refused(letter))
        mw.run_sequence(sr, ctx, base, dtype, head + [letter, "W"], P, tag="refusal")  # and the problem goes on working
    assert seen == set(mw.REFUSALS) | set(mw.DOOR_REFUSALS)
