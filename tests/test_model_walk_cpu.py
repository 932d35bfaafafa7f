"""tests/model_walk.py checked without the code under test: the case table is complete, the state model's algebra is
include/srmap.h's, and the numpy anchor agrees with the oracle where the oracle can express a state and with each feature
restatement it is composed from.

The fixed sequences (17 of 5 to 8 steps, 117 steps) reach NET_STATES = 71 distinct net states per base and dtype, the
doors' installed values counted by their position; the pair matrix is 31 x 31 = 961 ordered pairs per base and dtype.

Mutations of the MODEL (model_walk.MUTATIONS; no library is ever broken on purpose) and the test here that fails under
each -- test_every_mutation_of_the_model_is_caught runs them all:

  affine does not clear a flow                          test_motions_replace_one_another
  NULL to the bank call keeps custom_blur               test_null_restores_the_created_blur
  a 5 x 5 kernel leaves b = 3                           test_a_kernel_brings_its_size
  lambda0 = 0 keeps the BTV fused                       test_lambda_zero_moves_the_fused_regulariser
  new observations are not re-normalised under ...      test_new_observations_are_normalised_by_the_gains_in_force
  a new prior is not multiplied by the hold-out         test_a_new_prior_is_multiplied_by_the_holdout

On the GPU the library contradicts the first three and the last through its getters (flow(), active_impl(), the size of
blur_kernel(), data_weights()) in every test of tests/test_gpu_model_walk.py that walks the letters involved, and the
fifth through the anchor (the twin is handed the stack itself: only the anchor reads which stack the model believes was
normalised; test_the_fresh_twin_of_every_net_state_against_the_anchor, sequences photometric-observations-null and
register-lattice-under-gains).  The fourth has no getter: the model's fused_regulariser() is checked here alone, and on the
GPU a stale fused regulariser would show as the bits of an evaluation (test_fixed_sequences[lambda-zero-and-back], the
pairs with R0 and R3)."""
import numpy as np
import pytest

import oracle as orc

import model_walk as mw
from model_walk import C, H, K, S, W, h, w
from parity_log import relerr

NET_STATES = 71
ORACLE_BAR, RESTATEMENT_BAR = 1e-13, 1e-12


def final(seq, base="subpixel", dtype=0, mutation=None):
    return mw.walk_model(base, dtype, seq, mutation)[0]


# ------------------------------------------------------------------------------------------- the case table
def test_constants_match_the_binding():
    import srmap
    assert (mw.OK, mw.EINVAL, mw.EUNSUPPORTED) == (srmap.OK, srmap.EINVAL, srmap.EUNSUPPORTED)
    assert (mw.REG_TV, mw.REG_BTV, mw.TERM_DATA, mw.TERM_ALL) == (srmap.REG_TV, srmap.REG_BTV, srmap.TERM_DATA, srmap.TERM_ALL)
    assert (mw.IMPL_AUTO, mw.IMPL_DIRECT, mw.IMPL_TILED) == (srmap.IMPL_AUTO, srmap.IMPL_DIRECT, srmap.IMPL_TILED)
    assert (mw.SOLVER_CG, mw.SOLVER_LBFGS, mw.DATA_LOSS_L2, mw.DATA_LOSS_HUBER) == (srmap.SOLVER_CG, srmap.SOLVER_LBFGS, srmap.DATA_LOSS_L2, srmap.DATA_LOSS_HUBER)
    assert (mw.BLUR_PER_FRAME, mw.BLUR_PER_CHANNEL, mw.BLUR_PER_FRAME_CHANNEL) == (srmap.BLUR_PER_FRAME, srmap.BLUR_PER_CHANNEL, srmap.BLUR_PER_FRAME_CHANNEL)
    assert (orc.REG_TV, orc.REG_BTV) == (mw.REG_TV, mw.REG_BTV)
    import test_gpu_data_prior as gdp
    assert mw.INT_SHIFTS == gdp.INT_SHIFTS and mw.SUB_SHIFTS == gdp.SUB_SHIFTS


def test_the_case_table_is_complete():
    assert len(mw.PAIR_LETTERS) == 31 and len(set(mw.PAIR_LETTERS)) == 31
    assert len(mw.PAIRS) == 961 and len(set(mw.PAIRS)) == 961  # every ordered pair once (per base and dtype)
    assert not set(mw.PAIR_LETTERS) & (set(mw.DOORS) | set(mw.REFUSALS))  # doors and refusals stay out of the pair matrix
    assert len(mw.FIXED) >= 16 and all(5 <= len(s) <= 8 for s in mw.FIXED.values())
    used = {l for s in mw.FIXED.values() for l in s}
    assert used == set(mw.ALPHABET), set(mw.ALPHABET) ^ used
    # every refusal of a door and every door that runs, by the model's walk of the sequences
    refused, ran, keys = set(), set(), set()
    for seq in mw.FIXED.values():
        st = mw.State("subpixel", 0)
        for i, letter in enumerate(seq):
            if letter in mw.DOORS:
                r = st.door_refused(letter)
                (refused if r else ran).add(r or letter)
            before = st.key()
            st.apply(letter, mw.payload("subpixel"), mw.door_placeholder(letter, i) if letter in mw.DOORS else None)
            if letter in mw.REFUSALS:
                assert st.key() == before
            keys.add(st.key())
    assert refused == set(mw.DOOR_REFUSALS) and ran == set(mw.DOORS)
    assert len(keys) == NET_STATES, len(keys)
    # the cases the suite had not proven, by name
    F = mw.FIXED
    assert F["flow-affine-null-tiled"][:2] == ["Mf", "Ma"] and "It" in F["flow-affine-null-tiled"]
    assert F["kernel5-bank-null-plan"][:2] == ["B5", "Kf"] and F["kernel5-bank-null-plan"][3:5] == ["K0", "It"]
    assert [l for l in F["lambda-zero-and-back"] if l in ("R0", "R3")] == ["R0", "R3"]
    assert [l for l in F["holdout-register-lift"] if l in ("H+", "Gf", "H0")] == ["H+", "Gf", "H0"]
    assert [l for l in F["photometric-observations-null"] if l in ("P", "Y", "P0")] == ["P", "Y", "P0"]
    # a refusal in the middle of each of them (the lambda case has no refusing call of its own)
    for name in ("flow-affine-null-tiled", "kernel5-bank-null-plan", "holdout-register-lift", "photometric-observations-null"):
        st = mw.State("subpixel", 0)
        hit = False
        for i, letter in enumerate(F[name]):
            hit = hit or letter in mw.REFUSALS or (letter in mw.DOORS and st.door_refused(letter) is not None)
            st.apply(letter, mw.payload("subpixel"), mw.door_placeholder(letter, i) if letter in mw.DOORS else None)
        assert hit, name


def test_the_payloads_are_what_the_letters_say():
    import affine_restatement as ar
    import flow_restatement as fr
    P = mw.payload("tile")
    assert all(ar.deviation(m) <= ar.MAX_DEVIATION for m in P["affine"]) and ar.deviation(P["bad_affine"][2]) > ar.MAX_DEVIATION
    assert P["B3"].min() < 0 and not np.array_equal(P["B3"], P["B3"].T) and not np.array_equal(P["B3"], P["B3"][::-1, ::-1])
    assert P["B5"].shape == (5, 5) and P["Kf"].shape == (K, 3, 3) and P["Kc"].shape == (C, 5, 5) and P["Kfc"].shape == (K, C, 3, 3)
    for f in (P["flow"], P["flow2"], mw.fl.expand(P["nodes"], mw.LATTICE_STEP, H, W)):
        assert all(sum(fr.neighbour_differences(f[k])) <= fr.NEIGHBOUR_BOUND for k in range(K))  # the documented sufficient bound
    assert sum(fr.neighbour_differences(P["folded"][2])) > fr.NEIGHBOUR_BOUND and np.isnan(P["nan_flow"]).sum() == 1
    assert mw.BAND[0] % S == 0 and mw.BAND[1] % S == 0 and 0 < mw.BAND[0] < mw.BAND[1] < H
    assert not np.array_equal(P["y"], P["y2"])


# ------------------------------------------------------------------------------------------- the model's algebra
MOTIONS = {"Ma": "affine", "Mf": "flow", "Mg": "flow", "Ml": "lattice"}


def check_motions_replace_one_another(mutation=None):
    for a in MOTIONS:
        for b in MOTIONS:
            g = final([a, b], mutation=mutation).getters()
            st = final([a, b], mutation=mutation)
            assert st.motion[0] == MOTIONS[b], (a, b)
            assert (g["flow"] is not None) == (MOTIONS[b] == "flow") and (g["flow_lattice"] is not None) == (MOTIONS[b] == "lattice"), (a, b)
            assert not st.covered() and st.active_impl() == mw.IMPL_DIRECT


def check_null_restores_the_created_motion(mutation=None):
    for a in MOTIONS:
        for null in ("Ma0", "Mf0", "Ml0"):  # NULL to ANY of the three calls
            st = final([a, null], mutation=mutation)
            assert st.motion == ("created",) and st.covered() and st.active_impl() == mw.IMPL_TILED, (a, null)
            assert st.key() == final([], mutation=mutation).key()


def check_bank_and_kernel_replace_each_other(mutation=None):
    for a in ("B3", "B5"):
        for b in ("Kf", "Kc", "Kfc"):
            g = final([a, b], mutation=mutation).getters()
            assert g["blur_bank"][0] != 0 and g["blur_kernel"] == ("refused", mw.EUNSUPPORTED), (a, b)
            g = final([b, a], mutation=mutation).getters()
            assert g["blur_bank"] == (0, None) and np.array_equal(g["blur_kernel"], mw.payload("subpixel")[a]), (b, a)


def check_null_restores_the_created_blur(mutation=None):
    for a in ("B3", "B5", "Kf", "Kc", "Kfc"):
        for null in ("B0", "K0"):  # NULL on EITHER call
            st = final([a, null], mutation=mutation)
            assert st.blur == ("created",) and st.covered() and st.active_impl() == mw.IMPL_TILED, (a, null)
            assert st.getters()["blur_ksize"] == 3 and st.getters()["blur_bank"] == (0, None)


def check_a_kernel_brings_its_size(mutation=None):
    for seq, b in ((["B5"], 5), (["B3", "B5"], 5), (["B5", "B3"], 3), (["Kc"], 5), (["Kc", "Kf"], 3), (["B5", "B0"], 3)):
        st = final(seq, mutation=mutation)
        assert st.getters()["blur_ksize"] == b and st.taps_of(0, 0).shape == (b, b), seq


def check_lambda_zero_moves_the_fused_regulariser(mutation=None):
    assert final([], mutation=mutation).fused_regulariser() == 0
    assert final(["R0"], mutation=mutation).fused_regulariser() == 1 and final(["R0"], mutation=mutation).lam == [0.0, 0.02]
    assert final(["R0", "R3"], mutation=mutation).fused_regulariser() == 0 and final(["R0", "R3"], mutation=mutation).lam == [0.03, 0.02]


def check_the_independent_states_persist(mutation=None):
    head = ["P", "H+", "W", "Lh", "R0", "Cb", "It", "Y"]
    ref = final(head, mutation=mutation)
    for letter in ("Ma", "Mf", "Ml", "Ma0", "B3", "B5", "Kf", "Kc", "K0", "B0"):
        st = final(head + [letter], mutation=mutation)
        assert np.array_equal(st.photo, ref.photo) and st.hold == ref.hold and np.array_equal(st.eff, ref.eff) and st.huber, letter
        assert st.lam == ref.lam and st.rows == ref.rows and st.impl == ref.impl and st.obs == "y2", letter
    # and they are independent of one another: the order of two of them does not matter
    for a, b in (("P", "H+"), ("W", "R0"), ("Cb", "It"), ("P", "Y"), ("H+", "W"), ("Lh", "Cb")):
        assert final([a, b], mutation=mutation).key() == final([b, a], mutation=mutation).key(), (a, b)


def check_a_refusal_is_the_identity(mutation=None):
    for head in ([], ["Mf"], ["Ml", "Kf"], ["Ma", "B5", "P", "H+"]):
        ref = final(head, mutation=mutation)
        for letter in list(mw.REFUSALS) + mw.DOORS:
            st = final(head, mutation=mutation)
            if letter in mw.DOORS and st.door_refused(letter) is None:
                continue
            st.apply(letter, mw.payload("subpixel"), None)
            assert st.key() == ref.key(), (head, letter)
    assert final(["Kf"]).door_refused("Fb") == ("Fb", "bank") and final(["Kf"]).door_refused("Fp") is None and final(["Kf"]).door_refused("Fm") is None
    assert final(["Mf", "Kf"]).door_refused("Fb") == ("Fb", "bank") and final(["Kf", "Ml"]).door_refused("Fb") == ("Fb", "bank")  # the bank's comes first
    assert final(["Mf"]).door_refused("Fm") == ("Fm", "flow") and final(["Ml"]).door_refused("Fp") == ("Fp", "lattice")
    assert all(final(["Ma", "B5"]).door_refused(d) is None for d in mw.DOORS)


def check_new_observations_are_normalised_by_the_gains_in_force(mutation=None):
    import photometric_restatement as pr
    P = mw.payload("subpixel")
    for dtype in (0, 1):
        t = mw.np_dtype(dtype)
        for seq, stack in ((["P", "Y"], "y2"), (["P", "Yd"], "y2"), (["Y", "P"], "y2"), (["P"], "y")):
            got = mw.observations(final(seq, dtype=dtype, mutation=mutation), P)
            assert np.array_equal(got, pr.normalise(P[stack], P["gb"], t).astype(np.float64)), (seq, dtype)
        assert np.array_equal(mw.observations(final(["P", "Y", "P0"], dtype=dtype, mutation=mutation), P), mw.stored(P["y2"], dtype))


def check_a_new_prior_is_multiplied_by_the_holdout(mutation=None):
    import holdout_restatement as hr
    keep = 1.0 - hr.mask((K, C, h, w), *mw.HOLDOUT)
    for dtype in (0, 1):
        for seq in (["H+", "Gf"], ["Gf", "H+"], ["H+", "W", "Gl"]):
            st = final(seq, dtype=dtype, mutation=mutation)
            m = st.getters()["data_prior"]
            assert m is not None and np.any(m * keep != m)
            want = m * keep if st.user is None else mw.stored((m * keep).astype(mw.np_dtype(dtype)) * st.user.astype(mw.np_dtype(dtype)), dtype)
            assert np.array_equal(st.eff, want), seq
        # lifted: the caller's prior as it was given; without one, the weights from before
        st = final(["H+", "Gf", "H0"], dtype=dtype, mutation=mutation)
        assert np.array_equal(st.eff, st.m)
        assert final(["W", "H+", "H0"], dtype=dtype, mutation=mutation).key() == final(["W"], dtype=dtype, mutation=mutation).key()
        assert final(["H+", "H0"], dtype=dtype, mutation=mutation).eff is None


def test_motions_replace_one_another():
    check_motions_replace_one_another()


def test_null_restores_the_created_motion():
    check_null_restores_the_created_motion()


def test_bank_and_kernel_replace_each_other():
    check_bank_and_kernel_replace_each_other()


def test_null_restores_the_created_blur():
    check_null_restores_the_created_blur()


def test_a_kernel_brings_its_size():
    check_a_kernel_brings_its_size()


def test_lambda_zero_moves_the_fused_regulariser():
    check_lambda_zero_moves_the_fused_regulariser()


def test_the_independent_states_persist():
    check_the_independent_states_persist()


def test_a_refusal_is_the_identity():
    check_a_refusal_is_the_identity()


def test_new_observations_are_normalised_by_the_gains_in_force():
    check_new_observations_are_normalised_by_the_gains_in_force()


def test_a_new_prior_is_multiplied_by_the_holdout():
    check_a_new_prior_is_multiplied_by_the_holdout()


CAUGHT_BY = {
    "affine does not clear a flow": check_motions_replace_one_another,
    "NULL to the bank call keeps custom_blur": check_null_restores_the_created_blur,
    "a 5 x 5 kernel leaves b = 3": check_a_kernel_brings_its_size,
    "lambda0 = 0 keeps the BTV fused": check_lambda_zero_moves_the_fused_regulariser,
    "new observations are not re-normalised under photometric parameters": check_new_observations_are_normalised_by_the_gains_in_force,
    "a new prior is not multiplied by the hold-out": check_a_new_prior_is_multiplied_by_the_holdout,
}
ALL_CHECKS = [check_motions_replace_one_another, check_null_restores_the_created_motion, check_bank_and_kernel_replace_each_other,
              check_null_restores_the_created_blur, check_a_kernel_brings_its_size, check_lambda_zero_moves_the_fused_regulariser,
              check_the_independent_states_persist, check_a_refusal_is_the_identity,
              check_new_observations_are_normalised_by_the_gains_in_force, check_a_new_prior_is_multiplied_by_the_holdout]


@pytest.mark.parametrize("mutation", mw.MUTATIONS)
def test_every_mutation_of_the_model_is_caught(mutation):
    assert set(CAUGHT_BY) == set(mw.MUTATIONS)
    with pytest.raises(AssertionError):
        CAUGHT_BY[mutation](mutation)
    caught = []
    for check in ALL_CHECKS:
        try:
            check(mutation)
        except AssertionError:
            caught.append(check.__name__)
    print("%s: caught by %s" % (mutation, ", ".join(caught)))


# ------------------------------------------------------------------------------------------- the anchor
def rel(a, ref):
    return abs(a - ref) / max(1.0, abs(ref))


@pytest.mark.parametrize("base", sorted(mw.BASES))
def test_the_anchor_agrees_with_the_oracle_where_the_oracle_can_express_the_state(base):
    """Created motion and blur, with and without weights and a band: the data term is the oracle's operators under
    robust_restatement's weights and rows, the regularisers are the oracle's own terms; 1e-13 relative."""
    import robust_restatement as rr
    P = mw.payload(base)
    ref = orc.Problem(orc.ImageModel(scale=S, shifts=P["shifts"], blur_ksize=3, blur_sigma=1.0), P["y"])
    for kind, lam, rng_, decay in mw.REGS:
        ref.add_regularizer(kind, lam, rng_, decay)
    f_obj, g_obj = ref.objective(P["x"])
    regs = [ref.reg_term(r, P["x"]) for r in range(2)]
    for seq in ([], ["W"], ["Cb"], ["W", "Cb"], ["Cb", "Cf"]):
        st = final(seq, base=base)
        got, _ = mw.anchor(st, P)
        rows = None if st.rows == (0, H) else st.rows
        f_d, g_d = rr.weighted_data_term(P["model"], P["y"], st.eff, P["x"], True, rows)
        errs = [rel(got[mw.TERM_DATA][0], f_d), relerr(got[mw.TERM_DATA][1], g_d),
                relerr(got[mw.TERM_ALL][1], g_d + sum(g.reshape(g_d.shape) for _, g in regs))]
        if rows is None:
            errs.append(rel(got[mw.TERM_ALL][0], f_d + sum(f for f, _ in regs)))
        if not seq:
            errs += [rel(got[mw.TERM_ALL][0], f_obj), relerr(got[mw.TERM_ALL][1], g_obj.reshape(g_d.shape))]
        print("%s %s: %s" % (base, seq, " ".join("%.1e" % e for e in errs)))
        assert max(errs) <= ORACLE_BAR, (seq, errs)
    # the regularisers' cost under a band: three bands that tile the image add up to the oracle's whole terms
    parts = []
    for rows in ((0, mw.BAND[0]), mw.BAND, (mw.BAND[1], H)):
        st = final([], base=base)
        st.rows = rows
        got, _ = mw.anchor(st, P)
        parts.append(got[mw.TERM_ALL][0] - got[mw.TERM_DATA][0])
    assert rel(sum(parts), sum(f for f, _ in regs)) <= ORACLE_BAR
    # lambda 0 drops the term
    got, _ = mw.anchor(final(["R0"], base=base), P)
    assert rel(got[mw.TERM_ALL][0] - got[mw.TERM_DATA][0], regs[1][0]) <= ORACLE_BAR


@pytest.mark.parametrize("dtype", [0, 1])
def test_the_anchor_agrees_with_each_restatement_it_is_composed_from(dtype):
    import affine_restatement as ar
    import blur_bank_restatement as bb
    import blur_kernel_restatement as bk
    import flow_restatement as fr
    import holdout_restatement as hr
    import photometric_restatement as pr
    import robust_restatement as rr
    import srmap
    P = mw.payload("subpixel")
    t = mw.np_dtype(dtype)
    y, x = mw.stored(P["y"], dtype), P["x"]
    motion = ("shifts", P["shifts"])
    cases = [
        ("affine", ["Ma"], ar.AffineImageModel(S, P["affine"], 3, 1.0), y, None),
        ("flow", ["Mf"], fr.gaussian_model(S, P["flow"], 3, 1.0, t), y, None),
        ("lattice", ["Ml"], fr.gaussian_model(S, srmap.flow_lattice_expand(P["nodes"], mw.LATTICE_STEP, H, W, dtype), 3, 1.0, t), y, None),
        ("kernel", ["B5"], bk.BlurKernelModel(S, K, H, W, P["B5"], motion), y, None),
        ("bank", ["Kf"], bb.BlurBankModel(S, K, C, H, W, P["Kf"], bb.PER_FRAME, motion), y, None),
        ("photometric", ["P", "Y"], P["model"], pr.normalise(P["y2"], P["gb"], t).astype(np.float64), None),
        ("hold-out", ["H+"], P["model"], y, 1.0 - hr.mask(y.shape, *mw.HOLDOUT)),
        ("weights under Huber", ["W", "Lh"], P["model"], y, mw.stored(P["weights"], dtype)),
        ("affine, a per-channel bank and a band", ["Ma", "Kc", "Cb"], bb.BlurBankModel(S, K, C, H, W, P["Kc"], bb.PER_CHANNEL, ("affine", P["affine"])), y, None),
    ]
    for name, seq, model, yy, wts in cases:
        st = final(seq, dtype=dtype)
        got, mine = mw.anchor(st, P)
        rows = None if st.rows == (0, H) else st.rows
        f, g = rr.weighted_data_term(model, yy, wts, x, True, rows)
        ea = max(relerr(mine.apply(x, k), model.apply(x, k)) for k in range(K))
        errs = (rel(got[mw.TERM_DATA][0], f), relerr(got[mw.TERM_DATA][1], g), ea)
        print("f%d %s: cost %.1e gradient %.1e apply %.1e" % ((32 if dtype else 64, name) + errs))
        assert max(errs) <= RESTATEMENT_BAR, (name, errs)
