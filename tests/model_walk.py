"""The model-state walk: a problem's model taken through sequences of its setters, a plain Python model of what the
library should hold after each step, a builder of the FRESH problem of that net state, and a numpy anchor of the net
state's cost and gradient (tests/test_gpu_model_walk.py runs it on the GPU; tests/test_model_walk_cpu.py checks the case
table, the model's algebra and the anchor with the oracle and the restatements alone).

Imports without a GPU: numpy, the oracle and the restatements.  The library (srmap) and torch reach the functions below
as arguments.

Bases: tests/test_gpu_data_prior.py's INT_SHIFTS ("tile") and SUB_SHIFTS ("subpixel"), LR 17 x 23, scale 2, K = 4, C = 2,
created blur 3 / sigma 1, BTV(2, 0.6) lambda 0.01 then TV lambda 0.02, observations = the forward model of
robust_restatement.prototype_ground_truth plus sigma 0.01 noise.

One letter per step (ALPHABET).  The replacement rules are include/srmap.h's: affine, flow and lattice replace one another
and NULL to any of the three calls restores the created motion; bank and single kernel replace each other and NULL on
either restores the created blur; photometric parameters, hold-out, weights, loss, lambdas, cost rows and the
implementation choice are independent and persist; a refusal changes nothing.  The data-weight part (eff / user / prior /
loss) is tests/test_gpu_weight_states.py's model with the hold-out as a factor of the prior (csrc/data_weights.hpp).

The tile family covers a state iff it has no affine motion, flow, lattice, free-form kernel or bank: the first lines of
ztile_plan (csrc/ztile_plan.hip) restated, not imported; both bases are inside its geometry.

MUTATIONS names the deliberate faults State accepts (State(..., mutation=name)); tests/test_model_walk_cpu.py lists the
test that catches each.  They live in this model only: no library is ever broken on purpose."""
import os
import sys

import numpy as np

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_restatement as ar  # noqa: E402
import blur_bank_restatement as bb  # noqa: E402
import blur_kernel_restatement as bk  # noqa: E402
import flow_lattice_restatement as fl  # noqa: E402
import flow_restatement as fr  # noqa: E402
import holdout_restatement as hr  # noqa: E402
import photometric_restatement as pr  # noqa: E402
import robust_restatement as rr  # noqa: E402

# include/srmap.h (test_model_walk_cpu.py compares them with the binding's)
OK, EINVAL, EUNSUPPORTED = 0, 1, 4
REG_TV, REG_BTV = 0, 2
TERM_DATA, TERM_ALL = 1, 3
IMPL_AUTO, IMPL_DIRECT, IMPL_TILED = 0, 1, 2
SOLVER_CG, SOLVER_LBFGS = 0, 1
DATA_LOSS_L2, DATA_LOSS_HUBER = 0, 1
BLUR_PER_FRAME, BLUR_PER_CHANNEL, BLUR_PER_FRAME_CHANNEL = 1, 2, 3

h, w, S, K, C = 17, 23, 2, 4, 2
H, W = h * S, w * S
INT_SHIFTS = [[0, 0], [1, -1], [-2, 1], [0, 2]]                          # tests/test_gpu_data_prior.py
SUB_SHIFTS = [[0.0, 0.0], [1.25, -0.75], [-0.5, 1.0], [0.3, 0.6]]
BASES = {"tile": INT_SHIFTS, "subpixel": SUB_SHIFTS}
BLUR = (3, 1.0)
REGS = [(REG_BTV, 0.01, 2, 0.6), (REG_TV, 0.02, 0, 0.0)]
LAMBDA0_BACK = 0.03
HOLDOUT = (0.1, 3)
DELTA = 0.04
BAND = (8, 20)  # multiples of the scale
LATTICE_STEP = 4
BAR = {0: 1e-12, 1: 2e-5}  # tests/test_gpu_affine.py, test_gpu_blur_kernel.py, test_gpu_blur_bank.py

MUTATIONS = ["affine does not clear a flow", "NULL to the bank call keeps custom_blur", "a 5 x 5 kernel leaves b = 3",
             "lambda0 = 0 keeps the BTV fused", "new observations are not re-normalised under photometric parameters",
             "a new prior is not multiplied by the hold-out"]

# ------------------------------------------------------------------------------------------- the alphabet
PAIR_LETTERS = ["Ma", "Mf", "Mg", "Ml", "Ma0", "Mf0", "Ml0",          # motion: affine, flow (host, device), lattice, the NULLs
                "B3", "B5", "B0", "Kf", "Kc", "Kfc", "K0",           # blur: free-form 3 / 5, NULL, the three banks, NULL
                "P", "P0", "Y", "Yd", "H+", "H0",                    # photometric, observations (host, device), hold-out
                "W", "W0", "Lh", "L2", "R0", "R3",                   # weights, loss, lambda of regulariser 0
                "Ia", "Id", "It", "Cb", "Cf"]                        # implementation, cost rows
DOORS = ["Fb", "Fp", "Fm", "Gf", "Gl"]  # fit_blur, fit_photometric, refine_motion, register_flow, register_flow_lattice
# letter -> (status, a word of srmap_last_error that names the call)
REFUSALS = {"xAdom": (EUNSUPPORTED, "affine motion"), "xAnan": (EINVAL, "affine motion"),
            "xFfold": (EUNSUPPORTED, "displacement field"), "xFnan": (EINVAL, "displacement field"),
            "xB9": (EUNSUPPORTED, "blur kernel"), "xB4": (EINVAL, "blur kernel"), "xBinf": (EINVAL, "blur kernel"),
            "xKmode": (EINVAL, "blur bank")}
# the doors that a state refuses: (door, what refuses it) -> the word of the message
DOOR_REFUSALS = {("Fb", "bank"): "blur bank", ("Fm", "flow"): "motion refinement", ("Fb", "flow"): "blur fit",
                 ("Fp", "flow"): "photometric fit", ("Fm", "lattice"): "motion refinement", ("Fb", "lattice"): "blur fit",
                 ("Fp", "lattice"): "photometric fit"}
ALPHABET = PAIR_LETTERS + DOORS + list(REFUSALS)

PAIRS = [(a, b) for a in PAIR_LETTERS for b in PAIR_LETTERS]

# name -> steps; written out by hand.  The first five are the cases the suite had not proven
FIXED = {
    "flow-affine-null-tiled": ["Mf", "Ma", "xAdom", "Ma0", "It", "Cb"],
    "kernel5-bank-null-plan": ["B5", "Kf", "Fb", "K0", "It", "W", "Cf"],
    "lambda-zero-and-back": ["R0", "It", "Cb", "R3", "W0", "Ia"],
    "holdout-register-lift": ["H+", "Gf", "Fm", "H0", "Mf0", "It"],
    "photometric-observations-null": ["P", "Y", "xBinf", "P0", "It", "Yd"],
    "lattice-refuses-the-fits": ["Ml", "Fm", "Fb", "Fp", "Ml0", "Fp", "Id"],
    "flow-refusals-then-a-fit": ["Mg", "Fb", "Fp", "xFfold", "xFnan", "Mf0", "Fb", "It"],
    "bank-modes": ["Kc", "Kfc", "xKmode", "Fp", "K0", "B3", "B0"],
    "weights-and-the-plan": ["W", "It", "Lh", "W0", "L2", "xB9", "Ia"],
    "refine-then-tiled": ["Fm", "It", "Ma0", "xAnan", "H+", "Lh", "H0"],
    "register-lattice-under-gains": ["P", "Gl", "Y", "Ml0", "P0", "H+", "It"],
    "kernel-sizes": ["B3", "B5", "xB4", "B0", "Kf", "B3", "K0"],
    "impl-around-motions": ["Id", "Ma", "Ia", "Ma0", "It", "Ml", "Ml0"],
    "holdout-weights-prior-door": ["W", "H+", "Lh", "Gf", "L2", "H0", "W0", "Mf0"],
    "fit-blur-then-bank": ["Fb", "Kfc", "B0", "Cb", "R0", "Fp", "Cf"],
    "device-inputs-under-a-band": ["Cb", "Mg", "Kc", "P", "Yd", "Mf0", "K0", "P0"],
    "motions-replace-one-another": ["Ml", "Ma", "Mf", "Ml", "Mf0", "It"],
}


def np_dtype(dtype):
    return np.float32 if dtype else np.float64


def stored(a, dtype):
    """`a` rounded once to the problem dtype, as doubles."""
    return np.asarray(a, dtype=np.float64).astype(np_dtype(dtype)).astype(np.float64)


# ------------------------------------------------------------------------------------------- the steps' payloads
_PAYLOAD = {}


def payload(base):
    """What the letters carry on `base`: host arrays only (the GPU test adds device tensors under "dev")."""
    if base in _PAYLOAD:
        return _PAYLOAD[base]
    shifts = BASES[base]
    rng = np.random.default_rng(2600 + len(base))
    model = orc.ImageModel(scale=S, shifts=shifts, blur_ksize=BLUR[0], blur_sigma=BLUR[1])
    gt = rr.prototype_ground_truth(C, H, W)
    clean = np.stack([model.apply(gt, k) for k in range(K)])
    y = clean + 0.01 * rng.standard_normal(clean.shape)
    y2 = clean + 0.01 * rng.standard_normal(clean.shape)
    x = gt + 0.02 * rng.standard_normal(gt.shape)
    flow = fr.from_shifts(SUB_SHIFTS, H, W)
    flow2 = fr.from_shifts(SUB_SHIFTS, H, W)
    for k in range(1, K):
        flow[k] += fr.sinusoid(H, W, 0.3, 23.0, phase=0.3 * k)
        flow2[k] += fr.sinusoid(H, W, 0.2, 19.0, phase=0.5 * k)
    lw, lh = fl.covering_size(W, H, LATTICE_STEP)
    g3 = bk.gaussian_taps(3, 1.0)
    g5 = bk.resize_kernel(g3, 5)
    bad_affine = np.stack([ar.translation(0.0, 0.0)] * K)
    bad_affine[2, 0, 0] = 1.3
    nan_affine = np.stack([ar.translation(0.0, 0.0)] * K)
    nan_affine[1, 1, 2] = np.nan
    folded = fr.from_shifts(SUB_SHIFTS, H, W)
    folded[2] = fr.folded(H, W)
    nan_flow = flow.copy()
    nan_flow[3, 1, 5, 7] = np.nan
    inf_taps = g3.copy()
    inf_taps[0, 2] = np.inf
    d = dict(
        base=base, shifts=shifts, model=model, gt=gt, y=y, y2=y2, x=x, x0=rr.bilinear(y[0], S), r=rng.random((C, h, w)),
        affine=np.stack([ar.rotation_about_centre(0.6 * k, (0.4 * k, -0.3 * k), W, H) for k in range(K)]),
        flow=flow, flow2=flow2,
        nodes=fl.random_nodes(np.random.default_rng(5), K, lw, lh, LATTICE_STEP, [(0.5 * k, -0.75 * k) for k in range(K)]),
        B3=np.array([[0.05, 0.10, 0.02], [0.15, 0.50, 0.10], [-0.04, 0.08, 0.04]]),  # asymmetric, one negative tap
        B5=0.6 * bk.anisotropic_psf() + 0.4 * bk.streak_psf(5),
        Kf=np.stack([g3 + 0.05 * rng.uniform(-1, 1, (3, 3)) for _ in range(K)]),
        Kc=np.stack([0.5 * g5 + 0.5 * bk.anisotropic_psf(5, 1.2 + 0.3 * c, 0.7, 0.4 + 0.5 * c) for c in range(C)]),
        Kfc=np.stack([g3 + 0.05 * rng.uniform(-1, 1, (3, 3)) for _ in range(K * C)]).reshape(K, C, 3, 3),
        gb=np.stack([np.linspace(0.9, 1.2, K), np.linspace(-0.05, 0.05, K)], axis=1),
        weights=0.5 + rng.random(y.shape),
        bad_affine=bad_affine, nan_affine=nan_affine, folded=folded, nan_flow=nan_flow,
        B9=np.full((9, 9), 1.0 / 81), B4=np.full((4, 4), 1.0 / 16), Binf=inf_taps)
    _PAYLOAD[base] = d
    return d


# ------------------------------------------------------------------------------------------- the model of the state
class State:
    """What the library should hold.  Arrays are doubles that hold values of the problem dtype where the library stores
    that dtype (flow, observations, weights, prior); taps, nodes, matrices and gains are kept as doubles."""

    def __init__(self, base, dtype, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.base, self.dtype, self.mutation = base, dtype, mutation
        self.motion = ("created",)
        self.blur = ("created",)
        self.photo = None
        self.obs = "y"
        self.obs_normalised = "y"  # which stack the normalised buffer was formed from (differs only under a mutation)
        self.hold = None
        self.eff = self.user = self.m = None
        self.huber = False
        self.lam = [r[1] for r in REGS]
        self.rows = (0, H)
        self.impl = IMPL_AUTO

    # ---- the data-weight part: tests/test_gpu_weight_states.py's Model, the hold-out a factor of the prior
    def prior_in_force(self):
        if self.m is None and self.hold is None:
            return None
        base = np.ones((K, C, h, w)) if self.m is None else self.m
        if self.hold is None or (self.mutation == "a new prior is not multiplied by the hold-out" and self.m is not None):
            return base.copy()
        return base * (1.0 - hr.mask((K, C, h, w), *self.hold))  # exact: the mask is 0 or 1

    def _product(self):
        P = self.prior_in_force()
        self.eff = P if self.user is None else stored(P.astype(np_dtype(self.dtype)) * self.user.astype(np_dtype(self.dtype)), self.dtype)

    def _ones_under_huber(self):
        if self.huber and self.eff is None:
            self.eff = np.ones((K, C, h, w))

    def _prior_changed(self, had):
        if self.prior_in_force() is None:
            if had:
                self.eff, self.user = self.user, None
                self._ones_under_huber()
            return
        if not had:
            self.user = self.eff  # the weights in force become the caller's factor
        self._product()

    def set_weights(self, wts):
        wts = None if wts is None else stored(wts, self.dtype)
        if self.prior_in_force() is not None:
            self.user = wts
            self._product()
        else:
            self.eff = wts
            self._ones_under_huber()

    def set_prior(self, m):
        had = self.prior_in_force() is not None
        self.m = None if m is None else stored(m, self.dtype)
        self._prior_changed(had)

    def set_holdout(self, hold):
        had = self.prior_in_force() is not None
        self.hold = hold
        self._prior_changed(had)

    def set_loss(self, huber):
        self.huber = huber
        self._ones_under_huber()  # back to L2 the buffer and its contents stay

    # ---- motion and blur
    def field_motion(self):
        return self.motion[0] if self.motion[0] in ("flow", "lattice") else None

    def set_motion(self, motion):
        if self.mutation == "affine does not clear a flow" and motion[0] == "affine" and self.motion[0] == "flow":
            return
        self.motion = motion

    def set_blur(self, blur, null_of_bank=False):
        if self.mutation == "NULL to the bank call keeps custom_blur" and null_of_bank and self.blur[0] != "created":
            self.blur = ("kernel", self.taps_of(0, 0))
            return
        self.blur = blur

    def set_observations(self, name):
        self.obs = name
        if not (self.mutation == "new observations are not re-normalised under photometric parameters" and self.photo is not None):
            self.obs_normalised = name

    def set_photometric(self, gb):
        self.photo = None if gb is None else np.asarray(gb, dtype=np.float64).copy()
        self.obs_normalised = self.obs

    # ---- what a door refuses in this state (None: it runs)
    def door_refused(self, letter):
        if letter == "Fb" and self.blur[0] == "bank":  # under a bank AND a field the bank's refusal comes first (csrc/blur_fit.hip)
            return (letter, "bank")
        if letter in ("Fb", "Fp", "Fm") and self.field_motion():
            return (letter, self.field_motion())
        return None

    # ---- one letter; `ret`: what a door's call returned (the values it installed)
    def apply(self, letter, P, ret=None):
        if letter in REFUSALS or (letter in DOORS and self.door_refused(letter)):
            return  # a refusal is the identity
        if letter == "Ma":
            self.set_motion(("affine", P["affine"]))
        elif letter == "Mf":
            self.set_motion(("flow", stored(P["flow"], self.dtype)))
        elif letter == "Mg":
            self.set_motion(("flow", stored(P["flow2"], self.dtype)))
        elif letter == "Ml":
            self.set_motion(("lattice", P["nodes"], LATTICE_STEP))
        elif letter in ("Ma0", "Mf0", "Ml0"):
            self.set_motion(("created",))
        elif letter in ("B3", "B5"):
            self.set_blur(("kernel", P[letter]))
        elif letter == "B0":
            self.set_blur(("created",))
        elif letter in ("Kf", "Kc", "Kfc"):
            self.set_blur(("bank", {"Kf": BLUR_PER_FRAME, "Kc": BLUR_PER_CHANNEL, "Kfc": BLUR_PER_FRAME_CHANNEL}[letter], P[letter]))
        elif letter == "K0":
            self.set_blur(("created",), null_of_bank=True)
        elif letter == "P":
            self.set_photometric(P["gb"])
        elif letter == "P0":
            self.set_photometric(None)
        elif letter in ("Y", "Yd"):
            self.set_observations("y2")
        elif letter == "H+":
            self.set_holdout(HOLDOUT)
        elif letter == "H0":
            self.set_holdout(None)
        elif letter == "W":
            self.set_weights(P["weights"])
        elif letter == "W0":
            self.set_weights(None)
        elif letter == "Lh":
            self.set_loss(True)
        elif letter == "L2":
            self.set_loss(False)
        elif letter == "R0":
            self.lam[0] = 0.0
        elif letter == "R3":
            self.lam[0] = LAMBDA0_BACK
        elif letter in ("Ia", "Id", "It"):
            self.impl = {"Ia": IMPL_AUTO, "Id": IMPL_DIRECT, "It": IMPL_TILED}[letter]
        elif letter == "Cb":
            self.rows = BAND
        elif letter == "Cf":
            self.rows = (0, H)
        elif letter == "Fb":
            if ret["installed"]:
                self.set_blur(("kernel", ret["taps"]))
        elif letter == "Fp":
            self.set_photometric(ret["gb"])
        elif letter == "Fm":
            self.set_motion(("affine", ret["matrices"]))
        elif letter == "Gf":
            self.set_motion(("flow", stored(ret["flow"], self.dtype)))
            self.set_prior(ret["prior"])
        elif letter == "Gl":
            self.set_motion(("lattice", ret["nodes"], ret["step"]))
            self.set_prior(ret["prior"])
        else:
            raise KeyError(letter)

    # ---- predictions
    def ksize(self):
        if self.blur[0] == "created":
            return BLUR[0]
        if self.mutation == "a 5 x 5 kernel leaves b = 3":
            return min(3, self.blur[-1].shape[-1])
        return self.blur[-1].shape[-1]

    def taps_of(self, k, c):
        """The taps of B_{k,c}."""
        if self.blur[0] == "created":
            return bk.gaussian_taps(*BLUR)
        if self.blur[0] == "kernel":
            return bk.resize_kernel(self.blur[1], self.ksize())
        return bb.flat_bank(self.blur[2], self.blur[1], K, C)[bb.entry_of(self.blur[1], C, k, c)]

    def covered(self):
        """Whether the tile family covers the state (the first lines of ztile_plan, restated)."""
        return self.motion[0] == "created" and self.blur[0] == "created"

    def active_impl(self):
        return IMPL_TILED if self.covered() and self.impl != IMPL_DIRECT else IMPL_DIRECT

    def tiled_refused(self):
        return self.impl == IMPL_TILED and not self.covered()

    def fused_regulariser(self):
        """The regulariser the tile plan fuses: the first with lambda > 0 (pick_fused_reg, restated); None: none."""
        for r, lam in enumerate(self.lam):
            if lam > 0 or (r == 0 and self.mutation == "lambda0 = 0 keeps the BTV fused"):
                return r
        return None

    def getters(self):
        """What every getter returns; a value None where the getter reports 'not set'."""
        bank = self.blur[0] == "bank"
        hmask = np.zeros((K, C, h, w)) if self.hold is None else hr.mask((K, C, h, w), *self.hold)
        return dict(
            flow=self.motion[1] if self.motion[0] == "flow" else None,
            flow_lattice=(self.motion[1], self.motion[2]) if self.motion[0] == "lattice" else None,
            blur_kernel=("refused", EUNSUPPORTED) if bank else self.taps_of(0, 0),
            blur_ksize=self.ksize(),
            blur_bank=(self.blur[1], bb.flat_bank(self.blur[2], self.blur[1], K, C)) if bank else (0, None),
            photometric=(self.photo if self.photo is not None else np.stack([np.ones(K), np.zeros(K)], axis=1), self.photo is not None),
            holdout=(self.hold or (0.0, None), hmask, np.concatenate([[hmask.sum()], hmask.reshape(K, -1).sum(1)])),
            data_prior=self.m, lambdas=list(self.lam), active_impl=self.active_impl())

    def key(self):
        """A hashable name of the net state (the twin builder's input)."""
        def b(a):
            return None if a is None else np.ascontiguousarray(a, dtype=np.float64).tobytes()
        return (self.base, self.dtype, self.motion[0], tuple(b(v) if isinstance(v, np.ndarray) else v for v in self.motion[1:]),
                self.blur[0], tuple(b(v) if isinstance(v, np.ndarray) else v for v in self.blur[1:]), b(self.photo), self.obs,
                self.hold, b(self.eff), b(self.user), b(self.m), self.huber, tuple(self.lam), self.rows, self.impl)


def walk_model(base, dtype, seq, mutation=None, placeholder=True):
    """The states after every step of `seq` with the model alone; a door installs a placeholder value of its kind."""
    P = payload(base)
    st = State(base, dtype, mutation)
    out = []
    for i, letter in enumerate(seq):
        st.apply(letter, P, door_placeholder(letter, i) if placeholder and letter in DOORS else None)
        out.append(st.key())
    return st, out


def door_placeholder(letter, i):
    """A value of the kind the door returns, different for every position in a sequence."""
    rng = np.random.default_rng(100 + i)
    if letter == "Fb":
        return dict(installed=True, taps=bk.gaussian_taps(3, 1.0) + 0.01 * rng.uniform(-1, 1, (3, 3)))
    if letter == "Fp":
        return dict(gb=np.stack([1.0 + 0.01 * rng.random(K), 0.01 * rng.random(K)], axis=1))
    if letter == "Fm":
        return dict(matrices=np.stack([ar.translation(*rng.uniform(-1, 1, 2)) for _ in range(K)]))
    prior = (rng.random((K, C, h, w)) < 0.9).astype(np.float64)
    if letter == "Gf":
        return dict(flow=fr.from_shifts(rng.uniform(-1, 1, (K, 2)), H, W), prior=prior)
    return dict(nodes=rng.uniform(-0.1, 0.1, (K, 2, h, w)), step=S, prior=prior)


# ------------------------------------------------------------------------------------------- the anchor
def anchor(st, P, x=None):
    """{terms: (cost, gradient)} of the net state in numpy: B_{k,c} M_k of blur_bank_restatement over the motion, the
    normalised observations of photometric_restatement, the effective weights (hold-out mask and prior included), the
    cost-row band, and the oracle's regularisers."""
    x = P["x"] if x is None else x
    t = np_dtype(st.dtype)
    if st.motion[0] == "created":
        motion = ("shifts", P["shifts"])
    elif st.motion[0] == "affine":
        motion = ("affine", st.motion[1])
    elif st.motion[0] == "flow":
        motion = ("flow", st.motion[1])
    else:
        motion = ("flow", fl.expand(st.motion[1], st.motion[2], H, W, t))
    bank = np.stack([st.taps_of(k, c) for k in range(K) for c in range(C)])
    model = bb.BlurBankModel(S, K, C, H, W, bank, bb.PER_FRAME_CHANNEL, motion)
    y = observations(st, P)
    rows = None if st.rows == (0, H) else st.rows
    f, g = rr.weighted_data_term(model, y, st.eff, x, True, rows)
    out = {TERM_DATA: (f, g.copy())}
    for (kind, _, rng_, decay), lam in zip(REGS, st.lam):
        if lam <= 0:
            continue
        vals, part = orc.reg_values_and_gradient(kind, x, np.full(x.shape, lam), rng_, decay)
        f += lam * np.sum((vals * vals)[:, st.rows[0]:st.rows[1]])
        g = g + part.reshape(g.shape)
    out[TERM_ALL] = (f, g)
    return out, model


def observations(st, P):
    """The frames the kernels read: the stack in force in the problem dtype, normalised by the gains in force."""
    t = np_dtype(st.dtype)
    if st.photo is None:
        return stored(P[st.obs], st.dtype)
    return pr.normalise(P[st.obs_normalised], st.photo, t).astype(np.float64)


# ------------------------------------------------------------------------------------------- the library side
def destroy(sr, p):
    sr.load().srmap_problem_destroy(p._h)
    p._h = None


def create(sr, ctx, base, dtype, P, observe=True):
    p = sr.Problem(ctx, W, H, C, K, S, BASES[base], BLUR[0], BLUR[1], dtype)
    if observe:
        p.set_observations(P["y"])
    for kind, lam, rng_, decay in REGS:
        p.add_regularizer(kind, lam, rng_, decay)
    return p


def outcome(sr, call):
    """("ok", value) or ("refused", status)."""
    try:
        return ("ok", call())
    except sr.SrmapError as e:
        return ("refused", e.status)


def same(a, b):
    """Bit equality of two outcomes / nested tuples of arrays and numbers."""
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def expect_refusal(sr, p, call, status, word, tag):
    before = [outcome(sr, lambda: p.eval(p._walk_x, t)) for t in (TERM_ALL, TERM_DATA)]
    try:
        call()
    except sr.SrmapError as e:
        text = sr.load().srmap_last_error(p.ctx._h).decode()
        assert e.status == status, (tag, e.status, status, str(e))
        assert text and word in text, (tag, word, text)
    else:
        raise AssertionError("%s: not refused" % tag)
    after = [outcome(sr, lambda: p.eval(p._walk_x, t)) for t in (TERM_ALL, TERM_DATA)]
    assert same(before, after), tag + ": the evaluation changed across a refused call"


def step(sr, p, st, letter, P, tag):
    """`letter` on the library problem p and on the model st."""
    dev = P["dev"][st.dtype]
    p._walk_x = P["x"]
    refused = st.door_refused(letter) if letter in DOORS else None
    ret = None
    if letter in REFUSALS:
        call = {"xAdom": lambda: p.set_affine_motion(P["bad_affine"]), "xAnan": lambda: p.set_affine_motion(P["nan_affine"]),
                "xFfold": lambda: p.set_flow(P["folded"]), "xFnan": lambda: p.set_flow(P["nan_flow"]),
                "xB9": lambda: p.set_blur_kernel(P["B9"]), "xB4": lambda: p.set_blur_kernel(P["B4"]),
                "xBinf": lambda: p.set_blur_kernel(P["Binf"]), "xKmode": lambda: p.set_blur_bank(P["Kf"], 7)}[letter]
        expect_refusal(sr, p, call, REFUSALS[letter][0], REFUSALS[letter][1], tag)
    elif refused:
        call = {"Fb": lambda: p.fit_blur(P["x"], ksize=3, apply=True), "Fp": lambda: p.fit_photometric(P["x"], apply=True),
                "Fm": lambda: p.refine_motion(P["x"], apply=True)}[letter]
        expect_refusal(sr, p, call, EUNSUPPORTED, DOOR_REFUSALS[refused], tag)
    elif letter == "Ma":
        p.set_affine_motion(P["affine"])
    elif letter == "Mf":
        p.set_flow(P["flow"])
    elif letter == "Mg":
        p.set_flow(dev["flow2"])
    elif letter == "Ml":
        p.set_flow_lattice(P["nodes"], LATTICE_STEP)
    elif letter == "Ma0":
        p.set_affine_motion(None)
    elif letter == "Mf0":
        p.set_flow(None)
    elif letter == "Ml0":
        p.set_flow_lattice(None, 0)
    elif letter in ("B3", "B5"):
        p.set_blur_kernel(P[letter])
    elif letter == "B0":
        p.set_blur_kernel(None)
    elif letter in ("Kf", "Kc", "Kfc"):
        p.set_blur_bank(P[letter], {"Kf": BLUR_PER_FRAME, "Kc": BLUR_PER_CHANNEL, "Kfc": BLUR_PER_FRAME_CHANNEL}[letter])
    elif letter == "K0":
        p.set_blur_bank(None)
    elif letter == "P":
        p.set_photometric(P["gb"])
    elif letter == "P0":
        p.set_photometric(None)
    elif letter == "Y":
        p.set_observations(P["y2"])
    elif letter == "Yd":
        p.set_observations_device(dev["y2"].data_ptr())
    elif letter == "H+":
        p.set_holdout(*HOLDOUT)
    elif letter == "H0":
        p.set_holdout(0)
    elif letter == "W":
        p.set_data_weights(P["weights"])
    elif letter == "W0":
        p.set_data_weights(None)
    elif letter == "Lh":
        p.set_data_loss(DATA_LOSS_HUBER, DELTA)
    elif letter == "L2":
        p.set_data_loss(DATA_LOSS_L2)
    elif letter == "R0":
        p.set_regularizer_lambda(0, 0.0)
    elif letter == "R3":
        p.set_regularizer_lambda(0, LAMBDA0_BACK)
    elif letter in ("Ia", "Id", "It"):
        p.set_impl({"Ia": IMPL_AUTO, "Id": IMPL_DIRECT, "It": IMPL_TILED}[letter])
    elif letter == "Cb":
        p.set_cost_rows(*BAND)
    elif letter == "Cf":
        p.set_cost_rows(0, H)
    elif letter == "Fb":
        taps, q, _ = p.fit_blur(P["x"], ksize=3, apply=True)
        ret = dict(installed=q[4] == 0.0, taps=taps)
    elif letter == "Fp":
        ret = dict(gb=p.fit_photometric(P["x"], apply=True)[0])
    elif letter == "Fm":
        ret = dict(matrices=p.refine_motion(P["x"], apply=True)[0])
    elif letter == "Gf":
        p.register_flow(prior=True)
        ret = dict(flow=p.flow(), prior=p.data_prior())  # the call returns the quality only: what it installed is read back
        assert ret["flow"] is not None and ret["prior"] is not None, tag
    elif letter == "Gl":
        p.register_flow_lattice(prior=True)
        lat = p.flow_lattice()
        assert lat is not None and p.data_prior() is not None, tag
        ret = dict(nodes=lat[0], step=lat[1], prior=p.data_prior())
    else:
        raise KeyError(letter)
    st.apply(letter, P, ret)


def twin(sr, ctx, st, P):
    """A FRESH problem handed the net state once, in one canonical order: motion, blur, photometric parameters,
    observations, prior, weights, loss, hold-out, lambdas, cost rows, implementation."""
    q = create(sr, ctx, st.base, st.dtype, P, observe=False)
    if st.motion[0] == "affine":
        q.set_affine_motion(st.motion[1])
    elif st.motion[0] == "flow":
        q.set_flow(st.motion[1])
    elif st.motion[0] == "lattice":
        q.set_flow_lattice(st.motion[1], st.motion[2])
    if st.blur[0] == "kernel":
        q.set_blur_kernel(st.blur[1])
    elif st.blur[0] == "bank":
        q.set_blur_bank(st.blur[2], st.blur[1])
    if st.photo is not None:
        q.set_photometric(st.photo)
    q.set_observations(P[st.obs])
    if st.m is not None:
        q.set_data_prior(st.m)
    wts = st.user if (st.m is not None or st.hold is not None) else st.eff
    if wts is not None:
        q.set_data_weights(wts)
    if st.huber:
        q.set_data_loss(DATA_LOSS_HUBER, DELTA)
    if st.hold is not None:
        q.set_holdout(*st.hold)
    for r, lam in enumerate(st.lam):
        if lam != REGS[r][1]:
            q.set_regularizer_lambda(r, lam)
    if st.rows != (0, H):
        q.set_cost_rows(*st.rows)
    if st.impl != IMPL_AUTO:
        q.set_impl(st.impl)
    return q


def read_getters(sr, p):
    hold = p.holdout()
    return dict(flow=p.flow(), flow_lattice=p.flow_lattice(), blur_kernel=outcome(sr, p.blur_kernel), blur_bank=p.blur_bank(),
                photometric=p.photometric(), holdout=hold, data_prior=p.data_prior(),
                lambdas=[p.regularizer_lambda(r) for r in range(len(REGS))], active_impl=p.active_impl(), data_weights=p.data_weights())


def check_getters(sr, got, st, tag):
    """The library's getters against the model, bit for bit."""
    want = st.getters()
    assert same(got["flow"], want["flow"]), tag + ": flow()"
    assert same(got["flow_lattice"], want["flow_lattice"]), tag + ": flow_lattice()"
    if isinstance(want["blur_kernel"], tuple):
        assert got["blur_kernel"] == want["blur_kernel"], tag + ": blur_kernel() under a bank"
    else:
        assert got["blur_kernel"][0] == "ok" and got["blur_kernel"][1].shape == (want["blur_ksize"],) * 2, tag + ": blur size"
        if st.blur[0] == "created":  # the library forms its own Gaussian: tests/test_gpu_blur_kernel.py's 1e-16
            assert np.max(np.abs(got["blur_kernel"][1] - want["blur_kernel"])) <= 1e-16, tag + ": created blur"
        else:
            assert np.array_equal(got["blur_kernel"][1], want["blur_kernel"]), tag + ": blur_kernel()"
    assert got["blur_bank"][0] == want["blur_bank"][0], tag + ": bank mode"
    if want["blur_bank"][0]:
        assert np.array_equal(got["blur_bank"][1].reshape(want["blur_bank"][1].shape), want["blur_bank"][1]), tag + ": blur_bank()"
    assert same(got["photometric"], want["photometric"]), tag + ": photometric()"
    (fraction, seed), hmask, counts = want["holdout"]
    assert got["holdout"][0] == fraction and (seed is None or got["holdout"][1] == seed), tag + ": holdout()"
    assert np.array_equal(got["holdout"][2], hmask) and np.array_equal(got["holdout"][3], counts), tag + ": hold-out mask"
    assert same(got["data_prior"], want["data_prior"]), tag + ": data_prior()"
    assert got["lambdas"] == want["lambdas"], tag + ": regularizer_lambda()"
    assert got["active_impl"] == want["active_impl"], tag + ": active_impl() %d, the model %d" % (got["active_impl"], want["active_impl"])
    eff = np.ones((K, C, h, w)) if st.eff is None else st.eff
    assert np.array_equal(got["data_weights"], eff), tag + ": data_weights()"


def evaluations(sr, p, P):
    """eval for TERM_ALL and TERM_DATA, apply / apply_transpose of frames 0 and K - 1: outcomes."""
    out = [outcome(sr, lambda: p.eval(P["x"], t)) for t in (TERM_ALL, TERM_DATA)]
    for k in (0, K - 1):
        out.append(outcome(sr, lambda: p.apply(P["x"], k)))
        out.append(outcome(sr, lambda: p.apply_transpose(P["r"], k)))
    return out


def check_against_twin(sr, ctx, p, st, P, tag):
    """After a step: the getters equal the model and the fresh twin's, the evaluations and operators the twin's bits or
    the same SRMAP_EUNSUPPORTED where the model says the tile family does not cover the state."""
    got = read_getters(sr, p)
    check_getters(sr, got, st, tag)
    q = twin(sr, ctx, st, P)
    try:
        fresh = read_getters(sr, q)
        for name in got:
            assert same(got[name], fresh[name]), "%s: %s differs from the fresh twin's" % (tag, name)
        a, b = evaluations(sr, p, P), evaluations(sr, q, P)
        for i, (u, v) in enumerate(zip(a, b)):
            assert same(u, v), "%s: evaluation %d differs from the fresh twin's" % (tag, i)
        for u in a[:2]:
            assert (u == ("refused", EUNSUPPORTED)) == st.tiled_refused(), "%s: %s, the model says refused = %s" % (tag, u[0], st.tiled_refused())
    finally:
        destroy(sr, q)


def short_options(sr):
    o = sr.default_irls_options()
    o.max_num_irls_iterations, o.max_num_solver_iterations = 2, 6
    return o


def solve_outcome(sr, p, P, solver):
    def run():
        p.set_solver(solver)
        x, rep = p.solve(P["x0"], short_options(sr))
        return ((rep.irls_rounds, rep.cg_iterations, rep.evaluations, rep.last_termination, rep.final_cost), x)
    return outcome(sr, run)


def run_sequence(sr, ctx, base, dtype, seq, P, solves=False, tag="", states=None):
    """`seq` on a fresh problem, a fresh twin compared after every step; solves: a short CG and a short L-BFGS solve at
    the end, report and solution in bits.  states: a dict that collects {key: a copy of the state} of every step."""
    import copy
    lib = sr.load()
    start = int(lib.srmap_live_allocations())
    p = create(sr, ctx, base, dtype, P)
    st = State(base, dtype)
    try:
        for i, letter in enumerate(seq):
            t = "%s f%d %s [%s] step %d (%s)" % (base, 32 if dtype else 64, tag, " ".join(seq), i, letter)
            step(sr, p, st, letter, P, t)
            check_against_twin(sr, ctx, p, st, P, t)
            if states is not None:
                states.setdefault(st.key(), copy.deepcopy(st))
        if solves:
            q = twin(sr, ctx, st, P)
            try:
                for solver in (SOLVER_CG, SOLVER_LBFGS):
                    a, b = solve_outcome(sr, p, P, solver), solve_outcome(sr, q, P, solver)
                    assert same(a, b), "%s f%d [%s]: solve %d differs from the fresh twin's" % (base, 32 if dtype else 64, " ".join(seq), solver)
                    assert (a == ("refused", EUNSUPPORTED)) == st.tiled_refused()
            finally:
                destroy(sr, q)
    finally:
        destroy(sr, p)
    end = int(lib.srmap_live_allocations())
    assert end == start, "%s [%s]: %d live allocations at the start, %d after both problems are destroyed" % (base, " ".join(seq), start, end)
    return st


def device_payload(P, torch):
    """The device tensors of the letters Mg and Yd, per dtype."""
    if "dev" not in P:
        P["dev"] = {}
        for dtype, tt in ((0, torch.float64), (1, torch.float32)):
            P["dev"][dtype] = {k: torch.tensor(np.ascontiguousarray(P[k]), dtype=tt, device="cuda") for k in ("flow2", "y2")}
        torch.cuda.synchronize()
    return P
