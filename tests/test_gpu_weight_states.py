"""The data-weight state of a problem (csrc/data_weights.hpp: the caller's weights w, the prior m, the loss) walked through
sequences of its setters on the GPU, against a numpy model of the state and against the library itself.

Steps: w := A (host) | B (device) | NULL, m := M (host) | M2 (device) | NULL, loss := Huber(delta) | L2, and U, one
srmap_update_data_weights_device.  Sequences: every ordered pair of the eight setters (64) and the fixed ones below.

After every step srmap_get_data_weights and srmap_get_data_prior must equal the model BIT FOR BIT: the effective weights
are m .* w formed in the problem dtype with one rounding, ones standing in for a missing factor.  At the end of a sequence
srmap_eval must give the bits of a fresh problem that was handed the effective weights as plain weights, and
srmap_live_allocations must be back where it started once both are destroyed.

The Huber step U is the one place where the model cannot give bits: the weights are m .* huber(A x - y) with the residual
of the GPU's forward kernel, which the oracle's A x reproduces to rounding only.  There the step is pinned twice: within
the bars of tests/test_gpu_robust.py (1e-12 in f64, 2e-5 in f32) of the restatement (tests/robust_restatement.py), and
bit for bit against a fresh problem that was given the same prior, the same loss and the same U; the model goes on from
those bits.

Shapes: HR 24 x 16, scale 2, 3 frames, 2 channels, sub-pixel shifts (unit weights are then bit-identical to no weights,
tests/test_gpu_robust.py), blur 3 / sigma 1, one TV regulariser; both dtypes."""
import itertools
import os
import sys

import numpy as np
import pytest

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_restatement as rr  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, S, K, C = 24, 16, 2, 3, 2
SHIFTS = [[0.0, 0.0], [1.25, -0.75], [-0.5, 1.0]]
DELTA = 0.04
HUBER_BAR = {0: 1e-12, 1: 2e-5}
SETTERS = ["wA", "wB", "w0", "mM", "mM2", "m0", "H", "L"]
PAIRS = [list(s) for s in itertools.product(SETTERS, repeat=2)]
FIXED = [["mM", "wA", "H", "m0", "w0"],
         ["H", "mM", "L", "m0", "w0"],
         ["mM", "H", "wA", "U", "mM2"],
         ["wA", "mM", "w0", "mM2", "m0"],
         ["H", "w0", "L", "w0"],
         ["wB", "H", "L", "mM2", "w0"],
         ["mM2", "wB", "m0", "H", "w0"],
         ["H", "mM", "wA", "L", "m0"],
         ["wA", "H", "m0", "mM", "L"],
         ["mM", "mM2", "wA", "wB", "m0"],
         ["H", "L", "H", "wA", "w0"],
         ["wB", "mM", "H", "w0", "m0"]]


class Model:
    """What the library holds: eff -- what the kernels read (None: all ones, no buffer); user -- the caller's factor kept
    beside a prior (None: ones); prior; huber.  Arrays are in the problem dtype."""

    def __init__(self, np_dtype):
        self.t, self.eff, self.user, self.prior, self.huber = np_dtype, None, None, None, False

    def product(self):
        self.eff = self.prior.copy() if self.user is None else self.prior * self.user  # one rounding, in the dtype

    def ones_under_huber(self):
        if self.huber and self.eff is None:
            self.eff = np.ones((K, C, H // S, W // S), dtype=self.t)

    def set_weights(self, w):
        w = None if w is None else np.asarray(w).astype(self.t)
        if self.prior is not None:
            self.user = w
            self.product()
        else:
            self.eff = w
            self.ones_under_huber()

    def set_prior(self, m):
        if m is None:
            if self.prior is not None:
                self.prior, self.eff, self.user = None, self.user, None
                self.ones_under_huber()
            return
        if self.prior is None:
            self.user = self.eff  # the weights in force become the caller's factor
        self.prior = np.asarray(m).astype(self.t)
        self.product()

    def set_loss(self, huber):
        self.huber = huber
        self.ones_under_huber()  # back to L2 the buffer and its contents stay


@pytest.fixture(scope="module")
def sr():
    import srmap
    return srmap


@pytest.fixture(scope="module")
def ctx(sr):
    c = sr.Context(0)
    p = sr.Problem(c, W, H, C, K, S, SHIFTS, 3, 1.0, sr.F32)  # the context's pinned staging exists from here on
    p.set_observations(np.zeros((K, C, H // S, W // S)))
    destroy(sr, p)
    return c


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(1800)
    model = orc.ImageModel(scale=S, shifts=SHIFTS, blur_ksize=3, blur_sigma=1.0)
    gt = rng.random((C, H, W))
    y = np.stack([model.apply(gt, k) for k in range(K)]) + 0.05 * rng.standard_normal((K, C, H // S, W // S))
    x = gt + 0.02 * rng.standard_normal(gt.shape)
    M2 = rng.random(y.shape)
    M2[1] = 0.0
    d = dict(model=model, y=y, x=x, A=2.0 * rng.random(y.shape), B=0.5 + rng.random(y.shape), M=rng.random(y.shape),
             M2=M2, regw=0.5 + rng.random(gt.shape))
    d["huber"] = rr.huber_weights(rr.residuals(model, y, x), DELTA)
    return d


@pytest.fixture(scope="module")
def device(data):
    import torch
    out = {}
    for dtype, tt in ((0, torch.float64), (1, torch.float32)):
        out[dtype] = {k: torch.tensor(data[k], dtype=tt, device="cuda") for k in ("B", "M2", "x")}
    torch.cuda.synchronize()
    return out


def destroy(sr, p):
    sr.load().srmap_problem_destroy(p._h)
    p._h = None


def make_problem(sr, ctx, dtype, data):
    p = sr.Problem(ctx, W, H, C, K, S, SHIFTS, 3, 1.0, dtype)
    p.set_observations(data["y"])
    p.add_regularizer(sr.REG_TV, 0.02)
    p.set_irls_weights(0, data["regw"])
    return p


def huber_step(sr, ctx, p, m, dtype, data, dev, tag):
    """U on p: the bits of a fresh problem with the same prior, the same loss and the same U; within the bar of the
    restatement's prior .* huber(r).  Returns those bits in the dtype."""
    p.update_data_weights_device(dev["x"].data_ptr())
    q = make_problem(sr, ctx, dtype, data)
    if m.prior is not None:
        q.set_data_prior(m.prior.astype(np.float64))
    q.set_data_loss(sr.DATA_LOSS_HUBER, DELTA)
    q.update_data_weights_device(dev["x"].data_ptr())
    got, fresh = p.data_weights(), q.data_weights()
    destroy(sr, q)
    assert np.array_equal(got, fresh), tag
    ref = data["huber"] if m.prior is None else m.prior.astype(np.float64) * data["huber"]
    err = float(np.max(np.abs(got - ref)))
    print("%s: |GPU - m .* huber(r)| %.2e (bar %.0e), down-weighted %.2f" % (tag, err, HUBER_BAR[dtype], np.mean(data["huber"] < 1)))
    assert err <= HUBER_BAR[dtype], tag
    return got.astype(m.t)


def run_sequence(sr, ctx, dtype, data, dev, seq):
    lib = sr.load()
    start = int(lib.srmap_live_allocations())
    p = make_problem(sr, ctx, dtype, data)
    m = Model(np.float32 if dtype else np.float64)
    for i, step in enumerate(seq):
        tag = "f%d %s step %d (%s)" % (32 if dtype else 64, " ".join(seq), i, step)
        if step == "wA":
            p.set_data_weights(data["A"])
            m.set_weights(data["A"])
        elif step == "wB":
            p.set_data_weights_device(dev["B"].data_ptr())
            m.set_weights(data["B"])
        elif step == "w0":
            p.set_data_weights(None)
            m.set_weights(None)
        elif step == "mM":
            p.set_data_prior(data["M"])
            m.set_prior(data["M"])
        elif step == "mM2":
            p.set_data_prior(dev["M2"])
            m.set_prior(data["M2"])
        elif step == "m0":
            p.set_data_prior(None)
            m.set_prior(None)
        elif step == "H":
            p.set_data_loss(sr.DATA_LOSS_HUBER, DELTA)
            m.set_loss(True)
        elif step == "L":
            p.set_data_loss(sr.DATA_LOSS_L2)
            m.set_loss(False)
        else:
            assert step == "U" and m.huber
            m.eff = huber_step(sr, ctx, p, m, dtype, data, dev, tag)
        want = np.ones(data["y"].shape) if m.eff is None else m.eff.astype(np.float64)
        assert np.array_equal(p.data_weights(), want), tag
        prior = p.data_prior()
        assert (prior is None) == (m.prior is None), tag
        assert prior is None or np.array_equal(prior, m.prior.astype(np.float64)), tag
    tag = "f%d %s" % (32 if dtype else 64, " ".join(seq))
    fresh = make_problem(sr, ctx, dtype, data)
    if m.eff is not None:
        fresh.set_data_weights(m.eff.astype(np.float64))
    fa, ga = p.eval(data["x"])
    fb, gb = fresh.eval(data["x"])
    assert fa == fb and np.array_equal(ga, gb), tag
    destroy(sr, p)
    destroy(sr, fresh)
    assert int(lib.srmap_live_allocations()) == start, tag


@pytest.mark.parametrize("dtype", [0, 1])
def test_every_ordered_pair_of_setters(sr, ctx, data, device, dtype):
    for seq in PAIRS:
        run_sequence(sr, ctx, dtype, data, device[dtype], seq)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("seq", FIXED, ids=["-".join(s) for s in FIXED])
def test_sequences_across_prior_huber_and_clears(sr, ctx, data, device, dtype, seq):
    run_sequence(sr, ctx, dtype, data, device[dtype], seq)
