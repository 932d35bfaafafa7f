"""The scenarios of tests/test_gpu_ownership.py, in ONE fresh process:

    python ownership_worker.py <results.jsonl>

srmap_live_allocations() counts the device and pinned-host blocks the library holds (csrc/dev_mem.hpp).  Every scenario
reads it around the calls it is about and appends one JSON record {"name", "checks": [[label, got, want], ...],
"info": {...}} to the results file; the test asserts got == want for every check.  Nothing here fails on the device:
every refusal is an argument check the library makes anyway.  An unexpected error is written as {"name", "error"} and
ends the process non-zero at once: no further scenario runs after it.

Shapes: HR 64 x 64, scale 2, 3 frames, 2 channels (LR 32 x 32: the flow registration still builds two pyramid levels,
the tile planner still covers the problem), both dtypes; 32 x 32 images for the stand-alone registrations.
"""
import json
import os
import sys
import traceback

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "super-resolution_amd", "python"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

W = H = 64
S, K, C = 2, 3, 2
INT_SHIFTS = [[0, 0], [1, 1], [0, 1]]
SUB_SHIFTS = [[0, 0], [0.5, 0.25], [-0.75, 0.375]]
# dy within floating-point rounding of a 1/32-px tie: warpAffine's y table is not uniform, the problem keeps a per-row table
TIE_SHIFTS = [[0.25, -0.0151367187499999], [-1.5, 0.0161132812500001], [0.0, 0.0]]
DTYPES = (("f64", 0), ("f32", 1))


def smooth_image(h, w, dx=0.0, dy=0.0):
    """An aperiodic smooth texture sampled at (x + dx, y + dy): what the registrations can lock on to."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x + dx, y + dy
    return (np.sin(0.21 * x + 0.08 * y) + np.cos(0.13 * x - 0.19 * y) + 0.02 * x - 0.015 * y
            + 1.5 * np.exp(-((x - 0.4 * w) ** 2 + (y - 0.6 * h) ** 2) / (0.08 * w * h)))


class Run:
    def __init__(self, out_path):
        torch.cuda.init()
        torch.zeros(1, device="cuda")  # torch's HIP runtime first (see tests/conftest.py)
        import srmap
        self.sr = srmap
        self.lib = srmap.load()
        self.out = open(out_path, "w")
        self.rng = np.random.default_rng(1700)
        self.x_true = np.stack([smooth_image(H, W), smooth_image(H, W, 3.0, -2.0)])
        self.x0 = self.x_true + 0.05 * self.rng.standard_normal(self.x_true.shape)

    def live(self):
        return int(self.lib.srmap_live_allocations())

    def record(self, name, checks, **info):
        self.out.write(json.dumps({"name": name, "checks": checks, "info": info}) + "\n")
        self.out.flush()

    def destroy(self, p):
        self.lib.srmap_problem_destroy(p._h)
        p._h = None

    def refused(self, call, *statuses):
        """call() must be refused with one of `statuses`; returns the status."""
        try:
            call()
        except self.sr.SrmapError as e:
            assert e.status in statuses, e
            return e.status
        raise AssertionError("the call was not refused")

    def problem(self, dtype, shifts=INT_SHIFTS, impl=None, observations=True):
        p = self.sr.Problem(self.ctx, W, H, C, K, S, shifts, 3, 1.0, dtype)
        if impl is not None:
            p.set_impl(impl)
        if observations:
            p.set_observations(np.stack([p.apply(self.x_true, k) for k in range(K)]))
        return p

    # ------------------------------------------------------------------------------------------------ scenarios
    def create_eval_destroy(self, tag, dtype):
        sr = self.sr
        for name, shifts, impl, want_impl in (("integer", INT_SHIFTS, None, sr.IMPL_TILED),
                                              ("subpixel", SUB_SHIFTS, None, sr.IMPL_TILED),
                                              ("rounding_tie", TIE_SHIFTS, None, sr.IMPL_DIRECT),  # the per-row y table
                                              ("direct", INT_SHIFTS, sr.IMPL_DIRECT, sr.IMPL_DIRECT)):
            before = self.live()
            p = self.problem(dtype, shifts, impl)
            p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.5)
            p.set_irls_weights(0, 0.5 + self.rng.random((C, H, W)))
            active = p.active_impl()
            f, g = p.eval(self.x0)
            held = self.live()
            self.destroy(p)
            self.record("create_eval_destroy[%s,%s]" % (name, tag),
                        [["active implementation", active, want_impl], ["finite cost", bool(np.isfinite(f)), True],
                         ["holds buffers while alive", held > before, True], ["after destroy", self.live(), before]],
                        held=held - before)

    def setters(self, tag, dtype):
        sr = self.sr
        p = self.problem(dtype)
        p.eval(self.x0)  # the problem's lazy buffers exist from here on

        def run(name, steps):
            """steps: (label, call, expected change of the count from the scenario's start, refused statuses or None).
            The change is None where the step re-plans: the tile plan's tables come and go with the model (an affine
            motion, a flow or a free-form blur has none; weights give it another form), so only the refused and the
            clearing steps have a count that follows from the call alone; the others are kept as information."""
            c0, checks, seen = self.live(), [], {}
            for label, call, delta, statuses in steps:
                if statuses:
                    before = self.live()
                    self.refused(call, *statuses)
                    checks.append([label + " (refused): unchanged", self.live(), before])
                else:
                    call()
                    seen[label] = self.live() - c0
                    if delta is not None:
                        checks.append([label, seen[label], delta])
            f, _ = p.eval(self.x0)  # the problem still evaluates
            checks.append(["finite cost afterwards", bool(np.isfinite(f)), True])
            self.record("setter[%s,%s]" % (name, tag), checks, changes=seen)

        ident = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (K, 1, 1))
        good_affine = ident.copy()
        good_affine[1] = [[1.01, 0.02, 0.5], [-0.02, 0.99, -0.25]]
        bad_affine = ident.copy()
        bad_affine[2, 0, 0] = 1.3  # deviation 0.3 > 0.25
        run("affine", [("set", lambda: p.set_affine_motion(good_affine), None, None),
                       ("deviation above 0.25", lambda: p.set_affine_motion(bad_affine), 0, (sr.EUNSUPPORTED,)),
                       ("cleared", lambda: p.set_affine_motion(None), 0, None)])

        field = sr.flow_from_shifts(INT_SHIFTS, H, W)
        nan_field = field.copy()
        nan_field[1, 0, 3, 4] = np.nan
        folded = field.copy()
        qx = np.arange(W, dtype=np.float64)[None, :]  # the middle third of every row samples ONE source column: a fold
        folded[1, 0] = np.where((qx >= W // 3) & (qx < 2 * W // 3), (W // 3 + 0.5) - qx, 0.0) * np.ones((H, 1))
        folded[1, 1] = 0.0
        run("flow", [("set", lambda: p.set_flow(field), None, None),
                     ("non-finite field", lambda: p.set_flow(nan_field), 0, (sr.EINVAL,)),
                     ("folding field", lambda: p.set_flow(folded), 0, (sr.EUNSUPPORTED,)),
                     ("cleared", lambda: p.set_flow(None), 0, None)])

        taps = np.outer([0.2, 0.6, 0.2], [0.25, 0.5, 0.25])
        run("blur", [("set", lambda: p.set_blur_kernel(taps), None, None),
                     ("even size", lambda: p.set_blur_kernel(np.full((4, 4), 1.0 / 16)), 0, (sr.EINVAL,)),
                     ("cleared", lambda: p.set_blur_kernel(None), 0, None)])

        gains = np.array([[1.0, 0.0], [1.1, 0.02], [0.9, -0.01]])
        bad_gains = gains.copy()
        bad_gains[1, 0] = 0.0
        run("photometric", [("set", lambda: p.set_photometric(gains), 2, None),  # the parameters and the normalised copy
                            ("gain of 0", lambda: p.set_photometric(bad_gains), 0, (sr.EINVAL,)),
                            ("set again", lambda: p.set_photometric(gains[::-1].copy()), 2, None),
                            ("cleared", lambda: p.set_photometric(None), 0, None)])

        n_lr = (K, C, p.h, p.w)
        prior, weights = 0.5 + 0.5 * self.rng.random(n_lr), self.rng.random(n_lr)
        run("prior_then_weights", [("prior", lambda: p.set_data_prior(prior), None, None),
                                   ("weights", lambda: p.set_data_weights(weights), None, None),
                                   ("negative weight", lambda: p.set_data_weights(-weights), 0, (sr.EINVAL,)),
                                   ("prior removed", lambda: p.set_data_prior(None), None, None),
                                   ("weights removed", lambda: p.set_data_weights(None), 0, None)])
        # a Huber loss owns the weight buffer and leaves it (the last outlier map) when the loss goes back to L2:
        # removing the weights is what clears it
        run("huber_then_prior", [("Huber on", lambda: p.set_data_loss(sr.DATA_LOSS_HUBER, 0.1), None, None),
                                 ("prior", lambda: p.set_data_prior(prior), None, None),
                                 ("Huber off", lambda: p.set_data_loss(sr.DATA_LOSS_L2), None, None),
                                 ("prior removed", lambda: p.set_data_prior(None), None, None),
                                 ("weights removed", lambda: p.set_data_weights(None), 0, None)])
        self.destroy(p)

    def replacement(self, tag, dtype):
        """The motions are alternatives, and so are the blurs: a problem taken from one to another holds exactly the
        blocks of a fresh problem given only the second (the first one's are all freed), and NULL to any setter of the
        family gives the count before the first setter.  (No step here keeps a tile plan but the last: neither a replaced
        motion nor a replaced blur has one.)"""
        def held(steps):
            """A fresh problem: the change of the count after each of `steps`, from the count before the first."""
            p = self.problem(dtype)
            p.eval(self.x0)
            c0, out = self.live(), []
            for step in steps:
                step(p)
                out.append(self.live() - c0)
            self.destroy(p)
            return out

        def family(name, setters, sequences):
            """sequences: (first, second, the setter that takes the closing NULL)."""
            fresh = {k: held([call])[0] for k, call in setters.items()}
            checks = []
            for a, b, closing in sequences:
                _, after_b, after_null = held([setters[a], setters[b], null[closing]])
                checks.append(["%s -> %s: as a fresh problem with the second alone" % (a, b), after_b, fresh[b]])
                checks.append(["%s -> %s -> %s(None)" % (a, b, closing), after_null, 0])
            self.record("replacement[%s,%s]" % (name, tag), checks, fresh=fresh)

        null = {"set_affine_motion": lambda p: p.set_affine_motion(None), "set_flow": lambda p: p.set_flow(None),
                "set_flow_lattice": lambda p: p.set_flow_lattice(None, 0), "set_blur_kernel": lambda p: p.set_blur_kernel(None),
                "set_blur_bank": lambda p: p.set_blur_bank(None)}
        affine = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (K, 1, 1))
        affine[1] = [[1.01, 0.02, 0.5], [-0.02, 0.99, -0.25]]
        field = self.sr.flow_from_shifts(INT_SHIFTS, H, W)
        nodes = np.full((K, 2, 5, 5), 0.25)  # step 16: the last node one cell beyond the 64 x 64 image
        family("motion", {"affine": lambda p: p.set_affine_motion(affine), "flow": lambda p: p.set_flow(field),
                          "lattice": lambda p: p.set_flow_lattice(nodes, 16)},
               [("affine", "flow", "set_affine_motion"), ("affine", "lattice", "set_flow"), ("flow", "affine", "set_flow_lattice"),
                ("lattice", "flow", "set_affine_motion"), ("flow", "lattice", "set_flow")])
        taps = np.outer([0.2, 0.6, 0.2], [0.25, 0.5, 0.25])
        bank = np.stack([taps, taps.T, taps[::-1].copy()])  # a kernel per frame
        family("blur", {"free-form": lambda p: p.set_blur_kernel(taps), "bank": lambda p: p.set_blur_bank(bank, self.sr.BLUR_PER_FRAME)},
               [("free-form", "bank", "set_blur_kernel"), ("bank", "free-form", "set_blur_bank")])

    def churn(self, tag, dtype):
        sr = self.sr
        p = self.problem(dtype)
        p.eval(self.x0)
        counts = []
        for _ in range(3):
            p.add_regularizer(sr.REG_TV, 0.01)
            p.set_irls_weights(0, np.ones((C, H, W)))
            p.eval(self.x0)
            p.clear_regularizers()
            p.eval(self.x0)
            counts.append(self.live())
        self.record("churn[regularizers,%s]" % tag, [["repetition %d" % i, c, counts[0]] for i, c in enumerate(counts)])
        counts = []
        for _ in range(3):
            p.set_data_loss(sr.DATA_LOSS_HUBER, 0.1)
            p.eval(self.x0)
            p.set_data_loss(sr.DATA_LOSS_L2)
            p.eval(self.x0)
            counts.append(self.live())
        self.record("churn[data_loss,%s]" % tag, [["repetition %d" % i, c, counts[0]] for i, c in enumerate(counts)])
        self.destroy(p)

    def twice(self, name, call):
        """A call with scratch of its own: once to create the lazy buffers the problem or the context keeps (IRLS
        weights, the staging of host images, the residuals), then the count around a second call."""
        call()
        before = self.live()
        call()
        self.record(name, [["after == before", self.live(), before]])

    def scratch(self, tag, dtype):
        sr = self.sr
        p = self.problem(dtype, SUB_SHIFTS)
        p.add_regularizer(sr.REG_BTV, 0.01, 2, 0.5)
        o = sr.default_irls_options()
        o.max_num_solver_iterations, o.max_num_irls_iterations = 3, 2
        self.twice("scratch[solve_cg,%s]" % tag, lambda: p.solve(self.x0, o))
        p.set_solver(sr.SOLVER_LBFGS, 3)
        self.twice("scratch[solve_lbfgs,%s]" % tag, lambda: p.solve(self.x0, o))
        p.set_solver(sr.SOLVER_CG)
        o.split_channels = 1
        self.twice("scratch[solve_split_channels,%s]" % tag, lambda: p.solve(self.x0, o))
        self.twice("scratch[cg_trace,%s]" % tag, lambda: p.cg_trace(self.x0, maxits=3))
        self.twice("scratch[lbfgs_trace,%s]" % tag, lambda: p.lbfgs_trace(self.x0, m=3, maxits=3))
        self.twice("scratch[fit_blur,%s]" % tag, lambda: p.fit_blur(self.x_true, ksize=3, apply=False))
        self.twice("scratch[fit_photometric,%s]" % tag, lambda: p.fit_photometric(self.x_true, apply=False))
        self.twice("scratch[refine_motion,%s]" % tag, lambda: p.refine_motion(self.x_true, max_iterations=3, apply=False))
        p.set_flow(sr.flow_from_shifts(SUB_SHIFTS, H, W))
        self.twice("scratch[fit_blur_refused_under_flow,%s]" % tag,
                   lambda: self.refused(lambda: p.fit_blur(self.x_true, ksize=3, apply=False), sr.EUNSUPPORTED))
        self.twice("scratch[fit_photometric_refused_under_flow,%s]" % tag,
                   lambda: self.refused(lambda: p.fit_photometric(self.x_true, apply=False), sr.EUNSUPPORTED))
        p.set_flow(None)
        # the problem form installs the field and the prior: the second call replaces both
        self.twice("scratch[register_flow_problem,%s]" % tag, lambda: p.register_flow(channel=-1, prior=True, warps=2))
        self.destroy(p)

    def registrations(self):
        sr, ctx = self.sr, self.ctx
        moves = [(0.0, 0.0), (1.25, -0.5), (-0.75, 1.0)]
        images = np.stack([smooth_image(32, 32, dx, dy) for dx, dy in moves])
        self.twice("scratch[register_translational]", lambda: ctx.register_translational(images, with_quality=True))
        self.twice("scratch[register_affine]", lambda: ctx.register_affine(images, max_iterations=5, with_quality=True))
        self.twice("scratch[register_flow_host]", lambda: ctx.register_flow(images, warps=2))
        self.twice("scratch[register_flow_host_single_image]", lambda: ctx.register_flow(images[:1], warps=2))
        dev = torch.from_numpy(images).cuda()
        flow_out = torch.empty((3, 2, 32, 32), dtype=torch.float64, device="cuda")
        valid_out = torch.empty((3, 32, 32), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        self.twice("scratch[register_flow_device]", lambda: ctx.register_flow(dev, warps=2, flow_out=flow_out, valid_out=valid_out))
        self.twice("scratch[register_flow_device_single_image]",
                   lambda: ctx.register_flow(dev[:1].contiguous(), warps=2, flow_out=flow_out[:1].contiguous()))
        bad = dev.clone()
        bad[2, 5, 7] = float("nan")
        torch.cuda.synchronize()
        self.twice("scratch[register_flow_device_non_finite_pixel]",  # refused after the work ran
                   lambda: self.refused(lambda: ctx.register_flow(bad, warps=2, flow_out=flow_out), sr.EINVAL))
        cube = self.rng.random((3, 16, 16))
        M = self.rng.random((2, 3))
        self.twice("scratch[channel_map]", lambda: ctx.channel_map(M, cube, offset_in=np.ones(3), offset_out=np.zeros(2)))
        self.twice("scratch[pca]", lambda: ctx.pca(self.rng.random((3, 64))))

    def main(self):
        start = self.live()
        self.ctx = self.sr.Context(0)
        self.destroy(self.problem(0))  # the context's pinned staging exists from here on (it goes with the context)
        for tag, dtype in DTYPES:
            self.create_eval_destroy(tag, dtype)
            self.setters(tag, dtype)
            self.replacement(tag, dtype)
            self.churn(tag, dtype)
            self.scratch(tag, dtype)
        self.registrations()
        held = self.live()
        self.lib.srmap_ctx_destroy(self.ctx._h)
        self.ctx._h = None
        self.record("end", [["count at the start", start, 0], ["every problem and context destroyed", self.live(), 0]],
                    context_held=held)


if __name__ == "__main__":
    run = Run(sys.argv[1])
    try:
        run.main()
    except Exception:  # noqa: BLE001 -- written down, and nothing further runs
        run.out.write(json.dumps({"name": "worker", "error": traceback.format_exc()}) + "\n")
        run.out.close()
        traceback.print_exc()
        sys.exit(1)
    run.out.close()
