"""ctypes binding of libsrmap.so (include/srmap.h) for the test-suite and
bench.py.  This is harness plumbing: the product is the C-ABI library and the
C++ facade in super-resolution_amd/host.  There is no CPU fallback -- importing
works anywhere (so that symbol checks can run without a GPU), but creating a
context without a HIP device raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRMAP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libsrmap.so")

OK, EINVAL, ENOMEM, EHIP, EUNSUPPORTED = 0, 1, 2, 3, 4
F64, F32 = 0, 1
REG_TV, REG_TV3D, REG_BTV = 0, 1, 2
REG_GRADIENT_REFERENCE, REG_GRADIENT_EXACT = 0, 1  # srmap_reg_gradient
TERM_DATA, TERM_REG, TERM_ALL = 1, 2, 3
IMPL_AUTO, IMPL_DIRECT, IMPL_TILED = 0, 1, 2
SOLVER_CG, SOLVER_LBFGS = 0, 1  # srmap_solver (MapSolverOptions::least_squares_solver)
DATA_LOSS_L2, DATA_LOSS_HUBER = 0, 1  # srmap_data_loss
HUBER_DELTA_FIXED, HUBER_DELTA_MAD = 0, 1  # srmap_huber_delta_mode

c_double_p = C.POINTER(C.c_double)


class SrmapError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("srmap status %d: %s" % (status, message))
        self.status = status


class ProblemDesc(C.Structure):
    _fields_ = [("hr_width", C.c_int), ("hr_height", C.c_int), ("channels", C.c_int),
                ("frames", C.c_int), ("scale", C.c_int), ("shifts_xy", c_double_p),
                ("blur_ksize", C.c_int), ("blur_sigma", C.c_double), ("dtype", C.c_int)]


class IrlsOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int),
                ("max_num_solver_iterations", C.c_int),
                ("gradient_norm_threshold", C.c_double),
                ("cost_decrease_threshold", C.c_double),
                ("parameter_variation_threshold", C.c_double),
                ("split_channels", C.c_int),
                ("max_num_irls_iterations", C.c_int),
                ("irls_cost_difference_threshold", C.c_double),
                ("host_paced_passes", C.c_int)]


class AffineRegistrationOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("hr_scale", C.c_int), ("max_iterations", C.c_int),
                ("step_tolerance", C.c_double), ("max_levels", C.c_int), ("initial_affine_2x3", c_double_p)]


class FlowRegistrationOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("hr_scale", C.c_int), ("warps", C.c_int), ("window_radius", C.c_int),
                ("damping", C.c_double), ("smooth_radius", C.c_int), ("valid_margin", C.c_int), ("max_levels", C.c_int),
                ("initial_affine_2x3", c_double_p)]


class MotionRefinementOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("dof", C.c_int), ("max_iterations", C.c_int), ("step_tolerance", C.c_double),
                ("initial_damping", C.c_double), ("apply", C.c_int), ("initial_affine_2x3", c_double_p)]


class BlurFitOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("ksize", C.c_int), ("sum_to_one", C.c_int), ("ridge", C.c_double), ("apply", C.c_int)]


class PhotometricFitOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("model", C.c_int), ("gauge_frame", C.c_int), ("min_gain", C.c_double),
                ("max_gain", C.c_double), ("apply", C.c_int)]


LAMBDA_PATH_MAX_SCALES, LAMBDA_PATH_ROW = 32, 11  # SRMAP_LAMBDA_PATH_MAX_SCALES, SRMAP_LAMBDA_PATH_ROW


class LambdaPathOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("num_scales", C.c_int), ("scales", C.c_double * LAMBDA_PATH_MAX_SCALES),
                ("patience", C.c_int), ("final_solve", C.c_int)]


LAMBDA_RULE_MIN, LAMBDA_RULE_ONE_SE = 0, 1  # SRMAP_LAMBDA_RULE_*
LAMBDA_RULES = {"min": LAMBDA_RULE_MIN, "one_se": LAMBDA_RULE_ONE_SE}


class LambdaCvOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int), ("num_scales", C.c_int), ("scales", C.c_double * LAMBDA_PATH_MAX_SCALES),
                ("folds", C.c_int), ("rule", C.c_int), ("seed", C.c_ulonglong), ("se_factor", C.c_double),
                ("patience", C.c_int), ("final_solve", C.c_int)]


class SolveReport(C.Structure):
    _fields_ = [("irls_rounds", C.c_int), ("cg_iterations", C.c_int), ("evaluations", C.c_int),
                ("last_termination", C.c_int), ("final_cost", C.c_double), ("loop_seconds", C.c_double),
                ("wait_seconds", C.c_double), ("waits", C.c_int)]


class ShardDesc(C.Structure):
    _fields_ = [("mode", C.c_int), ("own_row0", C.c_int), ("own_row1", C.c_int),
                ("send_up_rows", C.c_int), ("send_down_rows", C.c_int),
                ("own_ch0", C.c_int), ("own_ch1", C.c_int), ("reg_rank", C.c_int),
                ("frame_groups", C.c_int), ("frame_comm", C.c_void_p)]


SHARD_NONE, SHARD_FRAMES, SHARD_ROWS, SHARD_CHANNELS, SHARD_GRID = 0, 1, 2, 3, 4
BLUR_PER_FRAME, BLUR_PER_CHANNEL, BLUR_PER_FRAME_CHANNEL = 1, 2, 3  # srmap_blur_bank_mode
HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p)
HOST_SENDRECV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)

# every symbol include/srmap.h declares: (name, restype, argtypes)
_SIGNATURES = [
    ("srmap_ctx_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("srmap_ctx_destroy", None, [C.c_void_p]),
    ("srmap_last_error", C.c_char_p, [C.c_void_p]),
    ("srmap_version", C.c_char_p, []),
    ("srmap_live_allocations", C.c_longlong, []),
    ("srmap_problem_create", C.c_int, [C.c_void_p, C.POINTER(ProblemDesc), C.POINTER(C.c_void_p)]),
    ("srmap_problem_set_cost_rows", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("srmap_problem_destroy", None, [C.c_void_p]),
    ("srmap_problem_set_impl", C.c_int, [C.c_void_p, C.c_int]),
    ("srmap_problem_set_solver", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("srmap_problem_set_affine_motion", C.c_int, [C.c_void_p, c_double_p]),
    ("srmap_problem_set_flow", C.c_int, [C.c_void_p, c_double_p]),
    ("srmap_problem_set_flow_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("srmap_problem_get_flow", C.c_int, [C.c_void_p, c_double_p, C.POINTER(C.c_int)]),
    ("srmap_problem_set_flow_lattice", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_double_p]),
    ("srmap_problem_set_flow_lattice_device", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("srmap_problem_get_flow_lattice", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p]),
    ("srmap_problem_set_blur_kernel", C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    ("srmap_problem_get_blur_kernel", C.c_int, [C.c_void_p, C.POINTER(C.c_int), c_double_p]),
    ("srmap_blur_fit_options_default", None, [C.c_void_p]),
    ("srmap_fit_blur", C.c_int, [C.c_void_p, c_double_p, C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("srmap_fit_blur_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("srmap_problem_set_blur_bank", C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p]),
    ("srmap_problem_get_blur_bank", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p]),
    ("srmap_fit_blur_bank", C.c_int, [C.c_void_p, c_double_p, C.c_int, C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("srmap_fit_blur_bank_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("srmap_problem_set_photometric", C.c_int, [C.c_void_p, c_double_p]),
    ("srmap_problem_get_photometric", C.c_int, [C.c_void_p, c_double_p, C.POINTER(C.c_int)]),
    ("srmap_photometric_fit_options_default", None, [C.c_void_p]),
    ("srmap_fit_photometric", C.c_int, [C.c_void_p, c_double_p, C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("srmap_fit_photometric_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("srmap_problem_lr_size", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("srmap_set_observations", C.c_int, [C.c_void_p, c_double_p]),
    ("srmap_problem_active_impl", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("srmap_set_observations_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("srmap_add_regularizer", C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double, C.POINTER(C.c_int)]),
    ("srmap_clear_regularizers", C.c_int, [C.c_void_p]),
    ("srmap_set_irls_weights", C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    ("srmap_update_irls_weights_device", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    ("srmap_set_data_weights", C.c_int, [C.c_void_p, c_double_p]),
    ("srmap_set_data_weights_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("srmap_get_data_weights", C.c_int, [C.c_void_p, c_double_p]),
    ("srmap_problem_set_data_loss", C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    ("srmap_update_data_weights_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("srmap_set_data_prior", C.c_int, [C.c_void_p, c_double_p]),
    ("srmap_set_data_prior_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("srmap_get_data_prior", C.c_int, [C.c_void_p, c_double_p, C.POINTER(C.c_int)]),
    ("srmap_problem_set_huber_scale", C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double]),
    ("srmap_problem_get_huber_delta", C.c_int, [C.c_void_p, C.POINTER(C.c_int), c_double_p, c_double_p, c_double_p]),
    ("srmap_residual_scale", C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("srmap_residual_scale_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_double_p, c_double_p]),
    ("srmap_problem_set_holdout", C.c_int, [C.c_void_p, C.c_double, C.c_ulonglong]),
    ("srmap_problem_get_holdout", C.c_int, [C.c_void_p, c_double_p, C.POINTER(C.c_ulonglong), c_double_p, c_double_p]),
    ("srmap_problem_set_holdout_fold", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_ulonglong]),
    ("srmap_problem_get_holdout_fold", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]),
    ("srmap_holdout_score", C.c_int, [C.c_void_p, c_double_p, C.c_double, c_double_p, c_double_p]),
    ("srmap_holdout_score_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, c_double_p, c_double_p]),
    ("srmap_problem_set_regularizer_lambda", C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    ("srmap_problem_get_regularizer_lambda", C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    ("srmap_problem_set_regularizer_gradient", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("srmap_problem_get_regularizer_gradient", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    ("srmap_lambda_path_options_default", None, [C.c_void_p]),
    ("srmap_solve_lambda_path", C.c_int, [C.c_void_p, C.POINTER(IrlsOptions), C.c_void_p, c_double_p, c_double_p, c_double_p,
                                          C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(SolveReport)]),
    ("srmap_lambda_cv_options_default", None, [C.c_void_p]),
    ("srmap_solve_lambda_path_folds", C.c_int, [C.c_void_p, C.POINTER(IrlsOptions), C.c_void_p, c_double_p, c_double_p, c_double_p,
                                                c_double_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(SolveReport)]),
    ("srmap_apply", C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p]),
    ("srmap_apply_transpose", C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p]),
    ("srmap_reg_values", C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p]),
    ("srmap_reg_values_and_gradient", C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]),
    ("srmap_eval", C.c_int, [C.c_void_p, C.c_uint, c_double_p, c_double_p, c_double_p]),
    ("srmap_eval_device", C.c_int, [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, c_double_p, C.c_void_p]),
    ("srmap_last_cost", C.c_int, [C.c_void_p, c_double_p]),
    ("srmap_device_alloc", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    ("srmap_device_free", C.c_int, [C.c_void_p, C.c_void_p]),
    ("srmap_upload", C.c_int, [C.c_void_p, c_double_p, C.c_void_p, C.c_size_t]),
    ("srmap_download", C.c_int, [C.c_void_p, C.c_void_p, c_double_p, C.c_size_t]),
    ("srmap_channel_map", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    ("srmap_channel_map_device", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, c_double_p, c_double_p, c_double_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("srmap_register_translational", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_double_p, c_double_p]),
    ("srmap_register_translational_ex", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p]),
    ("srmap_affine_registration_options_default", None, [C.c_void_p]),
    ("srmap_register_affine", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_double_p, C.c_void_p, c_double_p, c_double_p]),
    ("srmap_flow_registration_options_default", None, [C.c_void_p]),
    ("srmap_register_flow", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_double_p, C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("srmap_register_flow_device", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_double_p]),
    ("srmap_problem_register_flow", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, c_double_p]),
    ("srmap_problem_register_flow_lattice", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, c_double_p]),
    ("srmap_motion_refinement_options_default", None, [C.c_void_p]),
    ("srmap_refine_motion", C.c_int, [C.c_void_p, c_double_p, C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("srmap_refine_motion_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, c_double_p, c_double_p, c_double_p]),
    ("srmap_channel_pca", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, c_double_p, c_double_p, c_double_p, c_double_p]),
    ("srmap_channel_pca_device", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, c_double_p, c_double_p, c_double_p, C.c_void_p]),
    ("srmap_synchronize", C.c_int, [C.c_void_p]),
    ("srmap_irls_options_default", None, [C.POINTER(IrlsOptions)]),
    ("srmap_solve", C.c_int, [C.c_void_p, C.POINTER(IrlsOptions), c_double_p, c_double_p, C.POINTER(SolveReport)]),
    ("srmap_problem_selfcheck", C.c_int, [C.c_void_p, c_double_p]),
    ("srmap_comm_get_unique_id", C.c_int, [C.c_void_p, C.c_char_p]),
    ("srmap_comm_create_rccl", C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("srmap_comm_create_host", C.c_int, [C.c_void_p, C.c_int, C.c_int, HOST_ALLREDUCE_FN, HOST_SENDRECV_FN, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("srmap_comm_destroy", None, [C.c_void_p]),
    ("srmap_comm_info", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("srmap_comm_set_overlap", C.c_int, [C.c_void_p, C.c_int]),
    ("srmap_comm_describe", C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    ("srmap_comm_split", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("srmap_comm_allreduce", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]),
    ("srmap_eval_sharded_device", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ShardDesc), C.c_uint, C.c_void_p, C.c_void_p, c_double_p, C.c_void_p]),
    ("srmap_solve_sharded", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ShardDesc), C.POINTER(IrlsOptions), c_double_p, c_double_p, C.POINTER(SolveReport)]),
    ("srmap_cg_trace", C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, c_double_p, c_double_p,
                                 C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p, C.c_int, C.POINTER(C.c_int)]),
    ("srmap_lbfgs_trace", C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, c_double_p, c_double_p,
                                    C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p, C.c_int, C.POINTER(C.c_int)]),
]
EXPORTED_SYMBOLS = [s[0] for s in _SIGNATURES]

_lib = None


def load():
    """dlopen libsrmap.so; raises if the HIP library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libsrmap.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'`; "
                               "there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in _SIGNATURES:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(c_double_p)


def _flow_options(n, hr_scale, init, warps, window_radius, damping, smooth_radius, valid_margin, max_levels, struct_size):
    """srmap_flow_registration_options from keyword values; the second result keeps the matrices alive."""
    o = FlowRegistrationOptions()
    load().srmap_flow_registration_options_default(C.byref(o))
    o.hr_scale, o.warps, o.window_radius, o.damping = hr_scale, warps, window_radius, damping
    o.smooth_radius, o.valid_margin, o.max_levels = smooth_radius, valid_margin, max_levels
    if struct_size is not None:
        o.struct_size = struct_size
    ini = None
    if init is not None:
        ini, pi = _d(init)
        assert ini.size == n * 6, (ini.shape, n)
        o.initial_affine_2x3 = pi
    return o, ini


class Context:
    def __init__(self, device=0):
        self._h = C.c_void_p()
        st = load().srmap_ctx_create(device, C.byref(self._h))
        if st != OK:
            raise SrmapError(st, "srmap_ctx_create failed (no usable HIP device %d; no CPU path exists)" % device)

    def check(self, st):
        if st != OK:
            raise SrmapError(st, load().srmap_last_error(self._h).decode())

    def synchronize(self):
        self.check(load().srmap_synchronize(self._h))

    def channel_map(self, M, x, offset_in=None, offset_out=None):
        """out[r] = sum_c M[r, c] * (x[c] - offset_in[c]) + offset_out[r] on a planar image x[C, ...] (GPU DGEMM)."""
        Mm, pM = _d(M)
        a, pa = _d(x)
        ro, ri = Mm.shape
        assert a.shape[0] == ri
        n = a.size // ri
        out = np.empty((ro,) + a.shape[1:])
        oi = _d(offset_in) if offset_in is not None else (None, None)
        oo = _d(offset_out) if offset_out is not None else (None, None)
        self.check(load().srmap_channel_map(self._h, ro, ri, n, pM, oi[1], oo[1], pa, out.ctypes.data_as(c_double_p)))
        return out

    def channel_map_device(self, M, in_ptr, out_ptr, n, offset_in=None, offset_out=None, stream=None):
        """The same on device-resident planar f64 cubes (raw device pointers, n pixels per channel)."""
        Mm, pM = _d(M)
        ro, ri = Mm.shape
        oi = _d(offset_in) if offset_in is not None else (None, None)
        oo = _d(offset_out) if offset_out is not None else (None, None)
        self.check(load().srmap_channel_map_device(self._h, ro, ri, n, pM, oi[1], oo[1], C.c_void_p(in_ptr),
                                                   C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None))

    def register_translational(self, images, with_quality=False):
        """registration::TranslationalRegistration: images [n][H][W] -> shifts [n][2] (dx, dy) relative to image 0
        (with_quality: also [n][2] = separation of the coarse minimum, RMS residual -- srmap.h)."""
        a, pa = _d(images)
        n, H, W = a.shape
        out = np.zeros((n, 2))
        if not with_quality:
            self.check(load().srmap_register_translational(self._h, n, W, H, pa, out.ctypes.data_as(c_double_p)))
            return out
        q = np.zeros((n, 2))
        self.check(load().srmap_register_translational_ex(self._h, n, W, H, pa, out.ctypes.data_as(c_double_p),
                                                          q.ctypes.data_as(c_double_p)))
        return out, q

    def register_affine(self, images, hr_scale=1, init=None, max_iterations=30, step_tolerance=1e-4, max_levels=0,
                        with_quality=False, struct_size=None):
        """srmap_register_affine: images [n][H][W] -> [n][2][3] = [a b tx; c d ty] of F_k, I_k(F_k(p)) ~= I_0(p), t in
        units of hr_scale input pixels (ready for Problem.set_affine_motion); init: [n][2][3] starting matrices in input
        pixels instead of the coarse search (with_quality: also [n][4] = separation, RMS residual, used pixel fraction,
        Gauss-Newton passes -- srmap.h).  struct_size overrides the options' size field (tests)."""
        a, pa = _d(images)
        n, H, W = a.shape
        o = AffineRegistrationOptions()
        load().srmap_affine_registration_options_default(C.byref(o))
        o.hr_scale, o.max_iterations, o.step_tolerance, o.max_levels = hr_scale, max_iterations, step_tolerance, max_levels
        if struct_size is not None:
            o.struct_size = struct_size
        if init is not None:
            ini, pi = _d(init)
            assert ini.size == n * 6, (ini.shape, n)
            o.initial_affine_2x3 = pi
        out, q = np.zeros((n, 2, 3)), np.zeros((n, 4))
        self.check(load().srmap_register_affine(self._h, n, W, H, pa, C.byref(o), out.ctypes.data_as(c_double_p),
                                                q.ctypes.data_as(c_double_p) if with_quality else None))
        return (out, q) if with_quality else out

    def register_flow(self, images, hr_scale=1, init=None, warps=8, window_radius=4, damping=0.05, smooth_radius=2,
                      valid_margin=3, max_levels=0, struct_size=None, flow_out=None, valid_out=None, stream=None):
        """srmap_register_flow: images [n][H][W] -> (flow [n][2][s H][s W], valid [n][H][W], quality [n][3]) with
        s = hr_scale: the fields u_k, I_0(q + u_k(q)) ~= I_k(q), in units of HR pixels (ready for Problem.set_flow), the
        validity mask at input resolution (ready for Problem.set_data_prior / set_data_weights, one plane per channel)
        and (RMS residual, valid fraction, max dx + dy of the field) per image -- srmap.h.  init: [n][2][3] starting
        matrices in input pixels (register_affine's) instead of u = 0.  struct_size overrides the options' size field
        (tests).  A device double tensor for `images` (anything with data_ptr(), read on `stream`) runs
        srmap_register_flow_device: flow_out (required) and valid_out (optional) are device double buffers of those
        sizes, and the quality alone is returned."""
        device = hasattr(images, "data_ptr")
        if device:
            assert images.is_contiguous() and images.element_size() == 8 and images.dim() == 3
            n, H, W = (int(v) for v in images.shape)
        else:
            assert flow_out is None and valid_out is None, "flow_out / valid_out go with a device tensor for images"
            a, pa = _d(images)
            n, H, W = a.shape
        o, keep = _flow_options(n, hr_scale, init, warps, window_radius, damping, smooth_radius, valid_margin, max_levels, struct_size)
        s = max(1, int(hr_scale))
        q = np.zeros((n, 3))
        if device:
            assert flow_out is not None and flow_out.is_contiguous() and flow_out.element_size() == 8 and flow_out.numel() == n * 2 * s * s * H * W
            assert valid_out is None or (valid_out.is_contiguous() and valid_out.element_size() == 8 and valid_out.numel() == n * H * W)
            self.check(load().srmap_register_flow_device(self._h, n, W, H, C.c_void_p(images.data_ptr()), C.c_void_p(stream or 0),
                                                         C.byref(o), C.c_void_p(flow_out.data_ptr()),
                                                         C.c_void_p(valid_out.data_ptr()) if valid_out is not None else None,
                                                         q.ctypes.data_as(c_double_p)))
            return q
        flow, valid = np.zeros((n, 2, s * H, s * W)), np.zeros((n, H, W))
        self.check(load().srmap_register_flow(self._h, n, W, H, pa, C.byref(o), flow.ctypes.data_as(c_double_p),
                                              valid.ctypes.data_as(c_double_p), q.ctypes.data_as(c_double_p)))
        return flow, valid, q

    def pca(self, samples):
        """PCA of planar samples [rows][count] on the GPU: (mean, eigenvalues descending, basis rows = eigenvectors)."""
        a, pa = _d(samples)
        rows, count = a.shape
        mean, ev, basis = np.empty(rows), np.empty(rows), np.empty((rows, rows))
        self.check(load().srmap_channel_pca(self._h, rows, count, pa, mean.ctypes.data_as(c_double_p),
                                            ev.ctypes.data_as(c_double_p), basis.ctypes.data_as(c_double_p)))
        return mean, ev, basis

    def pca_device(self, in_ptr, rows, n, first, stride, count, stream=None):
        mean, ev, basis = np.empty(rows), np.empty(rows), np.empty((rows, rows))
        self.check(load().srmap_channel_pca_device(self._h, rows, n, C.c_void_p(in_ptr), first, stride, count,
                                                   mean.ctypes.data_as(c_double_p), ev.ctypes.data_as(c_double_p),
                                                   basis.ctypes.data_as(c_double_p), C.c_void_p(stream or 0)))
        return mean, ev, basis

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:  # at interpreter exit the module globals may be gone
            _lib.srmap_ctx_destroy(self._h)
            self._h = None


def flow_from_shifts(shifts, H, W):
    """The displacement field [K][2][H][W] of the translations shifts [K][2] = (dx, dy) in MotionShift's convention:
    u = (-dx, -dy) everywhere."""
    s = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    out = np.empty((len(s), 2, H, W))
    out[:, 0] = -s[:, 0, None, None]
    out[:, 1] = -s[:, 1, None, None]
    return out


def flow_from_affine(matrices, H, W):
    """The displacement field [K][2][H][W] of the affine maps matrices [K][2][3] = [a b tx; c d ty] (the convention of
    Problem.set_affine_motion): u(q) = F^-1(q) - q."""
    m = np.asarray(matrices, dtype=np.float64).reshape(-1, 2, 3)
    qy, qx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((len(m), 2, H, W))
    for k, F in enumerate(m):
        Li = np.linalg.inv(F[:, :2])
        ti = -Li @ F[:, 2]
        out[k, 0] = (Li[0, 0] * qx + (Li[0, 1] * qy + ti[0])) - qx
        out[k, 1] = (Li[1, 0] * qx + (Li[1, 1] * qy + ti[1])) - qy
    return out


def flow_lattice_expand(nodes, step, H, W, dtype=F64):
    """The dense field [K][2][H][W] of the lattice nodes [K][2][lh][lw] at `step` HR pixels between nodes, as the kernels
    interpolate it (srmap_problem_set_flow_lattice): bilinear at (x, y) / step clamped to the lattice, in double, rounded
    once to `dtype` (F32 or F64) and returned as doubles -- what Problem.set_flow then stores unchanged."""
    n = np.asarray(nodes, dtype=np.float64)
    lh, lw = n.shape[-2:]
    assert step >= 1 and lw >= 2 and lh >= 2
    cx = np.clip(np.arange(W, dtype=np.float64) / float(step), 0.0, lw - 1.0)
    cy = np.clip(np.arange(H, dtype=np.float64) / float(step), 0.0, lh - 1.0)
    xi = np.minimum(np.floor(cx).astype(np.int64), lw - 2)
    yi = np.minimum(np.floor(cy).astype(np.int64), lh - 2)
    fx, fy = (cx - xi)[None, :], (cy - yi)[:, None]
    Y, X = yi[:, None], xi[None, :]
    v = ((1 - fy) * ((1 - fx) * n[..., Y, X] + fx * n[..., Y, X + 1]) +
         fy * ((1 - fx) * n[..., Y + 1, X] + fx * n[..., Y + 1, X + 1]))
    return v.astype(np.float32).astype(np.float64) if dtype == F32 else v


def default_irls_options():
    o = IrlsOptions()
    load().srmap_irls_options_default(C.byref(o))
    return o


class Problem:
    def __init__(self, ctx, hr_width, hr_height, channels, frames, scale, shifts=None,
                 blur_ksize=0, blur_sigma=0.0, dtype=F64):
        self.ctx = ctx
        self.W, self.H, self.C, self.K, self.s = hr_width, hr_height, channels, frames, scale
        self.dtype = dtype
        d = ProblemDesc()
        d.hr_width, d.hr_height, d.channels, d.frames, d.scale = hr_width, hr_height, channels, frames, scale
        self._shifts = None
        if shifts is not None:
            self._shifts = np.ascontiguousarray(shifts, dtype=np.float64).reshape(-1, 2)
            assert len(self._shifts) == frames
            d.shifts_xy = self._shifts.ctypes.data_as(c_double_p)
        d.blur_ksize, d.blur_sigma, d.dtype = blur_ksize, blur_sigma, dtype
        self._h = C.c_void_p()
        ctx.check(load().srmap_problem_create(ctx._h, C.byref(d), C.byref(self._h)))
        lw, lh = C.c_int(), C.c_int()
        load().srmap_problem_lr_size(self._h, C.byref(lw), C.byref(lh))
        self.w, self.h = lw.value, lh.value
        self.nreg = 0

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:  # at interpreter exit the module globals may be gone
            _lib.srmap_problem_destroy(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def set_impl(self, impl):
        self.ctx.check(load().srmap_problem_set_impl(self._h, impl))

    def set_solver(self, solver, m=5):
        """Inner minimiser of solve(): SOLVER_CG (default) or SOLVER_LBFGS with m history pairs (1 <= m <= 8)."""
        self.ctx.check(load().srmap_problem_set_solver(self._h, solver, m))

    def set_affine_motion(self, matrices):
        """Per-frame affine motion [K][2][3] = [a b tx; c d ty] in HR pixel coordinates, (x, y) order: content at p sits at
        L p + t in frame k's HR-grid image.  None restores the motion the problem was created with."""
        if matrices is None:
            self.ctx.check(load().srmap_problem_set_affine_motion(self._h, None))
        else:
            a, pa = _d(matrices)
            assert a.size == self.K * 6, (a.shape, self.K)
            self.ctx.check(load().srmap_problem_set_affine_motion(self._h, pa))

    def set_flow(self, flow, stream=None):
        """Per-frame displacement field [K][2][H][W], the (ux, uy) planes in HR pixels: frame k's HR-grid image at q is x
        sampled bilinearly at q + u_k(q).  A host array (rounded once to the problem's dtype) or a device tensor of the
        problem's dtype (anything with data_ptr(); read on `stream`, None = the context's).  None restores the motion the
        problem was created with.  A flow and an affine motion are alternatives: setting one replaces the other."""
        n = self.K * 2 * self.H * self.W
        if flow is None:
            self.ctx.check(load().srmap_problem_set_flow(self._h, None))
        elif hasattr(flow, "data_ptr"):
            assert flow.numel() == n and flow.is_contiguous() and flow.element_size() == (4 if self.dtype == F32 else 8)
            self.ctx.check(load().srmap_problem_set_flow_device(self._h, C.c_void_p(flow.data_ptr()), C.c_void_p(stream or 0)))
        else:
            a, pa = _d(flow)
            assert a.size == n, (a.shape, self.K, self.H, self.W)
            self.ctx.check(load().srmap_problem_set_flow(self._h, pa))

    def flow(self):
        """The displacement field in force, [K][2][H][W] doubles, or None when no flow is set."""
        v = C.c_int(0)
        self.ctx.check(load().srmap_problem_get_flow(self._h, None, C.byref(v)))
        if not v.value:
            return None
        out = np.empty((self.K, 2, self.H, self.W))
        self.ctx.check(load().srmap_problem_get_flow(self._h, out.ctypes.data_as(c_double_p), C.byref(v)))
        return out

    def set_flow_lattice(self, nodes, step, stream=None):
        """The displacement field on a control lattice: nodes [K][2][lh][lw] doubles, node (i, j) at HR pixel
        (i step, j step); the kernels interpolate u (flow_lattice_expand).  A host array or a device tensor of doubles
        (anything with data_ptr(); read on `stream`, None = the context's).  None restores the motion the problem was
        created with.  Lattice, dense flow and affine motion are alternatives: setting one replaces the others."""
        if nodes is None:
            self.ctx.check(load().srmap_problem_set_flow_lattice(self._h, 0, 0, 0, None))
            return
        on_device = hasattr(nodes, "data_ptr")
        if not on_device:
            nodes = np.asarray(nodes, dtype=np.float64)
        shape = tuple(nodes.shape)
        assert len(shape) == 4 and shape[0] == self.K and shape[1] == 2, shape
        lh, lw = shape[2], shape[3]
        if on_device:
            assert nodes.is_contiguous() and str(nodes.dtype).endswith("float64"), "a device lattice is float64"
            self.ctx.check(load().srmap_problem_set_flow_lattice_device(self._h, step, lw, lh, C.c_void_p(nodes.data_ptr()),
                                                                        C.c_void_p(stream or 0)))
        else:
            a, pa = _d(nodes)
            self.ctx.check(load().srmap_problem_set_flow_lattice(self._h, step, lw, lh, pa))

    def flow_lattice(self):
        """(nodes [K][2][lh][lw] doubles, step) of the lattice in force, or None when none is set."""
        st, lw, lh = C.c_int(0), C.c_int(0), C.c_int(0)
        self.ctx.check(load().srmap_problem_get_flow_lattice(self._h, C.byref(st), C.byref(lw), C.byref(lh), None))
        if not st.value:
            return None
        out = np.empty((self.K, 2, lh.value, lw.value))
        self.ctx.check(load().srmap_problem_get_flow_lattice(self._h, C.byref(st), C.byref(lw), C.byref(lh), out.ctypes.data_as(c_double_p)))
        return out, st.value

    def set_blur_kernel(self, taps):
        """Free-form blur kernel [ksize][ksize] (odd, 1...7; the forward model correlates with it, the adjoint is its flip in
        both axes).  None restores the blur the problem was created with."""
        if taps is None:
            self.ctx.check(load().srmap_problem_set_blur_kernel(self._h, 0, None))
        else:
            a, pa = _d(taps)
            assert a.ndim == 2 and a.shape[0] == a.shape[1], a.shape
            self.ctx.check(load().srmap_problem_set_blur_kernel(self._h, a.shape[0], pa))

    def blur_kernel(self):
        """The blur in force, [ksize][ksize] ([[1]] without a blur)."""
        k = C.c_int(0)
        self.ctx.check(load().srmap_problem_get_blur_kernel(self._h, C.byref(k), None))
        out = np.empty((k.value, k.value))
        self.ctx.check(load().srmap_problem_get_blur_kernel(self._h, C.byref(k), out.ctypes.data_as(c_double_p)))
        return out

    def _fit(self, name, x, stream, *tail):
        """The fit entry point `name` on the HR image x: its host form for a host array [C][H][W], its _device form on `stream`
        for a device tensor (anything with data_ptr())."""
        if hasattr(x, "data_ptr"):
            assert x.numel() == self.C * self.H * self.W
            self.ctx.check(getattr(load(), name + "_device")(self._h, C.c_void_p(x.data_ptr()), C.c_void_p(stream or 0), *tail))
        else:
            a, pa = _d(x)
            assert a.size == self.C * self.H * self.W
            self.ctx.check(getattr(load(), name)(self._h, pa, *tail))

    @staticmethod
    def _blur_fit_options(ksize, sum_to_one, ridge, apply, struct_size):
        o = BlurFitOptions()
        load().srmap_blur_fit_options_default(C.byref(o))
        o.ksize, o.sum_to_one, o.ridge, o.apply = (0 if ksize is None else ksize), (1 if sum_to_one else 0), ridge, (1 if apply else 0)
        if struct_size is not None:
            o.struct_size = struct_size
        return o

    def fit_blur(self, x, ksize=None, sum_to_one=True, ridge=0.0, apply=True, stream=None, struct_size=None):
        """srmap_fit_blur: the ksize x ksize taps that best explain the observations from the KNOWN HR image x (a host array
        [C][H][W], or a device tensor of the problem's dtype, read on `stream`).  ksize None = the size of the kernel in
        force.  Returns (taps [ksize][ksize], quality [5] = E at the kernel in force, E at the fit, smallest / largest pivot,
        status, sums = the upper triangle of the Gram of [s_0 ... s_{n-1}, y]).  apply installs the fit as set_blur_kernel
        would.  struct_size overrides the options' size field (tests)."""
        o = self._blur_fit_options(ksize, sum_to_one, ridge, apply, struct_size)
        kk = ksize if ksize else self.blur_kernel().shape[0]
        n = max(kk, 1) ** 2
        taps, q, ne = np.zeros(n), np.zeros(5), np.zeros((n + 1) * (n + 2) // 2)
        self._fit("srmap_fit_blur", x, stream, C.byref(o), taps.ctypes.data_as(c_double_p), q.ctypes.data_as(c_double_p), ne.ctypes.data_as(c_double_p))
        k = int(round(np.sqrt(n)))
        return taps.reshape(k, k), q, ne

    def _bank_entries(self, mode):
        return {BLUR_PER_FRAME: self.K, BLUR_PER_CHANNEL: self.C, BLUR_PER_FRAME_CHANNEL: self.K * self.C}[mode]

    def set_blur_bank(self, taps, mode=None):
        """Blur-kernel bank: a kernel per frame [K][b][b] (BLUR_PER_FRAME), per channel [C][b][b] (BLUR_PER_CHANNEL) or per
        (frame, channel) [K][C][b][b] (BLUR_PER_FRAME_CHANNEL); every entry as set_blur_kernel takes its kernel.  The mode is
        inferred from the array's shape where that is unambiguous and required for a [n][b][b] array when K == C.  None
        restores the blur the problem was created with."""
        if taps is None:
            self.ctx.check(load().srmap_problem_set_blur_bank(self._h, 0, 0, None))
            return
        a, pa = _d(taps)
        if mode is None:
            if a.ndim == 4:
                mode = BLUR_PER_FRAME_CHANNEL
            elif a.ndim == 3 and self.K != self.C and a.shape[0] in (self.K, self.C):
                mode = BLUR_PER_FRAME if a.shape[0] == self.K else BLUR_PER_CHANNEL
            else:
                raise ValueError("set_blur_bank: the mode cannot be inferred from shape %s with K = %d, C = %d" % (a.shape, self.K, self.C))
        if mode in (BLUR_PER_FRAME, BLUR_PER_CHANNEL, BLUR_PER_FRAME_CHANNEL):
            lead = (self.K, self.C) if mode == BLUR_PER_FRAME_CHANNEL else (self._bank_entries(mode),)
            if a.shape[:-2] != lead or a.ndim < 3 or a.shape[-1] != a.shape[-2]:
                raise ValueError("set_blur_bank: shape %s is not %s + (b, b)" % (a.shape, lead))
        self.ctx.check(load().srmap_problem_set_blur_bank(self._h, mode, a.shape[-1], pa))

    def blur_bank(self):
        """(mode, taps) of the bank in force -- taps [K][b][b], [C][b][b] or [K][C][b][b] -- or (0, None) when none is set."""
        m, k = C.c_int(0), C.c_int(0)
        self.ctx.check(load().srmap_problem_get_blur_bank(self._h, C.byref(m), C.byref(k), None))
        if m.value == 0:
            return 0, None
        lead = (self.K, self.C) if m.value == BLUR_PER_FRAME_CHANNEL else (self._bank_entries(m.value),)
        out = np.empty(lead + (k.value, k.value))
        self.ctx.check(load().srmap_problem_get_blur_bank(self._h, C.byref(m), C.byref(k), out.ctypes.data_as(c_double_p)))
        return m.value, out

    def fit_blur_bank(self, x, mode, ksize=None, sum_to_one=True, ridge=0.0, apply=True, stream=None, struct_size=None):
        """srmap_fit_blur_bank: fit_blur's quadratic solved separately over the observations of each entry of `mode`, from
        the KNOWN HR image x (a host array [C][H][W], or a device tensor of the problem's dtype, read on `stream`).  Returns
        (taps [entries...][ksize][ksize], quality [entries][5] in fit_blur's layout -- status 0 fitted, 3 degenerate: the
        entry keeps its kernel --, sums [entries][(n + 1)(n + 2) / 2]).  apply installs the result as set_blur_bank would.
        A calibration fit: blind alternation with a solve is not offered."""
        o = self._blur_fit_options(ksize, sum_to_one, ridge, apply, struct_size)
        kc = C.c_int(0)
        self.ctx.check(load().srmap_problem_get_blur_kernel(self._h, C.byref(kc), None))
        kk = ksize if ksize else kc.value
        n = max(kk, 1) ** 2
        entries = self._bank_entries(mode) if mode in (BLUR_PER_FRAME, BLUR_PER_CHANNEL, BLUR_PER_FRAME_CHANNEL) else 1
        taps, q, ne = np.zeros((entries, n)), np.zeros((entries, 5)), np.zeros((entries, (n + 1) * (n + 2) // 2))
        self._fit("srmap_fit_blur_bank", x, stream, mode, C.byref(o), taps.ctypes.data_as(c_double_p), q.ctypes.data_as(c_double_p), ne.ctypes.data_as(c_double_p))
        k = int(round(np.sqrt(n)))
        lead = (self.K, self.C) if mode == BLUR_PER_FRAME_CHANNEL else (entries,)
        return taps.reshape(lead + (k, k)), q, ne

    def set_cost_rows(self, hr_row0, hr_row1):
        """Row-band sharding: count only the cost terms of HR rows [hr_row0, hr_row1)."""
        self.ctx.check(load().srmap_problem_set_cost_rows(self._h, hr_row0, hr_row1))

    def set_observations(self, lr):
        a, pa = _d(lr)
        assert a.size == self.K * self.C * self.h * self.w, (a.shape, self.K, self.C, self.h, self.w)
        self.ctx.check(load().srmap_set_observations(self._h, pa))

    def active_impl(self):
        v = C.c_int(-1)
        self.ctx.check(load().srmap_problem_active_impl(self._h, C.byref(v)))
        return v.value

    def set_observations_device(self, ptr, stream=None):
        self.ctx.check(load().srmap_set_observations_device(self._h, C.c_void_p(ptr), C.c_void_p(stream or 0)))

    def add_regularizer(self, kind, lam, btv_range=0, btv_decay=0.0):
        idx = C.c_int(-1)
        self.ctx.check(load().srmap_add_regularizer(self._h, kind, lam, btv_range, btv_decay, C.byref(idx)))
        self.nreg += 1
        return idx.value

    def clear_regularizers(self):
        self.ctx.check(load().srmap_clear_regularizers(self._h))
        self.nreg = 0

    def set_irls_weights(self, reg, w):
        if w is None:
            self.ctx.check(load().srmap_set_irls_weights(self._h, reg, None))
        else:
            a, pa = _d(w)
            assert a.size == self.C * self.H * self.W
            self.ctx.check(load().srmap_set_irls_weights(self._h, reg, pa))

    def update_irls_weights_device(self, reg, x_ptr, stream=None):
        self.ctx.check(load().srmap_update_irls_weights_device(self._h, reg, C.c_void_p(x_ptr), C.c_void_p(stream or 0)))

    def set_data_weights(self, w):
        """Per-observation weights of the data term, [K][C][h][w] like the observations; None = all ones."""
        if w is None:
            self.ctx.check(load().srmap_set_data_weights(self._h, None))
        else:
            a, pa = _d(w)
            assert a.size == self.K * self.C * self.h * self.w, (a.shape, self.K, self.C, self.h, self.w)
            self.ctx.check(load().srmap_set_data_weights(self._h, pa))

    def set_data_weights_device(self, ptr, stream=None):
        self.ctx.check(load().srmap_set_data_weights_device(self._h, C.c_void_p(ptr), C.c_void_p(stream or 0)))

    def data_weights(self):
        """The current data weights [K][C][h][w] (ones if none are set); after a Huber solve, the outlier map."""
        out = np.empty((self.K, self.C, self.h, self.w))
        self.ctx.check(load().srmap_get_data_weights(self._h, out.ctypes.data_as(c_double_p)))
        return out

    def set_data_prior(self, m, stream=None):
        """Persistent prior on the data weights, [K][C][h][w]: every kernel reads m .* w, also under a Huber loss (whose
        re-weighting gives m .* huber(r)).  A host array, or a device tensor of the problem's dtype (anything with
        data_ptr(), read on `stream`); None removes it."""
        n = self.K * self.C * self.h * self.w
        if m is None:
            self.ctx.check(load().srmap_set_data_prior(self._h, None))
        elif hasattr(m, "data_ptr"):
            assert m.numel() == n and m.is_contiguous() and m.element_size() == (4 if self.dtype == F32 else 8)
            self.ctx.check(load().srmap_set_data_prior_device(self._h, C.c_void_p(m.data_ptr()), C.c_void_p(stream or 0)))
        else:
            a, pa = _d(m)
            assert a.size == n, (a.shape, self.K, self.C, self.h, self.w)
            self.ctx.check(load().srmap_set_data_prior(self._h, pa))

    def data_prior(self):
        """The prior in force, [K][C][h][w] doubles, or None when none is set."""
        v = C.c_int(0)
        self.ctx.check(load().srmap_get_data_prior(self._h, None, C.byref(v)))
        if not v.value:
            return None
        out = np.empty((self.K, self.C, self.h, self.w))
        self.ctx.check(load().srmap_get_data_prior(self._h, out.ctypes.data_as(c_double_p), C.byref(v)))
        return out

    def register_flow(self, channel=-1, init=None, prior=True, hr_scale=1, warps=8, window_radius=4, damping=0.05,
                      smooth_radius=2, valid_margin=3, max_levels=0, struct_size=None):
        """srmap_problem_register_flow: register the problem's own observations (channel, or -1 = the channel mean) on
        the device and install the field as set_flow would; prior: the validity masks become the data prior.  Returns
        the quality [K][3], also when the field is refused (SrmapError with .quality set)."""
        o, keep = _flow_options(self.K, hr_scale, init, warps, window_radius, damping, smooth_radius, valid_margin, max_levels, struct_size)
        q = np.zeros((self.K, 3))
        try:
            self.ctx.check(load().srmap_problem_register_flow(self._h, channel, C.byref(o), 1 if prior else 0, q.ctypes.data_as(c_double_p)))
        except SrmapError as e:
            e.quality = q
            raise
        return q

    def register_flow_lattice(self, channel=-1, init=None, prior=True, hr_scale=1, warps=8, window_radius=4, damping=0.05,
                              smooth_radius=2, valid_margin=3, max_levels=0, struct_size=None):
        """srmap_problem_register_flow_lattice: register_flow that stops at the input level and installs the estimate as
        a lattice (step = scale on the LR grid), without forming the HR field.  Returns the quality [K][3], also when the
        lattice is refused (SrmapError with .quality set)."""
        o, keep = _flow_options(self.K, hr_scale, init, warps, window_radius, damping, smooth_radius, valid_margin, max_levels, struct_size)
        q = np.zeros((self.K, 3))
        try:
            self.ctx.check(load().srmap_problem_register_flow_lattice(self._h, channel, C.byref(o), 1 if prior else 0, q.ctypes.data_as(c_double_p)))
        except SrmapError as e:
            e.quality = q
            raise
        return q

    def set_data_loss(self, loss, huber_delta=0.0):
        """DATA_LOSS_L2 (default) or DATA_LOSS_HUBER with its delta (> 0, in the observations' units)."""
        self.ctx.check(load().srmap_problem_set_data_loss(self._h, loss, huber_delta))

    def update_data_weights_device(self, x_ptr, stream=None):
        """One Huber re-weighting step from the residuals at the device image x_ptr."""
        self.ctx.check(load().srmap_update_data_weights_device(self._h, C.c_void_p(x_ptr), C.c_void_p(stream or 0)))

    def set_huber_scale(self, mode, tuning=1.345, min_delta=1e-4):
        """HUBER_DELTA_FIXED (default: set_data_loss's delta) or HUBER_DELTA_MAD: every Huber re-weighting uses
        delta = max(tuning * 1.4826 * median|r|, min_delta) of its own residuals over all frames."""
        self.ctx.check(load().srmap_problem_set_huber_scale(self._h, mode, tuning, min_delta))

    def huber_delta(self):
        """(mode, delta, scales [1 + K], counts [1 + K]) of the last Huber step; the fixed delta and zeros in the FIXED mode."""
        mode, delta = C.c_int(0), C.c_double(0.0)
        scales, counts = np.zeros(1 + self.K), np.zeros(1 + self.K)
        self.ctx.check(load().srmap_problem_get_huber_delta(self._h, C.byref(mode), C.byref(delta), scales.ctypes.data_as(c_double_p),
                                                            counts.ctypes.data_as(c_double_p)))
        return mode.value, delta.value, scales, counts

    def residual_scale(self, x, stream=None):
        """srmap_residual_scale: (scales [1 + K], counts [1 + K]) at the HR image x (a host array [C][H][W], or a device
        tensor of the problem's dtype, read on `stream`): scales[0] = 1.4826 * the lower median of |A x - y| over all
        counted observations, scales[1 + k] of frame k alone."""
        scales, counts = np.zeros(1 + self.K), np.zeros(1 + self.K)
        self._fit("srmap_residual_scale", x, stream, scales.ctypes.data_as(c_double_p), counts.ctypes.data_as(c_double_p))
        return scales, counts

    def set_holdout(self, fraction, seed=1):
        """srmap_problem_set_holdout: keep the share `fraction` (0 < fraction <= 0.5) of the observations, chosen by a hash
        of (index, seed), out of the data term; 0 lifts the hold-out."""
        self.ctx.check(load().srmap_problem_set_holdout(self._h, fraction, seed))

    def set_holdout_fold(self, folds, fold, seed=1):
        """srmap_problem_set_holdout_fold: hold out fold `fold` of the partition of the observations into `folds` (2...32)
        folds by the hash of (index, seed); folds 0 lifts the hold-out.  Replaces a fraction, and is replaced by one."""
        self.ctx.check(load().srmap_problem_set_holdout_fold(self._h, folds, fold, seed))

    def holdout_fold(self):
        """(folds, fold, seed) of the fold in force; folds 0: none, or a fraction is set."""
        folds, fold, seed = C.c_int(0), C.c_int(0), C.c_ulonglong(0)
        self.ctx.check(load().srmap_problem_get_holdout_fold(self._h, C.byref(folds), C.byref(fold), C.byref(seed)))
        return folds.value, fold.value, seed.value

    def holdout(self, want_mask=True):
        """(fraction, seed, mask [K][C][h][w] of 0 / 1 or None, counts [1 + K]) of the hold-out in force; fraction 0: none."""
        fr, seed = C.c_double(0.0), C.c_ulonglong(0)
        mask = np.zeros((self.K, self.C, self.h, self.w)) if want_mask else None
        counts = np.zeros(1 + self.K)
        self.ctx.check(load().srmap_problem_get_holdout(self._h, C.byref(fr), C.byref(seed),
                                                        mask.ctypes.data_as(c_double_p) if want_mask else None,
                                                        counts.ctypes.data_as(c_double_p)))
        return fr.value, seed.value, mask, counts

    def holdout_score(self, x, delta=None, stream=None):
        """srmap_holdout_score at the HR image x (a host array [C][H][W], or a device tensor of the problem's dtype, read on
        `stream`): (score [1 + K], sums [1 + K][4] = S1, S2, S0, n) over the held-out observations.  delta: 0 = squared
        residuals, > 0 = the Huber function, None = the problem's."""
        score, sums = np.zeros(1 + self.K), np.zeros((1 + self.K, 4))
        self._fit("srmap_holdout_score", x, stream, -1.0 if delta is None else float(delta), score.ctypes.data_as(c_double_p),
                  sums.ctypes.data_as(c_double_p))
        return score, sums

    def set_regularizer_lambda(self, reg, lam):
        """The regularization parameter of regulariser `reg`, changed in place (its IRLS weights stay)."""
        self.ctx.check(load().srmap_problem_set_regularizer_lambda(self._h, reg, lam))

    def regularizer_lambda(self, reg):
        v = C.c_double(0.0)
        self.ctx.check(load().srmap_problem_get_regularizer_lambda(self._h, reg, C.byref(v)))
        return v.value

    def set_regularizer_gradient(self, reg, mode):
        """The gradient regulariser `reg` contributes: REG_GRADIENT_REFERENCE (the reference's, bug for bug; the default) or
        REG_GRADIENT_EXACT (the gradient of the cost).  The cost, the values and the IRLS weights are the same in both."""
        self.ctx.check(load().srmap_problem_set_regularizer_gradient(self._h, reg, mode))

    def regularizer_gradient(self, reg):
        v = C.c_int(0)
        self.ctx.check(load().srmap_problem_get_regularizer_gradient(self._h, reg, C.byref(v)))
        return v.value

    def solve_lambda_path(self, x0, scales, options=None, patience=0, final_solve=True, struct_size=None):
        """srmap_solve_lambda_path: one solve from x0 per multiplier in `scales` (strictly decreasing) of the problem's
        lambdas, each scored on the held-out observations.  Returns (x, table [rows_run][11] = scale, score, S1, S2, S0, n,
        IRLS rounds, iterations, evaluations, final cost, delta used; chosen; report): x is the solve on all observations
        at the chosen lambdas (final_solve) or the chosen row's solution.  struct_size overrides the options' size field
        (tests)."""
        a, pa = _d(x0)
        assert a.size == self.C * self.H * self.W
        po = LambdaPathOptions()
        load().srmap_lambda_path_options_default(C.byref(po))
        sc = [float(v) for v in scales]
        po.num_scales = len(sc)
        for j in range(LAMBDA_PATH_MAX_SCALES):
            po.scales[j] = sc[j] if j < len(sc) else 0.0
        po.patience, po.final_solve = patience, 1 if final_solve else 0
        if struct_size is not None:
            po.struct_size = struct_size
        out = np.empty((self.C, self.H, self.W))
        table = np.zeros((max(1, min(len(sc), LAMBDA_PATH_MAX_SCALES)), LAMBDA_PATH_ROW))
        rows, chosen, rep = C.c_int(0), C.c_int(-1), SolveReport()
        o = options if options is not None else default_irls_options()
        self.ctx.check(load().srmap_solve_lambda_path(self._h, C.byref(o), C.byref(po), pa, out.ctypes.data_as(c_double_p),
                                                      table.ctypes.data_as(c_double_p), C.byref(rows), C.byref(chosen), C.byref(rep)))
        return out, table[:rows.value].copy(), chosen.value, rep

    def solve_lambda_path_folds(self, x0, scales, folds=5, seed=1, rule="one_se", se_factor=1.0, options=None, patience=0,
                                final_solve=True, struct_size=None):
        """srmap_solve_lambda_path_folds: per multiplier in `scales` one solve from x0 and one score for every fold of the
        partition into `folds`; rule "min" chooses the least mean score, "one_se" the largest lambda whose mean is within
        se_factor standard errors (over the folds) of it.  Returns (x, table [rows_run][11] = scale, mean, se, pooled S1, S2,
        S0, n, summed IRLS rounds, iterations, evaluations, delta used; fold_table [rows_run][folds][11] in
        solve_lambda_path's layout; chosen; report): x and report are the solve on all observations at the chosen lambdas,
        None without final_solve.  The hold-out in force at the call is in force on return.  struct_size overrides the
        options' size field (tests)."""
        a, pa = _d(x0)
        assert a.size == self.C * self.H * self.W
        po = LambdaCvOptions()
        load().srmap_lambda_cv_options_default(C.byref(po))
        sc = [float(v) for v in scales]
        po.num_scales = len(sc)
        for j in range(LAMBDA_PATH_MAX_SCALES):
            po.scales[j] = sc[j] if j < len(sc) else 0.0
        po.folds, po.seed, po.se_factor = folds, seed, se_factor
        po.rule = LAMBDA_RULES[rule] if isinstance(rule, str) else rule
        po.patience, po.final_solve = patience, 1 if final_solve else 0
        if struct_size is not None:
            po.struct_size = struct_size
        out = np.empty((self.C, self.H, self.W)) if final_solve else None
        nrows, nf = max(1, min(len(sc), LAMBDA_PATH_MAX_SCALES)), max(1, min(int(folds), 32))
        table, fold_table = np.zeros((nrows, LAMBDA_PATH_ROW)), np.zeros((nrows, nf, LAMBDA_PATH_ROW))
        rows, chosen, rep = C.c_int(0), C.c_int(-1), SolveReport()
        o = options if options is not None else default_irls_options()
        self.ctx.check(load().srmap_solve_lambda_path_folds(self._h, C.byref(o), C.byref(po), pa,
                                                            out.ctypes.data_as(c_double_p) if final_solve else None,
                                                            table.ctypes.data_as(c_double_p), fold_table.ctypes.data_as(c_double_p),
                                                            C.byref(rows), C.byref(chosen), C.byref(rep)))
        return out, table[:rows.value].copy(), fold_table[:rows.value].copy(), chosen.value, rep if final_solve else None

    def apply(self, hr, k):
        a, pa = _d(hr)
        assert a.size == self.C * self.H * self.W
        out = np.empty((self.C, self.h, self.w))
        self.ctx.check(load().srmap_apply(self._h, k, pa, out.ctypes.data_as(c_double_p)))
        return out

    def apply_transpose(self, lr, k):
        a, pa = _d(lr)
        assert a.size == self.C * self.h * self.w
        out = np.empty((self.C, self.H, self.W))
        self.ctx.check(load().srmap_apply_transpose(self._h, k, pa, out.ctypes.data_as(c_double_p)))
        return out

    def reg_values(self, reg, x):
        a, pa = _d(x)
        out = np.empty((self.C, self.H, self.W))
        self.ctx.check(load().srmap_reg_values(self._h, reg, pa, out.ctypes.data_as(c_double_p)))
        return out

    def reg_values_and_gradient(self, reg, x, gc):
        a, pa = _d(x)
        g, pg = _d(gc)
        vals = np.empty((self.C, self.H, self.W))
        grad = np.empty((self.C, self.H, self.W))
        self.ctx.check(load().srmap_reg_values_and_gradient(
            self._h, reg, pa, pg, vals.ctypes.data_as(c_double_p), grad.ctypes.data_as(c_double_p)))
        return vals, grad

    def eval(self, x, terms=TERM_ALL, want_grad=True):
        a, pa = _d(x)
        assert a.size == self.C * self.H * self.W
        cost = C.c_double()
        g = np.empty((self.C, self.H, self.W)) if want_grad else None
        self.ctx.check(load().srmap_eval(self._h, terms, pa, C.byref(cost),
                                         g.ctypes.data_as(c_double_p) if want_grad else None))
        return cost.value, g

    def eval_device(self, x_ptr, g_ptr, terms=TERM_ALL, want_cost=False, stream=None):
        cost = C.c_double()
        self.ctx.check(load().srmap_eval_device(self._h, terms, C.c_void_p(x_ptr),
                                                C.c_void_p(g_ptr) if g_ptr else None,
                                                C.byref(cost) if want_cost else None,
                                                C.c_void_p(stream) if stream else None))
        return cost.value if want_cost else None

    def last_cost(self):
        cost = C.c_double()
        self.ctx.check(load().srmap_last_cost(self._h, C.byref(cost)))
        return cost.value

    def solve(self, x0, options=None, comm=None, shard=None):
        """IRLSMapSolver::Solve; with a Comm and a ShardDesc: this rank's shard of the joint solve."""
        a, pa = _d(x0)
        assert a.size == self.C * self.H * self.W
        out = np.empty((self.C, self.H, self.W))
        rep = SolveReport()
        o = options if options is not None else default_irls_options()
        if comm is None:
            st = load().srmap_solve(self._h, C.byref(o), pa, out.ctypes.data_as(c_double_p), C.byref(rep))
        else:
            st = load().srmap_solve_sharded(self._h, comm._h, C.byref(shard), C.byref(o), pa,
                                            out.ctypes.data_as(c_double_p), C.byref(rep))
        self.ctx.check(st)
        return out, rep

    def refine_motion(self, x, dof=6, max_iterations=30, step_tolerance=1e-4, initial_damping=1e-3, apply=True, initial=None,
                      stream=None, struct_size=None):
        """srmap_refine_motion: re-fit the frame matrices to the HR estimate x through the forward model.  x: a host array
        [C][H][W], or a device tensor of the problem's dtype (anything with data_ptr(); it is read on `stream`, None = the
        context's stream, so it must be complete there).  initial: [K][2][3] starting matrices instead of the problem's
        motion.  Returns (matrices [K][2][3], quality [K][4] = cost at the start, cost at the result, passes, status,
        normal equations [K][28]).  apply installs the result as set_affine_motion would.  struct_size overrides the
        options' size field (tests)."""
        o = MotionRefinementOptions()
        load().srmap_motion_refinement_options_default(C.byref(o))
        o.dof, o.max_iterations, o.step_tolerance, o.initial_damping = dof, max_iterations, step_tolerance, initial_damping
        o.apply = 1 if apply else 0
        if struct_size is not None:
            o.struct_size = struct_size
        if initial is not None:
            ini, pi = _d(initial)
            assert ini.size == self.K * 6, (ini.shape, self.K)
            o.initial_affine_2x3 = pi
        out, q, ne = np.zeros((self.K, 2, 3)), np.zeros((self.K, 4)), np.zeros((self.K, 28))
        self._fit("srmap_refine_motion", x, stream, C.byref(o), out.ctypes.data_as(c_double_p), q.ctypes.data_as(c_double_p), ne.ctypes.data_as(c_double_p))
        return out, q, ne

    def solve_joint(self, x0, options=None, rounds=3, **refine):
        """Joint estimation: a solve from x0, then `rounds` times (refine_motion at the current x, a solve warm-started from
        it).  Returns (x, [SolveReport per solve], [(matrices, quality) per refinement]); refine: refine_motion's keywords."""
        x, rep = self.solve(x0, options)
        reports, refinements = [rep], []
        for _ in range(rounds):
            mats, q, _ = self.refine_motion(x, apply=True, **refine)
            refinements.append((mats, q))
            x, rep = self.solve(x, options)
            reports.append(rep)
        return x, reports, refinements

    def set_photometric(self, gain_bias):
        """Per-frame photometric parameters [K][2] = (gain, bias): the problem then solves against (y - bias) / gain.  None
        restores the raw observations bit for bit."""
        if gain_bias is None:
            self.ctx.check(load().srmap_problem_set_photometric(self._h, None))
        else:
            a, pa = _d(gain_bias)
            assert a.size == self.K * 2, (a.shape, self.K)
            self.ctx.check(load().srmap_problem_set_photometric(self._h, pa))

    def photometric(self):
        """(parameters in force [K][2], ones and zeros when none are set; whether any are set)."""
        out, flag = np.empty((self.K, 2)), C.c_int(0)
        self.ctx.check(load().srmap_problem_get_photometric(self._h, out.ctypes.data_as(c_double_p), C.byref(flag)))
        return out, bool(flag.value)

    def fit_photometric(self, x, model=0, gauge_frame=0, min_gain=0.25, max_gain=4.0, apply=True, stream=None, struct_size=None):
        """srmap_fit_photometric: per frame the (gain, bias) that best map the model's prediction from the HR image x (a host
        array [C][H][W], or a device tensor of the problem's dtype, read on `stream`) onto the RAW observations.  model: 0
        gain and bias, 1 gain only, 2 bias only; gauge_frame keeps its parameters (-1: none).  Returns (gain_bias [K][2],
        quality [K][4] = E at the parameters in force, E at the result, sum of the weights, status, sums [K][6]).  apply
        installs the result as set_photometric would.  struct_size overrides the options' size field (tests)."""
        o = PhotometricFitOptions()
        load().srmap_photometric_fit_options_default(C.byref(o))
        o.model, o.gauge_frame, o.min_gain, o.max_gain, o.apply = model, gauge_frame, min_gain, max_gain, (1 if apply else 0)
        if struct_size is not None:
            o.struct_size = struct_size
        gb, q, sums = np.zeros((self.K, 2)), np.zeros((self.K, 4)), np.zeros((self.K, 6))
        self._fit("srmap_fit_photometric", x, stream, C.byref(o), gb.ctypes.data_as(c_double_p), q.ctypes.data_as(c_double_p), sums.ctypes.data_as(c_double_p))
        return gb, q, sums

    def solve_photometric(self, x0, options=None, rounds=3, **fit):
        """Exposure-compensated solve: fit_photometric at x0, a solve from x0, then `rounds` times (fit_photometric at the
        current x, a solve warm-started from it).  Returns (x, [SolveReport per solve], [(gain_bias, quality) per fit]);
        fit: fit_photometric's keywords."""
        gb, q, _ = self.fit_photometric(x0, apply=True, **fit)
        fits = [(gb, q)]
        x, rep = self.solve(x0, options)
        reports = [rep]
        for _ in range(rounds):
            gb, q, _ = self.fit_photometric(x, apply=True, **fit)
            fits.append((gb, q))
            x, rep = self.solve(x, options)
            reports.append(rep)
        return x, reports, fits

    def selfcheck(self):
        """Largest relative deviation of the solver's derived beta denominator from the directly summed y.dk (host-paced solves)."""
        v = C.c_double(0.0)
        self.ctx.check(load().srmap_problem_selfcheck(self._h, C.byref(v)))
        return v.value

    def eval_sharded_device(self, comm, shard, x_ptr, g_ptr, terms=TERM_ALL, want_cost=False, stream=None):
        cost = C.c_double()
        self.ctx.check(load().srmap_eval_sharded_device(
            self._h, comm._h if comm is not None else None, C.byref(shard) if shard is not None else None, terms,
            C.c_void_p(x_ptr), C.c_void_p(g_ptr) if g_ptr else None, C.byref(cost) if want_cost else None,
            C.c_void_p(stream) if stream else None))
        return cost.value if want_cost else None

    def cg_trace(self, x0, epsg=0.0, epsf=0.0, epsx=0.0, maxits=0, cap=4096):
        """One nonlinear-CG run; returns (x, iterations, nfev, termination, [f of every evaluation])."""
        a, pa = _d(x0)
        out = np.empty((self.C, self.H, self.W))
        its, nfev, term, tl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        tr = np.zeros(cap)
        self.ctx.check(load().srmap_cg_trace(self._h, epsg, epsf, epsx, maxits, pa, out.ctypes.data_as(c_double_p),
                                             C.byref(its), C.byref(nfev), C.byref(term),
                                             tr.ctypes.data_as(c_double_p), cap, C.byref(tl)))
        return out, its.value, nfev.value, term.value, tr[:min(cap, tl.value)].copy()

    def lbfgs_trace(self, x0, m=5, epsg=0.0, epsf=0.0, epsx=0.0, maxits=0, cap=4096):
        """One L-BFGS run with m history pairs; returns (x, iterations, nfev, termination, [f of every evaluation])."""
        a, pa = _d(x0)
        out = np.empty((self.C, self.H, self.W))
        its, nfev, term, tl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        tr = np.zeros(cap)
        self.ctx.check(load().srmap_lbfgs_trace(self._h, m, epsg, epsf, epsx, maxits, pa, out.ctypes.data_as(c_double_p),
                                                C.byref(its), C.byref(nfev), C.byref(term),
                                                tr.ctypes.data_as(c_double_p), cap, C.byref(tl)))
        return out, its.value, nfev.value, term.value, tr[:min(cap, tl.value)].copy()


class Comm:
    """srmap_comm: RCCL (ranks on different GPUs) or host callbacks over a torch.distributed group (gloo / any)."""

    def __init__(self, ctx, rank, world, backend="rccl", unique_id=None, dist=None, group=None, group_ranks=None):
        self.ctx, self.rank, self.world = ctx, rank, world
        self._h = C.c_void_p()
        self._keep = None
        if backend == "rccl":
            assert unique_id is not None and len(unique_id) == 128
            ctx.check(load().srmap_comm_create_rccl(ctx._h, unique_id, rank, world, C.byref(self._h)))
        else:
            import torch

            def _arr(ptr, count, dtype):
                ct = C.c_float if dtype == F32 else C.c_double
                return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(count,))

            def _ar(buf, count, dtype, op, _user):
                try:
                    t = torch.from_numpy(_arr(buf, count, dtype))
                    dist.all_reduce(t, op=dist.ReduceOp.MAX if op == 1 else dist.ReduceOp.SUM, group=group)
                    return 0
                except Exception as e:  # pragma: no cover
                    print("host all-reduce failed:", e)
                    return 1

            def _sr(send, sbytes, dst, recv, rbytes, src, _user):
                try:
                    reqs = []
                    if dst >= 0 and sbytes:
                        ts = torch.from_numpy(np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_uint8)), shape=(sbytes,)).copy())
                        reqs.append(dist.isend(ts, group_ranks[dst] if group_ranks else dst, group=group))
                    tr = None
                    if src >= 0 and rbytes:
                        tr = torch.empty(rbytes, dtype=torch.uint8)
                        reqs.append(dist.irecv(tr, group_ranks[src] if group_ranks else src, group=group))
                    for r in reqs:
                        r.wait()
                    if tr is not None:
                        np.ctypeslib.as_array(C.cast(recv, C.POINTER(C.c_uint8)), shape=(rbytes,))[:] = tr.numpy()
                    return 0
                except Exception as e:  # pragma: no cover
                    print("host send/recv failed:", e)
                    return 1

            self._keep = (HOST_ALLREDUCE_FN(_ar), HOST_SENDRECV_FN(_sr))
            ctx.check(load().srmap_comm_create_host(ctx._h, rank, world, self._keep[0], self._keep[1], None, C.byref(self._h)))

    def allreduce(self, dev_ptr, count, dtype=F64, op=0, stream=None):
        self.ctx.check(load().srmap_comm_allreduce(self._h, C.c_void_p(dev_ptr), count, dtype, op,
                                                   C.c_void_p(stream) if stream else None))

    def info(self):
        """(rank, size, backend) as the communicator itself reports them (size = ncclCommCount for RCCL; backend 1 = RCCL)."""
        r, w, b = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(load().srmap_comm_info(self._h, C.byref(r), C.byref(w), C.byref(b)))
        return r.value, w.value, b.value

    def set_overlap(self, on):
        """Row shards: halo exchange under the interior tile rows (default: host backend on, RCCL off)."""
        self.ctx.check(load().srmap_comm_set_overlap(self._h, 1 if on else 0))

    def describe(self):
        """'rccl <version> <path of the loaded librccl>' or 'host callbacks'."""
        buf = C.create_string_buffer(512)
        self.ctx.check(load().srmap_comm_describe(self._h, buf, C.c_size_t(512)))
        return buf.value.decode()

    def split(self, color, key, new_rank, new_world):
        """ncclCommSplit (RCCL backend): the ranks passing the same color form a new communicator."""
        c = Comm.__new__(Comm)
        c.ctx, c.rank, c.world, c._keep = self.ctx, new_rank, new_world, None
        c._h = C.c_void_p()
        self.ctx.check(load().srmap_comm_split(self._h, color, key, new_rank, new_world, C.byref(c._h)))
        return c

    @staticmethod
    def unique_id(ctx):
        buf = C.create_string_buffer(128)
        ctx.check(load().srmap_comm_get_unique_id(ctx._h, buf))
        return buf.raw

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:  # at interpreter exit the module globals may be gone
            _lib.srmap_comm_destroy(self._h)
            self._h = None
