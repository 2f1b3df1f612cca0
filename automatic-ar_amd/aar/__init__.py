"""ctypes binding of libaar.so -- the C ABI declared in include/aar.h.

This is test / benchmark plumbing: the product is the C-ABI library (HIP kernels for gfx950) and the C++
MultiCamMapper mirror in automatic-ar_amd/host/.  Nothing here computes; every numeric call lands in a
HIP kernel and raises AarError(AAR_ERR_NO_DEVICE) on a machine without a GPU -- there is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AAR_LIB") or os.path.join(os.path.dirname(_HERE), "libaar.so")   # AAR_LIB: A/B runs of two builds

AAR_OK = 0
AAR_ERR_INVALID, AAR_ERR_NO_DEVICE, AAR_ERR_HIP, AAR_ERR_UNSUPPORTED = -1, -2, -3, -4
AAR_ERR_NUMERIC, AAR_ERR_IO, AAR_ERR_COMM = -5, -6, -7
RES_F32, RES_F64 = 0, 1
COMM_ID_BYTES = 128

# every symbol include/aar.h declares (tests/test_capi_symbols.py checks the header against this list and the .so)
SYMBOLS = [
    "aar_last_error", "aar_dataset_free", "aar_dataset_full_len", "aar_synth_default", "aar_synth_generate",
    "aar_solution_read", "aar_solution_write", "aar_solution_write_yaml", "aar_detections_write",
    "aar_rodrigues_vec2mat", "aar_rodrigues_mat2vec", "aar_plan_shards", "aar_comm_make_id", "aar_comm_create",
    "aar_comm_destroy", "aar_problem_desc_from_dataset", "aar_problem_create", "aar_problem_destroy",
    "aar_problem_full_len", "aar_problem_num_vars", "aar_problem_local_obs", "aar_eval_residuals",
    "aar_eval_normal_equations", "aar_eval_damped_step", "aar_lm_default_params", "aar_lm_init", "aar_lm_step",
    "aar_lm_get_solution", "aar_lm_solve", "aar_get_stage_times", "aar_reproj_stats", "aar_device_count",
    "aar_device_synchronize", "aar_set_kernel_profiling", "aar_get_kernel_times", "aar_kernel_name",
    "aar_problem_set_huber_delta", "aar_problem_get_huber_delta", "aar_track", "aar_cam_config_read",
    "aar_undistort_points", "aar_local_group_create", "aar_local_group_destroy", "aar_comm_create_local",
    "aar_cam_configs_read", "aar_detections_read", "aar_detections_free", "aar_subseqs_read", "aar_ippe_square",
    "aar_vote_transforms", "aar_init_default_params", "aar_initializer_run", "aar_initializer_object_poses",
    "aar_comm_get_stats", "aar_lm_set_step_callback", "aar_lm_set_stop_function", "aar_problem_extract_z", "aar_problem_merge_z",
    "aar_solution_read_ex", "aar_cam_configs_read_ex", "aar_set_stage_timers", "aar_problem_pcg_iterations",
    "aar_solver_default_options", "aar_problem_create_ex", "aar_problem_get_solver_stats", "aar_problem_set_test_hook",
    "aar_problem_covariance", "aar_covariance_write_yaml",
    "aar_predict_query_validate", "aar_problem_predict_corners", "aar_problem_detection_leverage", "aar_leverage_write_yaml",
    "aar_problem_detection_loo", "aar_problem_gate_detections", "aar_loo_write_yaml",
    "aar_problem_residual_report", "aar_dataset_select_observations", "aar_residual_report_write_yaml",
    "aar_problem_constraints_validate", "aar_problem_create_constrained", "aar_problem_num_priors", "aar_problem_eval_priors",
    "aar_problem_num_pair_priors", "aar_problem_eval_pair_priors", "aar_relative_pose",
    "aar_smooth_params_validate", "aar_track_smooth", "aar_track_smooth_system", "aar_track_smooth_system2", "aar_smooth_solve_launches", "aar_track_smooth_covariance", "aar_track_smooth_covariance2",
    "aar_smooth_fit_default_params", "aar_smooth_fit_params_validate", "aar_track_smooth_fit", "aar_track_smooth_fit_terms", "aar_track_smooth_fit2", "aar_track_smooth_fit_terms2",
    "aar_smooth_query_validate", "aar_track_smooth_query", "aar_track_smooth_query2", "aar_track_smooth_query2_step", "aar_track_smooth_lag3",
    "aar_smooth_relative_validate", "aar_track_smooth_relative",
    "aar_track_smooth_detection_leverage", "aar_track_smooth_detection_loo", "aar_track_smooth_predict_corners",
    "aar_track_smooth_gate_detections", "aar_smooth_loo_write_yaml",
    "aar_tracker_default_params", "aar_tracker_params_validate", "aar_tracker_create", "aar_tracker_push", "aar_tracker_window",
    "aar_tracker_reset", "aar_tracker_destroy",
    "aar_tracker_default_detection_params", "aar_tracker_detection_params_validate", "aar_tracker_enable_detections",
    "aar_tracker_push_detections", "aar_tracker_uncertainty", "aar_tracker_covariance_write_yaml",
    "aar_tracker_bank_params_validate", "aar_tracker_bank_create", "aar_tracker_bank_size", "aar_tracker_bank_push",
    "aar_tracker_bank_enable_detections", "aar_tracker_bank_push_detections", "aar_tracker_bank_window", "aar_tracker_bank_uncertainty",
    "aar_tracker_bank_reset", "aar_tracker_bank_get_stats", "aar_tracker_bank_destroy",
    "aar_tracker_default_gate_params", "aar_tracker_gate_params_validate", "aar_tracker_enable_gate", "aar_tracker_last_gate",
    "aar_tracker_gate_detail", "aar_tracker_gate_bank_enable", "aar_tracker_gate_bank_last", "aar_tracker_gate_bank_detail",
    "aar_tracker_default_motion_params", "aar_tracker_motion_params_validate", "aar_tracker_enable_motion", "aar_tracker_last_motion",
    "aar_tracker_predict", "aar_tracker_motion_bank_enable", "aar_tracker_motion_bank_last", "aar_tracker_motion_bank_predict",
]
TRACKER_BANK_MAX_MEMBERS = 1024
TRACKER_MAX_LAG = 15
TRACKER_START_VOTE, TRACKER_START_BEST = 1, 2
TRACKER_ANCHOR_FIXED, TRACKER_ANCHOR_MARGINAL = 0, 1
TRACKER_ANCHORS = {"fixed": TRACKER_ANCHOR_FIXED, "marginal": TRACKER_ANCHOR_MARGINAL}
TRACKER_STARTS = {"vote": TRACKER_START_VOTE, "best": TRACKER_START_BEST}
NUM_KERNELS = 18
PRIOR_CAMERA, PRIOR_MARKER = 0, 1
PREDICT_BEHIND, PREDICT_UNDEFINED = 1, 2
PREDICT_UNDETERMINED = 4
PRIOR_KINDS = {"camera": PRIOR_CAMERA, "marker": PRIOR_MARKER}
SOLVER_DIRECT, SOLVER_PCG, SOLVER_SPCG, SOLVER_AUTO = 0, 1, 2, 3
TEST_HOOK_SPCG_DROP = 1
ENV_SOLVER, ENV_DETERMINISTIC, ENV_PCG_ETA, ENV_PCG_MAX_IT = 1, 2, 4, 8
SOLVERS = {"direct": SOLVER_DIRECT, "pcg": SOLVER_PCG, "spcg": SOLVER_SPCG, "auto": SOLVER_AUTO}
SOLVER_NAMES = {v: k for k, v in SOLVERS.items()}


class AarError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("aar error %d: %s" % (code, msg))
        self.code = code


class CDataset(C.Structure):
    _fields_ = [
        ("num_cams", C.c_int32), ("num_markers", C.c_int32), ("num_frames", C.c_int32),
        ("root_cam", C.c_int32), ("root_marker", C.c_int32),
        ("cam_ids", C.POINTER(C.c_int32)), ("marker_ids", C.POINTER(C.c_int32)), ("frame_ids", C.POINTER(C.c_int32)),
        ("image_sizes", C.POINTER(C.c_int32)), ("cam_mats", C.POINTER(C.c_double)), ("dist_coeffs", C.POINTER(C.c_double)),
        ("marker_size", C.c_double), ("num_obs", C.c_int64),
        ("obs_frame", C.POINTER(C.c_int32)), ("obs_cam", C.POINTER(C.c_int32)), ("obs_marker", C.POINTER(C.c_int32)),
        ("obs_uv", C.POINTER(C.c_float)), ("x_full", C.POINTER(C.c_double)), ("x_truth", C.POINTER(C.c_double)),
        ("optimize_cam_poses", C.c_int32), ("optimize_marker_poses", C.c_int32),
        ("optimize_object_poses", C.c_int32), ("optimize_cam_intrinsics", C.c_int32),
    ]


class CSynthDesc(C.Structure):
    _fields_ = [
        ("num_cams", C.c_int32), ("num_markers", C.c_int32), ("num_frames", C.c_int32), ("seed", C.c_uint64),
        ("marker_size", C.c_double), ("noise_px", C.c_double), ("init_rot_sigma", C.c_double),
        ("init_trans_sigma", C.c_double), ("init_scale", C.c_double), ("cam_arc_deg", C.c_double),
        ("min_view_cos", C.c_double),
    ]


class CProblemDesc(C.Structure):
    _fields_ = [
        ("num_cams", C.c_int32), ("num_markers", C.c_int32), ("num_frames", C.c_int32),
        ("root_cam", C.c_int32), ("root_marker", C.c_int32),
        ("cam_mats", C.POINTER(C.c_double)), ("marker_size", C.c_double), ("num_obs", C.c_int64),
        ("obs_frame", C.POINTER(C.c_int32)), ("obs_cam", C.POINTER(C.c_int32)), ("obs_marker", C.POINTER(C.c_int32)),
        ("obs_uv", C.POINTER(C.c_float)),
        ("optimize_cam_poses", C.c_int32), ("optimize_marker_poses", C.c_int32), ("optimize_object_poses", C.c_int32),
        ("optimize_cam_intrinsics", C.c_int32),
        ("residual_mode", C.c_int32), ("with_huber", C.c_int32), ("device_id", C.c_int32), ("comm", C.c_void_p),
    ]


class CSolverOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("solver", C.c_int32), ("deterministic", C.c_int32), ("pcg_max_it", C.c_int32),
                ("pcg_eta", C.c_double), ("pcg_eta_loose", C.c_double), ("pcg_eta_switch", C.c_double), ("pcg_abs_tol", C.c_double)]


class CSolverStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("solver", C.c_int32), ("deterministic", C.c_int32), ("last_iterations", C.c_int32),
                ("total_iterations", C.c_int64), ("solves", C.c_int64), ("fallbacks", C.c_int64), ("pcg_eta", C.c_double),
                ("pcg_max_it", C.c_int32), ("env_overrides", C.c_int32), ("same_xcd_solves", C.c_int64), ("pcg_eta_loose", C.c_double),
                ("pcg_eta_switch", C.c_double), ("pcg_abs_tol", C.c_double)]


class CCovarianceReport(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_residuals", C.c_int64), ("num_vars", C.c_int64), ("sum_sq", C.c_double),
                ("sigma2", C.c_double), ("min_pivot", C.c_double), ("max_pivot", C.c_double), ("frames_written", C.c_int32)]


class CPredictReport(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_residuals", C.c_int64), ("num_vars", C.c_int64), ("sum_sq", C.c_double),
                ("sigma2", C.c_double), ("num_live_vars", C.c_int64), ("leverage_sum", C.c_double), ("undefined", C.c_int64),
                ("behind", C.c_int64), ("launches", C.c_int32), ("seconds", C.c_double)]


class CLooRule(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("f_max", C.c_double)]


class CLooReport(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("predict", CPredictReport), ("dof", C.c_int64), ("undetermined", C.c_int64),
                ("rejected", C.c_int64), ("f_max", C.c_double), ("max_f", C.c_double), ("argmax_f", C.c_int64)]


class COutlierRule(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("k_median", C.c_double), ("min_px", C.c_double)]


class CResidualReport(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_detections", C.c_int64), ("num_rejected", C.c_int64), ("num_nonfinite", C.c_int64),
                ("sum_sq", C.c_double), ("rmse", C.c_double), ("median", C.c_double), ("max", C.c_double), ("threshold", C.c_double),
                ("cams_emptied", C.c_int32), ("markers_emptied", C.c_int32), ("frames_emptied", C.c_int32)]


class CPosePrior(C.Structure):
    _fields_ = [("kind", C.c_int32), ("index", C.c_int32), ("x6", C.c_double * 6), ("info", C.c_double * 36)]


class CConstraints(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_fixed_cams", C.c_int32), ("fixed_cams", C.POINTER(C.c_int32)),
                ("n_fixed_markers", C.c_int32), ("fixed_markers", C.POINTER(C.c_int32)),
                ("n_priors", C.c_int32), ("priors", C.POINTER(CPosePrior))]


class CPairPrior(C.Structure):
    _fields_ = [("kind", C.c_int32), ("index_a", C.c_int32), ("index_b", C.c_int32), ("x6_rel", C.c_double * 6), ("info", C.c_double * 36)]


class CConstraintsV2(C.Structure):
    """aar_problem_constraints with the fields appended for the pair priors (CConstraints is the struct as it was before them: the
    library takes either, by struct_size)"""
    _fields_ = CConstraints._fields_ + [("n_pair_priors", C.c_int32), ("pair_priors", C.POINTER(CPairPrior))]


class Constraints:
    """aar_problem_constraints built from Python values (kept alive with the struct).  fixed_cams / fixed_markers: indices; priors: a list of
    (kind, index, x6, info) with kind "camera" | "marker" (or PRIOR_CAMERA / PRIOR_MARKER), x6 the 6-vector (rvec, t), info the 6x6 information matrix;
    pair_priors: a list of (kind, index_a, index_b, x6_rel, info), x6_rel the (rvec, t) of T_a^-1 T_b (relative_pose)."""

    def __init__(self, fixed_cams=None, fixed_markers=None, priors=None, pair_priors=None):
        self._fc = np.ascontiguousarray(list(fixed_cams or []), dtype=np.int32)
        self._fm = np.ascontiguousarray(list(fixed_markers or []), dtype=np.int32)
        pr = list(priors or [])
        self._pr = (CPosePrior * max(len(pr), 1))()
        for i, (kind, index, x6, info) in enumerate(pr):
            q = self._pr[i]
            q.kind = PRIOR_KINDS[kind] if isinstance(kind, str) else int(kind)
            q.index = int(index)
            x6 = np.asarray(x6, dtype=np.float64).reshape(6)
            info = np.asarray(info, dtype=np.float64).reshape(36)
            for k in range(6):
                q.x6[k] = float(x6[k])
            for k in range(36):
                q.info[k] = float(info[k])
        pp = list(pair_priors or [])
        self._pp = (CPairPrior * max(len(pp), 1))()
        for i, (kind, ia, ib, x6, info) in enumerate(pp):
            q = self._pp[i]
            q.kind = PRIOR_KINDS[kind] if isinstance(kind, str) else int(kind)
            q.index_a, q.index_b = int(ia), int(ib)
            x6 = np.asarray(x6, dtype=np.float64).reshape(6)
            info = np.asarray(info, dtype=np.float64).reshape(36)
            for k in range(6):
                q.x6_rel[k] = float(x6[k])
            for k in range(36):
                q.info[k] = float(info[k])
        c = CConstraintsV2()
        c.struct_size = C.sizeof(CConstraintsV2)
        c.n_pair_priors = len(pp)
        c.pair_priors = C.cast(self._pp, C.POINTER(CPairPrior)) if pp else None
        self.n_pair_priors = len(pp)
        c.n_fixed_cams = len(self._fc)
        c.fixed_cams = self._fc.ctypes.data_as(C.POINTER(C.c_int32)) if len(self._fc) else None
        c.n_fixed_markers = len(self._fm)
        c.fixed_markers = self._fm.ctypes.data_as(C.POINTER(C.c_int32)) if len(self._fm) else None
        c.n_priors = len(pr)
        c.priors = C.cast(self._pr, C.POINTER(CPosePrior)) if pr else None
        self.c = c
        self.n_priors = len(pr)

    def empty(self):
        return self.c.n_fixed_cams == 0 and self.c.n_fixed_markers == 0 and self.c.n_priors == 0 and self.c.n_pair_priors == 0


def constraints_validate(ds, fixed_cams=None, fixed_markers=None, priors=None, optimize=None, struct_size=None, pair_priors=None):
    """aar_problem_constraints_validate (host code): raises AarError(AAR_ERR_INVALID) with the library's message.  struct_size overrides
    the struct's own size (versioning tests)."""
    cds = ds.as_c()
    d = CProblemDesc()
    lib().aar_problem_desc_from_dataset(C.byref(cds), C.byref(d))
    if optimize is not None:
        d.optimize_cam_poses, d.optimize_marker_poses, d.optimize_object_poses = [int(b) for b in optimize]
    k = Constraints(fixed_cams, fixed_markers, priors, pair_priors)
    if struct_size is not None:
        k.c.struct_size = int(struct_size)
    _check(lib().aar_problem_constraints_validate(C.byref(d), C.byref(k.c)))


class CLmParams(C.Structure):
    _fields_ = [
        ("max_iters", C.c_int32), ("min_error", C.c_double), ("min_step_error_diff", C.c_double),
        ("min_average_step_error_diff", C.c_double), ("tau", C.c_double), ("verbose", C.c_int32),
    ]


class CSmoothParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sigma_rot", C.c_double), ("sigma_trans", C.c_double),
                ("frame_time", C.POINTER(C.c_double)), ("rel_motion", C.POINTER(C.c_double))]


class CSmoothParamsV2(C.Structure):
    """aar_smooth_params with the motion model (CSmoothParams stays the struct as it was before the model: a caller built against it)"""
    _fields_ = CSmoothParams._fields_ + [("model", C.c_int32), ("sigma_rot0", C.c_double), ("sigma_trans0", C.c_double)]


SMOOTH_MODEL_RANDOM_WALK, SMOOTH_MODEL_CONSTANT_VELOCITY = 0, 1
_SMOOTH_MODELS = {"rw": 0, "random_walk": 0, "cv": 1, "constant_velocity": 1}


class CSmoothReport(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_int32), ("stop_code", C.c_int32), ("rejected_tries", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_data_cost", C.c_double),
                ("final_prior_cost", C.c_double), ("final_mu", C.c_double), ("seconds", C.c_double)]


class CSmoothCovarianceReport(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_residuals", C.c_int64), ("num_vars", C.c_int64), ("data_cost", C.c_double),
                ("prior_cost", C.c_double), ("sigma2", C.c_double), ("launches", C.c_int32), ("seconds", C.c_double)]


class CSmoothQueryReport(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_residuals", C.c_int64), ("num_vars", C.c_int64), ("data_cost", C.c_double),
                ("prior_cost", C.c_double), ("sigma2", C.c_double), ("num_queries", C.c_int32), ("num_inside", C.c_int32),
                ("num_on_frame", C.c_int32), ("num_outside", C.c_int32), ("launches", C.c_int32), ("seconds", C.c_double)]


class CSmoothRelativeReport(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_residuals", C.c_int64), ("num_vars", C.c_int64), ("data_cost", C.c_double),
                ("prior_cost", C.c_double), ("sigma2", C.c_double), ("num_pairs", C.c_int32), ("num_direct", C.c_int32),
                ("num_chained", C.c_int32), ("max_lag", C.c_int32), ("launches", C.c_int32), ("seconds", C.c_double)]


class CSmoothPredictReport(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_residuals", C.c_int64), ("num_vars", C.c_int64), ("data_cost", C.c_double),
                ("prior_cost", C.c_double), ("sigma2", C.c_double), ("num_queries", C.c_int64), ("behind", C.c_int64),
                ("leverage_sum", C.c_double), ("num_inside", C.c_int32), ("num_on_frame", C.c_int32), ("num_outside", C.c_int32),
                ("launches", C.c_int32), ("seconds", C.c_double), ("kernel_seconds", C.c_double)]


class CSmoothLooReport(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_residuals", C.c_int64), ("num_vars", C.c_int64), ("data_cost", C.c_double),
                ("prior_cost", C.c_double), ("sigma2", C.c_double), ("dof", C.c_int64), ("behind", C.c_int64), ("undetermined", C.c_int64),
                ("rejected", C.c_int64), ("f_max", C.c_double), ("max_f", C.c_double), ("argmax_f", C.c_int64), ("leverage_sum", C.c_double),
                ("launches", C.c_int32), ("seconds", C.c_double), ("kernel_seconds", C.c_double)]


class SmoothParams:
    """aar_smooth_params built from Python values (the arrays are kept alive with the struct)"""

    def __init__(self, sigma_rot, sigma_trans, frame_time=None, rel_motion=None, struct_size=None, model=None, sigma_rot0=0.0, sigma_trans0=0.0):
        """model: None = the struct without the model fields (40 bytes: the random walk); "rw" / "cv" or an AAR_SMOOTH_MODEL_* value = the
        struct with them, sigma_rot0 / sigma_trans0 being pair 0's sigmas under "cv" """
        self._ft = None if frame_time is None else np.ascontiguousarray(frame_time, dtype=np.float64).reshape(-1)
        self._rm = None if rel_motion is None else np.ascontiguousarray(rel_motion, dtype=np.float64).reshape(-1)
        if model is None:
            c = CSmoothParams()
        else:
            c = CSmoothParamsV2()
            c.model = _SMOOTH_MODELS[model] if isinstance(model, str) else int(model)
            c.sigma_rot0, c.sigma_trans0 = float(sigma_rot0), float(sigma_trans0)
        c.struct_size = C.sizeof(c) if struct_size is None else int(struct_size)
        c.sigma_rot, c.sigma_trans = float(sigma_rot), float(sigma_trans)
        c.frame_time = None if self._ft is None else self._ft.ctypes.data_as(C.POINTER(C.c_double))
        c.rel_motion = None if self._rm is None else self._rm.ctypes.data_as(C.POINTER(C.c_double))
        self.c = c

    def check_lengths(self, num_frames):
        assert self._ft is None or len(self._ft) == num_frames
        assert self._rm is None or len(self._rm) == 6 * max(num_frames - 1, 0)


def smooth_params_validate(num_frames, sigma_rot, sigma_trans, frame_time=None, rel_motion=None, struct_size=None, **model):
    """aar_smooth_params_validate (host code): raises AarError(AAR_ERR_INVALID) with the library's message.  struct_size overrides the
    struct's own size (versioning tests)."""
    sp = SmoothParams(sigma_rot, sigma_trans, frame_time, rel_motion, struct_size, **model)
    sp.check_lengths(num_frames)
    _check(lib().aar_smooth_params_validate(int(num_frames), C.byref(sp.c)))


def smooth_solve_launches(num_frames, model="rw"):
    """aar_smooth_solve_launches (host code): kernel launches of one damped solve of the smoother at this size"""
    return int(lib().aar_smooth_solve_launches(int(num_frames), _SMOOTH_MODELS[model] if isinstance(model, str) else int(model)))


def smooth_query_validate(num_frames, sigma_rot, sigma_trans, query_time, frame_time=None, rel_motion=None, struct_size=None, **model):
    """aar_smooth_query_validate (host code): raises AarError(AAR_ERR_INVALID) with the library's message"""
    sp = SmoothParams(sigma_rot, sigma_trans, frame_time, rel_motion, struct_size, **model)
    sp.check_lengths(num_frames)
    qt = np.ascontiguousarray(query_time, dtype=np.float64).reshape(-1)
    _check(lib().aar_smooth_query_validate(int(num_frames), C.byref(sp.c), len(qt), _dptr(qt) if len(qt) else None))


def _pairs(pairs):
    """pairs [Q, 2] (or empty) as two contiguous int32 arrays"""
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    assert pr.size == 0 or (np.abs(pr).max() < 2 ** 31)
    return np.ascontiguousarray(pr[:, 0], dtype=np.int32), np.ascontiguousarray(pr[:, 1], dtype=np.int32)


def smooth_relative_validate(num_frames, sigma_rot, sigma_trans, pairs, frame_time=None, rel_motion=None, struct_size=None, **model):
    """aar_smooth_relative_validate (host code): raises AarError(AAR_ERR_INVALID) with the library's message.  pairs [Q, 2] = (a, b)"""
    sp = SmoothParams(sigma_rot, sigma_trans, frame_time, rel_motion, struct_size, **model)
    sp.check_lengths(num_frames)
    fa, fb = _pairs(pairs)
    ip = C.POINTER(C.c_int32)
    _check(lib().aar_smooth_relative_validate(int(num_frames), C.byref(sp.c), len(fa), fa.ctypes.data_as(ip) if len(fa) else None,
                                              fb.ctypes.data_as(ip) if len(fb) else None))


class CSmoothFitParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_iters", C.c_int32), ("rel_tol", C.c_double), ("estimate_px", C.c_int32),
                ("estimate_rot", C.c_int32), ("estimate_trans", C.c_int32)]


class CSmoothFitReport(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_int32), ("stop_code", C.c_int32), ("sigma_px", C.c_double),
                ("sigma_rot", C.c_double), ("sigma_trans", C.c_double), ("sigma_rot_eff", C.c_double), ("sigma_trans_eff", C.c_double),
                ("last_rel_change", C.c_double), ("lm_steps", C.c_int32), ("launches", C.c_int32), ("seconds", C.c_double),
                ("a_rot", C.c_double), ("u_rot", C.c_double), ("a_trans", C.c_double), ("u_trans", C.c_double), ("u_data", C.c_double),
                ("data_cost", C.c_double)]


def smooth_fit_params(struct_size=None, **over):
    """aar_smooth_fit_default_params with the given fields replaced (max_iters, rel_tol, estimate_px, estimate_rot, estimate_trans);
    struct_size overrides the struct's own size (versioning tests)"""
    p = CSmoothFitParams()
    lib().aar_smooth_fit_default_params(C.byref(p))
    for k, v in over.items():
        if k not in ("max_iters", "rel_tol", "estimate_px", "estimate_rot", "estimate_trans"):
            raise TypeError("aar_smooth_fit_params has no field %r" % k)
        setattr(p, k, float(v) if k == "rel_tol" else int(v))
    if struct_size is not None:
        p.struct_size = int(struct_size)
    return p


def smooth_fit_params_validate(struct_size=None, **over):
    """aar_smooth_fit_params_validate (host code): raises AarError(AAR_ERR_INVALID) with the library's message"""
    p = smooth_fit_params(struct_size, **over)
    _check(lib().aar_smooth_fit_params_validate(C.byref(p)))


class CTrackerParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("lag", C.c_int32), ("smooth", C.c_int32), ("sigma_rot", C.c_double), ("sigma_trans", C.c_double),
                ("with_huber", C.c_int32), ("huber_delta", C.c_float), ("max_obs_per_frame", C.c_int32), ("device_id", C.c_int32),
                ("anchor_mode", C.c_int32), ("covariance", C.c_int32)]


class CTrackerUncertainty(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("cov_valid", C.c_int32), ("sigma2", C.c_double), ("window_frames", C.c_int32),
                ("has_marginal", C.c_int32), ("frame_index", C.c_int64 * 16), ("cov", C.c_double * (16 * 36)), ("marginal_index", C.c_int64),
                ("marginal_info", C.c_double * 36), ("marginal_mean", C.c_double * 6), ("marginal_dropped", C.c_int64)]


class CTrackerGateParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("k_median", C.c_double), ("min_px", C.c_double), ("min_detections", C.c_int32)]


class CTrackerGateInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("gated", C.c_int32), ("n_in", C.c_int32), ("n_kept", C.c_int32), ("n_nonfinite", C.c_int32),
                ("median", C.c_double), ("max", C.c_double), ("threshold", C.c_double)]


class CTrackerMotionParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("model", C.c_int32), ("max_dt", C.c_double)]


class CTrackerMotionInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("model", C.c_int32), ("predicted", C.c_int32), ("rel", C.c_double * 6),
                ("velocity", C.c_double * 6), ("newest_time", C.c_double)]


class CTrackerBankStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("members", C.c_int32), ("pushes", C.c_int64), ("launches", C.c_int64), ("h2d_copies", C.c_int64),
                ("h2d_bytes", C.c_int64), ("d2h_copies", C.c_int64), ("d2h_bytes", C.c_int64)]


class CTrackerResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("frame_index", C.c_int64), ("window_frames", C.c_int32), ("iterations", C.c_int32),
                ("stop_code", C.c_int32), ("rejected_tries", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("final_data_cost", C.c_double), ("final_prior_cost", C.c_double), ("final_mu", C.c_double), ("pose", C.c_double * 6),
                ("has_lagged", C.c_int32), ("lagged_index", C.c_int64), ("lagged_pose", C.c_double * 6), ("seconds", C.c_double)]


def tracker_params(lag=0, smooth=False, sigma_rot=0.0, sigma_trans=0.0, with_huber=False, huber_delta=None, max_obs_per_frame=None, device=0,
                   struct_size=None, anchor="fixed", covariance=False):
    """aar_tracker_params from Python values (None = the library's default); anchor: "fixed" | "marginal" (or the integer)"""
    p = CTrackerParams()
    lib().aar_tracker_default_params(C.byref(p))
    p.lag, p.smooth, p.sigma_rot, p.sigma_trans = int(lag), int(smooth), float(sigma_rot), float(sigma_trans)
    p.with_huber, p.device_id = int(bool(with_huber)), int(device)
    p.anchor_mode, p.covariance = int(TRACKER_ANCHORS.get(anchor, anchor)), int(covariance)
    if huber_delta is not None:
        p.huber_delta = float(huber_delta)
    if max_obs_per_frame is not None:
        p.max_obs_per_frame = int(max_obs_per_frame)
    if struct_size is not None:
        p.struct_size = int(struct_size)
    return p


class CTrackerStartInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("voted", C.c_int32), ("candidates", C.c_int32), ("winner", C.c_int32), ("vote_cost", C.c_double),
                ("start_source", C.c_int32), ("cost_prediction", C.c_double), ("cost_vote", C.c_double), ("start_pose", C.c_double * 6)]


def tracker_params_validate(ds, **kw):
    """aar_tracker_params_validate (host code): raises AarError(AAR_ERR_INVALID) with the library's message"""
    c = ds.as_c()
    p = tracker_params(**kw)
    _check(lib().aar_tracker_params_validate(C.byref(c), C.byref(p)))


class CLmIter(C.Structure):
    _fields_ = [("err", C.c_double), ("mu", C.c_double), ("gain", C.c_double), ("delta_norm", C.c_double),
                ("accepted", C.c_int32), ("tries", C.c_int32)]


class CLmReport(C.Structure):
    _fields_ = [
        ("iterations", C.c_int32), ("stop_code", C.c_int32), ("initial_err", C.c_double), ("final_err", C.c_double),
        ("final_mu", C.c_double), ("solve_seconds", C.c_double), ("trial_points", C.c_int64),
        ("trace", C.POINTER(CLmIter)), ("trace_cap", C.c_int32),
    ]


class CCommStats(C.Structure):
    _fields_ = [("world_size", C.c_int32), ("rank", C.c_int32), ("ranks_seen", C.c_int32), ("allreduce_calls", C.c_int64),
                ("allreduce_bytes", C.c_int64), ("system_allreduce_bytes", C.c_int64)]


class CStageTimes(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("unpack", "jacobian_normal_eq", "schur", "chol", "backsub", "residual",
                                          "control", "allreduce", "total")] + [("launches", C.c_int64)]


_lib = None
STEP_CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.c_int64)
STOP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)


class CCamModel(C.Structure):
    _fields_ = [("K", C.c_double * 9), ("dist", C.c_double * 12), ("n_dist", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32)]


class CTrackerDetectionParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("cams", C.POINTER(CCamModel)), ("ippe_threshold", C.c_double), ("min_detections", C.c_int32),
                ("start_policy", C.c_int32)]


class CDetections(C.Structure):
    _fields_ = [("num_cams", C.c_int32), ("num_frames", C.c_int32), ("num_det", C.c_int64),
                ("det_frame", C.POINTER(C.c_int32)), ("det_cam", C.POINTER(C.c_int32)), ("det_id", C.POINTER(C.c_int32)),
                ("det_uv", C.POINTER(C.c_float))]


class CInitParams(C.Structure):
    _fields_ = [("marker_size", C.c_double), ("threshold", C.c_double), ("min_detections", C.c_int32),
                ("n_excluded", C.c_int32), ("excluded_cams", C.POINTER(C.c_int32)), ("device_id", C.c_int32)]


def lib():
    """Load libaar.so (built by __graft_entry__.build() / `make -C automatic-ar_amd`).  Fails loudly when missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libaar.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    L.aar_last_error.restype = C.c_char_p
    L.aar_dataset_full_len.restype = C.c_int64
    L.aar_dataset_full_len.argtypes = [C.POINTER(CDataset)]
    L.aar_dataset_free.argtypes = [C.POINTER(CDataset)]
    L.aar_dataset_free.restype = None
    L.aar_synth_default.argtypes = [C.POINTER(CSynthDesc), C.c_int32]
    L.aar_synth_default.restype = None
    L.aar_synth_generate.argtypes = [C.POINTER(CSynthDesc), C.POINTER(C.POINTER(CDataset))]
    L.aar_solution_read.argtypes = [C.c_char_p, C.POINTER(C.POINTER(CDataset))]
    L.aar_solution_read_ex.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.POINTER(CDataset))]
    for n in ("aar_solution_write", "aar_solution_write_yaml", "aar_detections_write"):
        getattr(L, n).argtypes = [C.c_char_p, C.POINTER(CDataset)]
    L.aar_rodrigues_vec2mat.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.aar_rodrigues_vec2mat.restype = None
    L.aar_rodrigues_mat2vec.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.aar_rodrigues_mat2vec.restype = None
    L.aar_plan_shards.argtypes = [C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int32)]
    L.aar_comm_make_id.argtypes = [C.c_char_p]
    L.aar_comm_create.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.aar_comm_destroy.argtypes = [C.c_void_p]
    L.aar_comm_get_stats.argtypes = [C.c_void_p, C.POINTER(CCommStats)]
    L.aar_comm_destroy.restype = None
    L.aar_problem_desc_from_dataset.argtypes = [C.POINTER(CDataset), C.POINTER(CProblemDesc)]
    L.aar_problem_desc_from_dataset.restype = None
    L.aar_problem_create.argtypes = [C.POINTER(CProblemDesc), C.POINTER(C.c_void_p)]
    L.aar_problem_create_ex.argtypes = [C.POINTER(CProblemDesc), C.POINTER(CSolverOptions), C.POINTER(C.c_void_p)]
    # (the constraints are size-versioned: CConstraints or CConstraintsV2, by struct_size)
    L.aar_problem_constraints_validate.argtypes = [C.POINTER(CProblemDesc), C.c_void_p]
    L.aar_problem_create_constrained.argtypes = [C.POINTER(CProblemDesc), C.POINTER(CSolverOptions), C.c_void_p, C.POINTER(C.c_void_p)]
    L.aar_problem_num_priors.argtypes = [C.c_void_p]
    L.aar_problem_num_priors.restype = C.c_int32
    L.aar_problem_eval_priors.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.aar_problem_num_pair_priors.argtypes = [C.c_void_p]
    L.aar_problem_num_pair_priors.restype = C.c_int32
    L.aar_problem_eval_pair_priors.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.aar_relative_pose.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.aar_solver_default_options.argtypes = [C.POINTER(CSolverOptions)]
    L.aar_solver_default_options.restype = None
    L.aar_problem_get_solver_stats.argtypes = [C.c_void_p, C.POINTER(CSolverStats)]
    L.aar_problem_set_test_hook.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.aar_problem_destroy.argtypes = [C.c_void_p]
    L.aar_problem_destroy.restype = None
    for n in ("aar_problem_full_len", "aar_problem_num_vars", "aar_problem_local_obs"):
        getattr(L, n).argtypes = [C.c_void_p]
        getattr(L, n).restype = C.c_int64
    dp = C.POINTER(C.c_double)
    L.aar_eval_residuals.argtypes = [C.c_void_p, dp, dp, dp]
    L.aar_eval_normal_equations.argtypes = [C.c_void_p, dp, dp, dp, dp]
    L.aar_eval_damped_step.argtypes = [C.c_void_p, dp, C.c_double, dp]
    L.aar_problem_covariance.argtypes = [C.c_void_p, dp, dp, dp, dp, C.POINTER(CCovarianceReport)]
    L.aar_covariance_write_yaml.argtypes = [C.c_char_p, C.POINTER(CDataset), dp, dp, C.c_double]
    u8p = C.POINTER(C.c_uint8)
    ip32 = C.POINTER(C.c_int32)
    L.aar_predict_query_validate.argtypes = [C.POINTER(CProblemDesc), C.c_int64, ip32, ip32, ip32]
    L.aar_problem_predict_corners.argtypes = [C.c_void_p, dp, C.c_int64, ip32, ip32, ip32, dp, dp, u8p, C.POINTER(CPredictReport)]
    L.aar_problem_detection_leverage.argtypes = [C.c_void_p, dp, dp, dp, C.POINTER(CPredictReport)]
    L.aar_problem_detection_loo.argtypes = [C.c_void_p, dp, C.POINTER(CLooRule), dp, dp, dp, dp, dp, dp, u8p, u8p, C.POINTER(CLooReport)]
    L.aar_problem_gate_detections.argtypes = [C.c_void_p, dp, C.c_int64, ip32, ip32, ip32, C.POINTER(C.c_float), dp, dp, u8p,
                                              C.POINTER(CPredictReport)]
    L.aar_loo_write_yaml.argtypes = [C.c_char_p, C.POINTER(CDataset), dp, dp, dp, dp, u8p, u8p, C.POINTER(CLooReport)]
    L.aar_leverage_write_yaml.argtypes = [C.c_char_p, C.POINTER(CDataset), dp, dp, C.c_double, C.POINTER(CPredictReport)]
    L.aar_problem_residual_report.argtypes = [C.c_void_p, dp, C.POINTER(COutlierRule), dp, u8p, dp, dp, dp, C.POINTER(CResidualReport)]
    L.aar_dataset_select_observations.argtypes = [C.POINTER(CDataset), u8p, C.POINTER(C.POINTER(CDataset))]
    L.aar_residual_report_write_yaml.argtypes = [C.c_char_p, C.POINTER(CDataset), dp, dp, dp, u8p, C.POINTER(CResidualReport)]
    L.aar_lm_default_params.argtypes = [C.POINTER(CLmParams)]
    L.aar_lm_default_params.restype = None
    L.aar_lm_init.argtypes = [C.c_void_p, dp, C.POINTER(CLmParams)]
    L.aar_lm_step.argtypes = [C.c_void_p, C.POINTER(CLmIter)]
    L.aar_lm_get_solution.argtypes = [C.c_void_p, dp, dp]
    L.aar_lm_solve.argtypes = [C.c_void_p, dp, C.POINTER(CLmParams), C.POINTER(CLmReport)]
    L.aar_get_stage_times.argtypes = [C.c_void_p, C.POINTER(CStageTimes)]
    L.aar_set_stage_timers.argtypes = [C.c_void_p, C.c_int]
    L.aar_problem_pcg_iterations.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.aar_reproj_stats.argtypes = [C.c_void_p, dp, dp, dp]
    L.aar_set_kernel_profiling.argtypes = [C.c_void_p, C.c_int]
    L.aar_get_kernel_times.argtypes = [C.c_void_p, dp, C.POINTER(C.c_int64)]
    L.aar_kernel_name.argtypes = [C.c_int]
    L.aar_kernel_name.restype = C.c_char_p
    L.aar_track.argtypes = [C.c_void_p, dp, C.POINTER(CLmParams), C.POINTER(C.c_int32), dp]
    L.aar_smooth_params_validate.argtypes = [C.c_int32, C.c_void_p]
    L.aar_track_smooth.argtypes = [C.c_void_p, dp, C.POINTER(CLmParams), C.c_void_p, dp, dp, C.POINTER(CSmoothReport)]
    L.aar_track_smooth_system.argtypes = [C.c_void_p, dp, C.c_void_p, C.c_double, dp, dp, dp, dp, dp]
    L.aar_smooth_solve_launches.argtypes = [C.c_int32, C.c_int32]
    L.aar_smooth_solve_launches.restype = C.c_int32
    L.aar_track_smooth_system2.argtypes = [C.c_void_p, dp, C.c_void_p, C.c_double, dp, dp, dp, dp, dp, dp]
    L.aar_track_smooth_covariance.argtypes = [C.c_void_p, dp, C.c_void_p, dp, dp, C.POINTER(CSmoothCovarianceReport)]
    L.aar_track_smooth_covariance2.argtypes = [C.c_void_p, dp, C.c_void_p, dp, dp, dp, C.POINTER(CSmoothCovarianceReport)]
    L.aar_smooth_query_validate.argtypes = [C.c_int32, C.c_void_p, C.c_int64, dp]
    L.aar_track_smooth_query.argtypes = [C.c_void_p, dp, C.c_void_p, C.c_int64, dp, dp, dp, C.POINTER(C.c_int32),
                                         C.POINTER(CSmoothQueryReport)]
    L.aar_track_smooth_query2.argtypes = L.aar_track_smooth_query.argtypes
    L.aar_track_smooth_query2_step.argtypes = [C.c_void_p, dp, C.c_void_p, C.c_int64, dp, dp, dp]
    L.aar_track_smooth_lag3.argtypes = [C.c_void_p, dp, C.c_void_p, dp]
    L.aar_smooth_relative_validate.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.aar_track_smooth_relative.argtypes = [C.c_void_p, dp, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp, dp, dp,
                                            C.POINTER(CSmoothRelativeReport)]
    L.aar_track_smooth_detection_leverage.argtypes = [C.c_void_p, dp, C.c_void_p, dp, dp, C.POINTER(CSmoothPredictReport)]
    L.aar_track_smooth_detection_loo.argtypes = [C.c_void_p, dp, C.c_void_p, C.POINTER(CLooRule), dp, dp, dp, dp, dp, dp, u8p, u8p,
                                                 C.POINTER(CSmoothLooReport)]
    L.aar_track_smooth_predict_corners.argtypes = [C.c_void_p, dp, C.c_void_p, C.c_int64, ip32, ip32, dp, dp, dp, u8p, ip32,
                                                   C.POINTER(CSmoothPredictReport)]
    L.aar_track_smooth_gate_detections.argtypes = [C.c_void_p, dp, C.c_void_p, C.c_int64, ip32, ip32, dp, C.POINTER(C.c_float), dp, dp, u8p, ip32,
                                                   C.POINTER(CSmoothPredictReport)]
    L.aar_smooth_loo_write_yaml.argtypes = [C.c_char_p, C.POINTER(CDataset), dp, dp, dp, dp, u8p, u8p, C.POINTER(CSmoothLooReport)]
    L.aar_smooth_fit_default_params.argtypes = [C.POINTER(CSmoothFitParams)]
    L.aar_smooth_fit_default_params.restype = None
    L.aar_smooth_fit_params_validate.argtypes = [C.POINTER(CSmoothFitParams)]
    L.aar_track_smooth_fit.argtypes = [C.c_void_p, dp, C.POINTER(CLmParams), C.c_void_p, C.POINTER(CSmoothFitParams), dp,
                                       C.POINTER(CSmoothFitReport)]
    L.aar_track_smooth_fit_terms.argtypes = [C.c_void_p, dp, C.c_void_p, dp, dp]
    L.aar_track_smooth_fit2.argtypes = L.aar_track_smooth_fit.argtypes
    L.aar_track_smooth_fit_terms2.argtypes = L.aar_track_smooth_fit_terms.argtypes
    L.aar_tracker_default_params.argtypes = [C.POINTER(CTrackerParams)]
    L.aar_tracker_default_params.restype = None
    L.aar_tracker_params_validate.argtypes = [C.POINTER(CDataset), C.POINTER(CTrackerParams)]
    L.aar_tracker_create.argtypes = [C.POINTER(CDataset), C.POINTER(CTrackerParams), C.POINTER(CLmParams), C.POINTER(C.c_void_p)]
    L.aar_tracker_push.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), dp,
                                   C.POINTER(CTrackerResult)]
    L.aar_tracker_window.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), dp, dp, dp, dp, C.POINTER(C.c_int32)]
    L.aar_tracker_reset.argtypes = [C.c_void_p]
    L.aar_tracker_default_detection_params.argtypes = [C.POINTER(CTrackerDetectionParams)]
    L.aar_tracker_default_detection_params.restype = None
    L.aar_tracker_detection_params_validate.argtypes = [C.POINTER(CDataset), C.POINTER(CTrackerDetectionParams)]
    L.aar_tracker_enable_detections.argtypes = [C.c_void_p, C.POINTER(CTrackerDetectionParams)]
    L.aar_tracker_push_detections.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), dp,
                                              C.POINTER(CTrackerResult), C.POINTER(CTrackerStartInfo)]
    L.aar_tracker_uncertainty.argtypes = [C.c_void_p, C.POINTER(CTrackerUncertainty)]
    L.aar_tracker_covariance_write_yaml.argtypes = [C.c_char_p, C.POINTER(CDataset), dp, dp, C.POINTER(C.c_uint8)]
    L.aar_tracker_destroy.argtypes = [C.c_void_p]
    L.aar_tracker_destroy.restype = None
    dsp, u8p = C.POINTER(C.POINTER(CDataset)), C.POINTER(C.c_uint8)
    L.aar_tracker_bank_params_validate.argtypes = [C.c_int32, dsp, C.POINTER(CTrackerParams)]
    L.aar_tracker_bank_create.argtypes = [C.c_int32, dsp, C.POINTER(CTrackerParams), C.POINTER(CLmParams), C.POINTER(C.c_void_p)]
    L.aar_tracker_bank_size.argtypes = [C.c_void_p]
    L.aar_tracker_bank_size.restype = C.c_int32
    L.aar_tracker_bank_push.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                        dp, u8p, C.POINTER(CTrackerResult)]
    L.aar_tracker_bank_enable_detections.argtypes = [C.c_void_p, C.POINTER(C.POINTER(CTrackerDetectionParams))]
    L.aar_tracker_bank_push_detections.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                   C.POINTER(C.c_float), dp, u8p, C.POINTER(CTrackerResult), C.POINTER(CTrackerStartInfo)]
    L.aar_tracker_bank_window.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), dp, dp, dp, dp, C.POINTER(C.c_int32)]
    L.aar_tracker_bank_uncertainty.argtypes = [C.c_void_p, C.c_int32, C.POINTER(CTrackerUncertainty)]
    L.aar_tracker_bank_reset.argtypes = [C.c_void_p]
    L.aar_tracker_bank_get_stats.argtypes = [C.c_void_p, C.POINTER(CTrackerBankStats)]
    L.aar_tracker_bank_destroy.argtypes = [C.c_void_p]
    L.aar_tracker_bank_destroy.restype = None
    L.aar_tracker_default_gate_params.argtypes = [C.POINTER(CTrackerGateParams)]
    L.aar_tracker_default_gate_params.restype = None
    L.aar_tracker_gate_params_validate.argtypes = [C.POINTER(CTrackerGateParams)]
    L.aar_tracker_enable_gate.argtypes = [C.c_void_p, C.POINTER(CTrackerGateParams)]
    L.aar_tracker_last_gate.argtypes = [C.c_void_p, C.POINTER(CTrackerGateInfo)]
    L.aar_tracker_gate_detail.argtypes = [C.c_void_p, C.POINTER(C.c_int32), dp, u8p]
    L.aar_tracker_gate_bank_enable.argtypes = [C.c_void_p, C.POINTER(CTrackerGateParams)]
    L.aar_tracker_gate_bank_last.argtypes = [C.c_void_p, C.c_int32, C.POINTER(CTrackerGateInfo)]
    L.aar_tracker_gate_bank_detail.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), dp, u8p]
    L.aar_tracker_default_motion_params.argtypes = [C.POINTER(CTrackerMotionParams)]
    L.aar_tracker_default_motion_params.restype = None
    L.aar_tracker_motion_params_validate.argtypes = [C.POINTER(CTrackerParams), C.POINTER(CTrackerMotionParams)]
    L.aar_tracker_enable_motion.argtypes = [C.c_void_p, C.POINTER(CTrackerMotionParams)]
    L.aar_tracker_last_motion.argtypes = [C.c_void_p, C.POINTER(CTrackerMotionInfo)]
    L.aar_tracker_predict.argtypes = [C.c_void_p, C.c_double, dp]
    L.aar_tracker_motion_bank_enable.argtypes = [C.c_void_p, C.POINTER(CTrackerMotionParams)]
    L.aar_tracker_motion_bank_last.argtypes = [C.c_void_p, C.c_int32, C.POINTER(CTrackerMotionInfo)]
    L.aar_tracker_motion_bank_predict.argtypes = [C.c_void_p, C.c_int32, C.c_double, dp]
    L.aar_local_group_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    L.aar_local_group_destroy.argtypes = [C.c_void_p]
    L.aar_local_group_destroy.restype = None
    L.aar_comm_create_local.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.aar_cam_config_read.argtypes = [C.c_char_p, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.aar_undistort_points.argtypes = [dp, dp, C.c_int32, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32]
    ip, lp, fp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    L.aar_cam_configs_read.argtypes = [C.c_char_p, C.POINTER(C.POINTER(CCamModel)), ip]
    L.aar_cam_configs_read_ex.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.POINTER(CCamModel)), ip]
    L.aar_detections_read.argtypes = [C.c_char_p, ip, C.c_int32, C.POINTER(C.POINTER(CDetections))]
    L.aar_detections_free.argtypes = [C.POINTER(CDetections)]
    L.aar_detections_free.restype = None
    L.aar_subseqs_read.argtypes = [C.c_char_p, C.POINTER(ip), ip]
    L.aar_ippe_square.argtypes = [C.c_double, C.POINTER(CCamModel), C.c_int64, fp, dp, dp, dp, dp, C.c_int32]
    L.aar_vote_transforms.argtypes = [C.c_double, C.c_int64, lp, dp, dp, dp, lp, dp, dp, C.c_int32]
    L.aar_init_default_params.argtypes = [C.POINTER(CInitParams)]
    L.aar_init_default_params.restype = None
    L.aar_initializer_run.argtypes = [C.POINTER(CDetections), C.POINTER(CCamModel), C.c_int32, C.POINTER(CInitParams),
                                      C.POINTER(C.POINTER(CDataset))]
    L.aar_initializer_object_poses.argtypes = [C.POINTER(CDataset), C.POINTER(CDetections), C.POINTER(CCamModel), C.c_int32,
                                               C.POINTER(CInitParams), C.POINTER(C.POINTER(CDataset))]
    L.aar_lm_set_step_callback.argtypes = [C.c_void_p, STEP_CB, C.c_void_p, C.c_int32]
    L.aar_lm_set_stop_function.argtypes = [C.c_void_p, STOP_FN, C.c_void_p]
    L.aar_problem_extract_z.argtypes = [C.c_void_p, dp, dp]
    L.aar_problem_merge_z.argtypes = [C.c_void_p, dp, dp]
    L.aar_problem_set_huber_delta.argtypes = [C.c_void_p, C.c_float]
    L.aar_problem_get_huber_delta.argtypes = [C.c_void_p]
    L.aar_problem_get_huber_delta.restype = C.c_float
    _lib = L
    return L


def _check(rc):
    if rc != AAR_OK:
        raise AarError(rc, lib().aar_last_error().decode("utf-8", "replace"))


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _u8ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _np(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


class Dataset:
    """numpy copy of an aar_dataset (the content of a `.solution` file)."""

    FIELDS = ("cam_ids", "marker_ids", "frame_ids", "image_sizes", "cam_mats", "dist_coeffs", "obs_frame", "obs_cam",
              "obs_marker", "obs_uv", "x_full", "x_truth")

    def __init__(self, cptr=None):
        if cptr is None:
            return
        d = cptr.contents
        self.num_cams, self.num_markers, self.num_frames = d.num_cams, d.num_markers, d.num_frames
        self.root_cam, self.root_marker = d.root_cam, d.root_marker
        self.marker_size = d.marker_size
        self.num_obs = d.num_obs
        Cn, M, F, N = d.num_cams, d.num_markers, d.num_frames, d.num_obs
        full = 6 * (Cn - 1) + 6 * (M - 1) + 6 * F
        self.cam_ids = _np(d.cam_ids, Cn, np.int32)
        self.marker_ids = _np(d.marker_ids, M, np.int32)
        self.frame_ids = _np(d.frame_ids, F, np.int32)
        self.image_sizes = _np(d.image_sizes, 2 * Cn, np.int32).reshape(Cn, 2)
        self.cam_mats = _np(d.cam_mats, 9 * Cn, np.float64).reshape(Cn, 9)
        self.dist_coeffs = _np(d.dist_coeffs, 5 * Cn, np.float64).reshape(Cn, 5)
        self.obs_frame = _np(d.obs_frame, N, np.int32)
        self.obs_cam = _np(d.obs_cam, N, np.int32)
        self.obs_marker = _np(d.obs_marker, N, np.int32)
        self.obs_uv = _np(d.obs_uv, 8 * N, np.float32).reshape(N, 8)
        self.x_full = _np(d.x_full, full, np.float64)
        self.x_truth = _np(d.x_truth, full, np.float64) if d.x_truth else None
        self.optimize_cam_poses = bool(d.optimize_cam_poses)
        self.optimize_marker_poses = bool(d.optimize_marker_poses)
        self.optimize_object_poses = bool(d.optimize_object_poses)
        self.optimize_cam_intrinsics = bool(d.optimize_cam_intrinsics)

    @property
    def full_len(self):
        return 6 * (self.num_cams - 1) + 6 * (self.num_markers - 1) + 6 * self.num_frames

    def num_vars(self):
        n = 0
        if self.optimize_cam_poses:
            n += 6 * (self.num_cams - 1)
        if self.optimize_marker_poses:
            n += 6 * (self.num_markers - 1)
        if self.optimize_object_poses:
            n += 6 * self.num_frames
        return n

    def as_c(self):
        """A CDataset whose pointers alias this object's arrays (keep `self` alive while it is used)."""
        d = CDataset()
        d.num_cams, d.num_markers, d.num_frames = self.num_cams, self.num_markers, self.num_frames
        d.root_cam, d.root_marker = self.root_cam, self.root_marker
        d.marker_size = self.marker_size
        d.num_obs = self.num_obs
        self._keep = {}
        for name, ct, dt in (("cam_ids", C.c_int32, np.int32), ("marker_ids", C.c_int32, np.int32),
                             ("frame_ids", C.c_int32, np.int32), ("image_sizes", C.c_int32, np.int32),
                             ("cam_mats", C.c_double, np.float64), ("dist_coeffs", C.c_double, np.float64),
                             ("obs_frame", C.c_int32, np.int32), ("obs_cam", C.c_int32, np.int32),
                             ("obs_marker", C.c_int32, np.int32), ("obs_uv", C.c_float, np.float32),
                             ("x_full", C.c_double, np.float64)):
            a = np.ascontiguousarray(getattr(self, name), dtype=dt)
            self._keep[name] = a
            setattr(d, name, a.ctypes.data_as(C.POINTER(ct)))
        d.x_truth = None
        d.optimize_cam_poses = int(self.optimize_cam_poses)
        d.optimize_marker_poses = int(self.optimize_marker_poses)
        d.optimize_object_poses = int(self.optimize_object_poses)
        d.optimize_cam_intrinsics = int(self.optimize_cam_intrinsics)
        return d

    def select_observations(self, keep):
        """aar_dataset_select_observations: a copy with the observations where keep is true, in their order; every id, camera, frame,
        x_full and x_truth kept."""
        k = np.ascontiguousarray(keep).astype(np.uint8)
        if k.ndim != 1 or k.shape[0] != self.num_obs:
            raise ValueError("keep must have one entry per observation (%d), got shape %s" % (self.num_obs, k.shape))
        c = self.as_c()
        truth = None
        if self.x_truth is not None:
            truth = np.ascontiguousarray(self.x_truth, dtype=np.float64)
            c.x_truth = _dptr(truth)
        p = C.POINTER(CDataset)()
        _check(lib().aar_dataset_select_observations(C.byref(c), _u8ptr(k), C.byref(p)))
        try:
            return Dataset(p)
        finally:
            lib().aar_dataset_free(p)


def synth_desc(config_index, **over):
    sd = CSynthDesc()
    lib().aar_synth_default(C.byref(sd), config_index)
    for k, v in over.items():
        setattr(sd, k, v)
    return sd


def synth(config_index, **over):
    """Deterministic synthetic data set; config_index 2..5 = BASELINE.json configs[1..4]."""
    sd = synth_desc(config_index, **over)
    p = C.POINTER(CDataset)()
    _check(lib().aar_synth_generate(C.byref(sd), C.byref(p)))
    try:
        return Dataset(p)
    finally:
        lib().aar_dataset_free(p)


def solution_read(path, reference_indexing=False):
    p = C.POINTER(CDataset)()
    _check(lib().aar_solution_read_ex(path.encode(), 1 if reference_indexing else 0, C.byref(p)))
    try:
        return Dataset(p)
    finally:
        lib().aar_dataset_free(p)


def solution_write(path, ds):
    c = ds.as_c()
    _check(lib().aar_solution_write(path.encode(), C.byref(c)))


def solution_write_yaml(path, ds):
    c = ds.as_c()
    _check(lib().aar_solution_write_yaml(path.encode(), C.byref(c)))


def detections_write(path, ds):
    c = ds.as_c()
    _check(lib().aar_detections_write(path.encode(), C.byref(c)))


def rodrigues_vec2mat(w):
    w = np.ascontiguousarray(w, dtype=np.float64)
    R = np.zeros(9)
    lib().aar_rodrigues_vec2mat(_dptr(w), _dptr(R))
    return R.reshape(3, 3)


def rodrigues_mat2vec(R):
    R = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
    w = np.zeros(3)
    lib().aar_rodrigues_mat2vec(_dptr(R), _dptr(w))
    return w


def relative_pose(x6_a, x6_b):
    """aar_relative_pose: the (rvec, t) of T_a^-1 T_b for two poses given as (rvec, t) -- a pair prior's x6_rel"""
    a = np.ascontiguousarray(x6_a, dtype=np.float64).reshape(6)
    b = np.ascontiguousarray(x6_b, dtype=np.float64).reshape(6)
    out = np.zeros(6)
    _check(lib().aar_relative_pose(_dptr(a), _dptr(b), _dptr(out)))
    return out


MAX_DIST = 12


def cam_config_read(path):
    """calib.{xml,yml,yaml} of one camera -> (K 3x3, dist (n,), (width, height)) -- libs/cam_config.cpp:52-80."""
    K = np.zeros(9)
    dist = np.zeros(MAX_DIST)
    n, w, h = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _check(lib().aar_cam_config_read(path.encode(), _dptr(K), _dptr(dist), C.byref(n), C.byref(w), C.byref(h)))
    return K.reshape(3, 3), dist[: n.value].copy(), (w.value, h.value)


def undistort_points(K, dist, uv, device=0):
    """MultiCamMapper::remove_distortions for one camera's corners (libs/multicam_mapper.cpp:554-578) on the GPU."""
    K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
    dist = np.ascontiguousarray(dist, dtype=np.float64).reshape(-1)
    uv = np.ascontiguousarray(uv, dtype=np.float32)
    out = np.empty_like(uv)
    fp = C.POINTER(C.c_float)
    _check(lib().aar_undistort_points(_dptr(K), _dptr(dist) if len(dist) else None, len(dist), uv.size // 2,
                                      uv.ctypes.data_as(fp), out.ctypes.data_as(fp), device))
    return out


# ---- Initializer (libs/initializer.cpp) ----
def cam_models(Ks, dists, sizes=None):
    """array of aar_cam_model, one per camera slot"""
    arr = (CCamModel * max(len(Ks), 1))()
    for i, (K, d) in enumerate(zip(Ks, dists)):
        K = np.asarray(K, dtype=np.float64).reshape(9)
        d = np.asarray(d, dtype=np.float64).reshape(-1)
        for j in range(9):
            arr[i].K[j] = K[j]
        for j in range(MAX_DIST):
            arr[i].dist[j] = d[j] if j < len(d) else 0.0
        arr[i].n_dist = len(d)
        if sizes is not None:
            arr[i].width, arr[i].height = int(sizes[i][0]), int(sizes[i][1])
    return arr


def cam_configs_read(folder, readdir_order=False):
    """CamConfig::read_cam_configs: list of (K 3x3, dist, (w, h)) in ascending sub-directory order (or readdir order, as the reference)"""
    p = C.POINTER(CCamModel)()
    n = C.c_int32(0)
    _check(lib().aar_cam_configs_read_ex(folder.encode(), 1 if readdir_order else 0, C.byref(p), C.byref(n)))
    out = []
    for i in range(n.value):
        m = p[i]
        out.append((np.array(m.K[:]).reshape(3, 3), np.array(m.dist[: m.n_dist]), (m.width, m.height)))
    C.CDLL(None).free(p)
    return out


class Detections:
    """numpy copy of an aar_detections (the content of an aruco.detections file)"""

    def __init__(self, num_cams, num_frames, det_frame, det_cam, det_id, det_uv):
        self.num_cams, self.num_frames = int(num_cams), int(num_frames)
        self.det_frame = np.ascontiguousarray(det_frame, dtype=np.int32)
        self.det_cam = np.ascontiguousarray(det_cam, dtype=np.int32)
        self.det_id = np.ascontiguousarray(det_id, dtype=np.int32)
        self.det_uv = np.ascontiguousarray(det_uv, dtype=np.float32).reshape(-1, 8)

    def as_c(self):
        c = CDetections()
        c.num_cams, c.num_frames, c.num_det = self.num_cams, self.num_frames, len(self.det_frame)
        ip = C.POINTER(C.c_int32)
        c.det_frame = self.det_frame.ctypes.data_as(ip)
        c.det_cam = self.det_cam.ctypes.data_as(ip)
        c.det_id = self.det_id.ctypes.data_as(ip)
        c.det_uv = self.det_uv.ctypes.data_as(C.POINTER(C.c_float))
        return c


def detections_read(path, subseqs=None):
    """Initializer::read_detections_file (libs/initializer.cpp:316-362)"""
    p = C.POINTER(CDetections)()
    ss = np.ascontiguousarray(subseqs if subseqs is not None else [], dtype=np.int32)
    _check(lib().aar_detections_read(path.encode(), ss.ctypes.data_as(C.POINTER(C.c_int32)) if len(ss) else None, len(ss),
                                     C.byref(p)))
    try:
        d = p.contents
        n = d.num_det
        return Detections(d.num_cams, d.num_frames, _np(d.det_frame, n, np.int32), _np(d.det_cam, n, np.int32),
                          _np(d.det_id, n, np.int32), _np(d.det_uv, 8 * n, np.float32))
    finally:
        lib().aar_detections_free(p)


def subseqs_read(path):
    p = C.POINTER(C.c_int32)()
    n = C.c_int32(0)
    _check(lib().aar_subseqs_read(path.encode(), C.byref(p), C.byref(n)))
    out = _np(p, n.value, np.int32)
    C.CDLL(None).free(p)
    return out


def ippe_square(marker_size, K, dist, uv, device=0):
    """aruco::solvePnP_ for n markers of one camera on the GPU: (T1[n,4,4], e1[n], T2[n,4,4], e2[n])"""
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 8)
    n = len(uv)
    cams = cam_models([K], [dist])
    T1 = np.zeros((max(n, 1), 16)); T2 = np.zeros((max(n, 1), 16)); e1 = np.zeros(max(n, 1)); e2 = np.zeros(max(n, 1))
    _check(lib().aar_ippe_square(float(marker_size), cams, n, uv.ctypes.data_as(C.POINTER(C.c_float)), _dptr(T1), _dptr(e1),
                                 _dptr(T2), _dptr(e2), device))
    return T1[:n].reshape(n, 4, 4), e1[:n], T2[:n].reshape(n, 4, 4), e2[:n]


def vote_transforms(marker_size, set_begin, T, T1inv, T2inv, device=0):
    """Initializer::find_best_transformation for several candidate sets on the GPU: (best[s], weight[s], cost[n])"""
    sb = np.ascontiguousarray(set_begin, dtype=np.int64)
    ns = len(sb) - 1
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1, 16)
    A = np.ascontiguousarray(T1inv, dtype=np.float64).reshape(-1, 16)
    B = np.ascontiguousarray(T2inv, dtype=np.float64).reshape(-1, 16)
    n = len(T)
    best = np.zeros(max(ns, 1), dtype=np.int64); weight = np.zeros(max(ns, 1)); cost = np.zeros(max(n, 1))
    lp = C.POINTER(C.c_int64)
    _check(lib().aar_vote_transforms(float(marker_size), ns, sb.ctypes.data_as(lp), _dptr(T), _dptr(A), _dptr(B),
                                     best.ctypes.data_as(lp), _dptr(weight), _dptr(cost), device))
    return best[:ns], weight[:ns], cost[:n]


def initializer_run(det, Ks, dists, marker_size, sizes=None, excluded=(), threshold=2.0, min_detections=2, device=0,
                    solution=None):
    """Initializer(...) + MultiCamMapper(Initializer&): the data set the reference writes as initial.solution.
    With `solution` (a Dataset): apps/track.cpp's use -- its cameras / markers stay fixed, only the object poses of the
    detections' frames are initialised (aar_initializer_object_poses)."""
    prm = CInitParams()
    lib().aar_init_default_params(C.byref(prm))
    prm.marker_size, prm.threshold, prm.min_detections, prm.device_id = marker_size, threshold, min_detections, device
    ex = np.ascontiguousarray(list(excluded), dtype=np.int32)
    prm.n_excluded = len(ex)
    prm.excluded_cams = ex.ctypes.data_as(C.POINTER(C.c_int32)) if len(ex) else None
    cams = cam_models(Ks, dists, sizes)
    c = det.as_c()
    p = C.POINTER(CDataset)()
    if solution is None:
        _check(lib().aar_initializer_run(C.byref(c), cams, len(Ks), C.byref(prm), C.byref(p)))
    else:
        sc = solution.as_c()
        _check(lib().aar_initializer_object_poses(C.byref(sc), C.byref(c), cams, len(Ks), C.byref(prm), C.byref(p)))
    try:
        return Dataset(p)
    finally:
        lib().aar_dataset_free(p)


def plan_shards(obs_per_frame, world):
    c = np.ascontiguousarray(obs_per_frame, dtype=np.int64)
    begin = np.zeros(world + 1, dtype=np.int32)
    _check(lib().aar_plan_shards(len(c), c.ctypes.data_as(C.POINTER(C.c_int64)), world,
                                 begin.ctypes.data_as(C.POINTER(C.c_int32))))
    return begin


def device_count():
    return lib().aar_device_count()


def lm_default_params(**over):
    p = CLmParams()
    lib().aar_lm_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


class Comm:
    """RCCL communicator of one rank (multi-GPU)."""

    @staticmethod
    def make_id():
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _check(lib().aar_comm_make_id(buf))
        return buf.raw

    def __init__(self, uid, world, rank, device):
        self.handle = C.c_void_p()
        self.world, self.rank = world, rank
        _check(lib().aar_comm_create(uid, world, rank, device, C.byref(self.handle)))

    @classmethod
    def local(cls, group, rank, device=0):
        """Rank `rank` of an in-process LocalGroup (all ranks on one GPU, one host thread each)."""
        self = cls.__new__(cls)
        self.handle = C.c_void_p()
        self.world, self.rank = group.world, rank
        _check(lib().aar_comm_create_local(group.handle, rank, device, C.byref(self.handle)))
        return self

    def stats(self):
        st = CCommStats()
        _check(lib().aar_comm_get_stats(self.handle, C.byref(st)))
        return {n: getattr(st, n) for n, _ in CCommStats._fields_}

    def close(self):
        if self.handle:
            lib().aar_comm_destroy(self.handle)
            self.handle = C.c_void_p()


class LocalGroup:
    """aar_local_group: the in-process stand-in for an RCCL communicator (tests / bring-up on a 1-GPU box)."""

    def __init__(self, world):
        self.world = world
        self.handle = C.c_void_p()
        _check(lib().aar_local_group_create(world, C.byref(self.handle)))

    def close(self):
        if self.handle:
            lib().aar_local_group_destroy(self.handle)
            self.handle = C.c_void_p()


class Covariance:
    """What Problem.covariance returns (see there)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def covariance_write_yaml(path, ds, entity_diag_flat, sigma2, frames=None):
    """aar_covariance_write_yaml: entity_diag_flat / frames as Problem.covariance returns them (a problem created from ds, its optimize flags)"""
    c = ds.as_c()
    d = np.ascontiguousarray(entity_diag_flat, dtype=np.float64)
    fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.float64).reshape(-1)
    _check(lib().aar_covariance_write_yaml(path.encode(), C.byref(c), _dptr(d), _dptr(fr) if fr is not None else None, float(sigma2)))


class ResidualReport:
    """What Problem.residual_report returns (see there)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _report_c(rep):
    r = CResidualReport()
    r.struct_size = C.sizeof(CResidualReport)
    for name, _ in CResidualReport._fields_[1:]:
        setattr(r, name, rep[name])
    return r


def residual_report_write_yaml(path, ds, rr, det_err=True):
    """aar_residual_report_write_yaml: rr as Problem.residual_report returns it for a (single-GPU) problem created from ds; det_err=False
    leaves the list of rejected detections out"""
    c = ds.as_c()
    cs = np.ascontiguousarray(rr.cam_stats, dtype=np.float64)
    ms = np.ascontiguousarray(rr.marker_stats, dtype=np.float64)
    e = np.ascontiguousarray(rr.det_err, dtype=np.float64) if det_err else None
    k = np.ascontiguousarray(rr.keep, dtype=np.uint8) if det_err else None
    r = _report_c(rr.report)
    _check(lib().aar_residual_report_write_yaml(path.encode(), C.byref(c), _dptr(cs), _dptr(ms), _dptr(e) if det_err else None,
                                                _u8ptr(k) if det_err else None, C.byref(r)))


def _queries(queries):
    """queries [Q, 3] = (camera index, marker index, frame index) -> three contiguous int32 arrays"""
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    if len(q) and (np.abs(q) > 2 ** 31 - 1).any():
        raise ValueError("a query index does not fit 32 bits")
    return [np.ascontiguousarray(q[:, k], dtype=np.int32) for k in range(3)]


def _i32ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if len(a) else None


def predict_query_validate(ds, queries):
    """aar_predict_query_validate (host code): raises AarError(AAR_ERR_INVALID) naming the first query whose index is out of range"""
    cds = ds.as_c()
    d = CProblemDesc()
    lib().aar_problem_desc_from_dataset(C.byref(cds), C.byref(d))
    qc, qm, qf = _queries(queries)
    _check(lib().aar_predict_query_validate(C.byref(d), len(qc), _i32ptr(qc), _i32ptr(qm), _i32ptr(qf)))


def _predict_report_dict(rep):
    return {name: getattr(rep, name) for name, _ in CPredictReport._fields_[1:]}


def _loo_report_dict(rep):
    d = {name: getattr(rep, name) for name, _ in CLooReport._fields_[2:]}
    d["predict"] = _predict_report_dict(rep.predict)
    return d


class DetectionLoo:
    """What Problem.detection_loo returns (aar_problem_detection_loo)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def loo_write_yaml(path, ds, loo, det_err=None):
    """aar_loo_write_yaml: loo as Problem.detection_loo returns it for a (single-GPU) problem created from ds; det_err as
    Problem.residual_report(x).det_err, or None"""
    c = ds.as_c()
    r = CLooReport()
    r.struct_size = C.sizeof(CLooReport)
    for name, _ in CLooReport._fields_[2:]:
        setattr(r, name, loo.report[name])
    r.predict.struct_size = C.sizeof(CPredictReport)
    for name, _ in CPredictReport._fields_[1:]:
        setattr(r.predict, name, loo.report["predict"][name])
    F, q, lev = (np.ascontiguousarray(getattr(loo, k), dtype=np.float64) for k in ("F", "q", "leverage"))
    st, keep = (np.ascontiguousarray(getattr(loo, k), dtype=np.uint8) for k in ("status", "keep"))
    e = None if det_err is None else np.ascontiguousarray(det_err, dtype=np.float64)
    _check(lib().aar_loo_write_yaml(path.encode(), C.byref(c), _dptr(F), _dptr(q), _dptr(lev), _dptr(e) if e is not None else None, _u8ptr(st),
                                    _u8ptr(keep), C.byref(r)))


def smooth_loo_write_yaml(path, ds, loo, det_err=None):
    """aar_smooth_loo_write_yaml: loo as Problem.track_smooth_detection_loo returns it for a (single-GPU) problem created from ds; det_err as
    Problem.residual_report(x).det_err, or None"""
    c = ds.as_c()
    r = CSmoothLooReport()
    r.struct_size = C.sizeof(CSmoothLooReport)
    for name, _ in CSmoothLooReport._fields_[1:]:
        setattr(r, name, loo.report[name])
    F, q, lev = (np.ascontiguousarray(getattr(loo, k), dtype=np.float64) for k in ("F", "q", "leverage"))
    st, keep = (np.ascontiguousarray(getattr(loo, k), dtype=np.uint8) for k in ("status", "keep"))
    e = None if det_err is None else np.ascontiguousarray(det_err, dtype=np.float64)
    _check(lib().aar_smooth_loo_write_yaml(path.encode(), C.byref(c), _dptr(F), _dptr(q), _dptr(lev), _dptr(e) if e is not None else None,
                                           _u8ptr(st), _u8ptr(keep), C.byref(r)))


def leverage_write_yaml(path, ds, leverage, report, h_min=0.0, det_err=None):
    """aar_leverage_write_yaml: leverage / report as Problem.detection_leverage returns them for a (single-GPU) problem created from ds;
    det_err as Problem.residual_report(...).det_err, or None"""
    c = ds.as_c()
    lv = np.ascontiguousarray(leverage, dtype=np.float64)
    e = None if det_err is None else np.ascontiguousarray(det_err, dtype=np.float64)
    r = CPredictReport()
    r.struct_size = C.sizeof(CPredictReport)
    for name, _ in CPredictReport._fields_[1:]:
        setattr(r, name, report[name])
    _check(lib().aar_leverage_write_yaml(path.encode(), C.byref(c), _dptr(lv) if len(lv) else None, _dptr(e) if e is not None else None,
                                         float(h_min), C.byref(r)))


def tracker_detection_params(Ks=None, dists=None, ippe_threshold=None, min_detections=None, start_policy=None, struct_size=None):
    """(aar_tracker_detection_params, the camera array it points to) from Python values (None = the library's default; Ks / dists by camera
    INDEX, None = the solution's own); start_policy: "vote" | "best" or the number"""
    p = CTrackerDetectionParams()
    lib().aar_tracker_default_detection_params(C.byref(p))
    cams = None
    if Ks is not None:
        cams = cam_models(Ks, dists if dists is not None else [np.zeros(0)] * len(Ks))
        p.cams = C.cast(cams, C.POINTER(CCamModel))
    if ippe_threshold is not None:
        p.ippe_threshold = float(ippe_threshold)
    if min_detections is not None:
        p.min_detections = int(min_detections)
    if start_policy is not None:
        p.start_policy = TRACKER_STARTS.get(start_policy, start_policy)
    if struct_size is not None:
        p.struct_size = int(struct_size)
    return p, cams


def tracker_detection_params_validate(ds, **kw):
    """aar_tracker_detection_params_validate (host code): raises AarError(AAR_ERR_INVALID) with the library's message"""
    c = ds.as_c()
    p, cams = tracker_detection_params(**kw)
    _check(lib().aar_tracker_detection_params_validate(C.byref(c), C.byref(p)))


def tracker_gate_params(k_median=None, min_px=None, min_detections=None, struct_size=None):
    """aar_tracker_gate_params from Python values (None = the library's default: 6, 3, 4)"""
    p = CTrackerGateParams()
    lib().aar_tracker_default_gate_params(C.byref(p))
    if k_median is not None:
        p.k_median = float(k_median)
    if min_px is not None:
        p.min_px = float(min_px)
    if min_detections is not None:
        p.min_detections = int(min_detections)
    if struct_size is not None:
        p.struct_size = int(struct_size)
    return p


def tracker_gate_params_validate(**kw):
    """aar_tracker_gate_params_validate (host code): raises AarError(AAR_ERR_INVALID) with the library's message"""
    p = tracker_gate_params(**kw)
    _check(lib().aar_tracker_gate_params_validate(C.byref(p)))


TRACKER_MOTIONS = {"random_walk": 0, "rw": 0, "constant_velocity": 1, "cv": 1}


def tracker_motion_params(model=None, max_dt=None, struct_size=None):
    """aar_tracker_motion_params from Python values (None = the library's default: constant velocity, no max_dt); model: "cv" |
    "constant_velocity" | "rw" | "random_walk" (or the integer)"""
    p = CTrackerMotionParams()
    lib().aar_tracker_default_motion_params(C.byref(p))
    if model is not None:
        p.model = int(TRACKER_MOTIONS.get(model, model))
    if max_dt is not None:
        p.max_dt = float(max_dt)
    if struct_size is not None:
        p.struct_size = int(struct_size)
    return p


def tracker_motion_params_validate(tracker=None, **kw):
    """aar_tracker_motion_params_validate (host code): raises AarError(AAR_ERR_INVALID) with the library's message.  tracker: a dict of
    tracker_params' keywords (None: smooth = 1, lag 0, unit sigmas)"""
    tp = tracker_params(**(dict(smooth=True, sigma_rot=1.0, sigma_trans=1.0) if tracker is None else tracker))
    p = tracker_motion_params(**kw)
    _check(lib().aar_tracker_motion_params_validate(C.byref(tp), C.byref(p)))


def _tracker_motion_info(m):
    return dict(model=m.model, predicted=m.predicted, rel=np.array(m.rel[:]), velocity=np.array(m.velocity[:]), newest_time=m.newest_time)


def _tracker_gate_info(g):
    return {k: getattr(g, k) for k, _ in CTrackerGateInfo._fields_ if k != "struct_size"}


def _tracker_result(r):
    out = {k: getattr(r, k) for k, _ in CTrackerResult._fields_ if k not in ("struct_size", "pose", "lagged_pose")}
    out["pose"] = np.array(r.pose[:])
    out["lagged_pose"] = np.array(r.lagged_pose[:]) if r.has_lagged else None
    return out


def _tracker_start_info(si):
    info = {k: getattr(si, k) for k, _ in CTrackerStartInfo._fields_ if k not in ("struct_size", "start_pose")}
    info["start_pose"] = np.array(si.start_pose[:])
    return info


def _tracker_uncertainty(u):
    w = u.window_frames
    return dict(cov_valid=u.cov_valid, sigma2=u.sigma2, window_frames=w, frame_index=np.array(u.frame_index[:w], dtype=np.int64),
                cov=np.array(u.cov[:36 * w]).reshape(w, 6, 6), has_marginal=u.has_marginal, marginal_index=u.marginal_index,
                marginal_info=np.array(u.marginal_info[:]).reshape(6, 6), marginal_mean=np.array(u.marginal_mean[:]),
                marginal_dropped=u.marginal_dropped)


def tracker_bank_params_validate(solutions, n_members=None, **kw):
    """aar_tracker_bank_params_validate (host code): raises AarError(AAR_ERR_INVALID) with the library's message.  solutions: data sets, a None
    entry is passed as a null pointer; n_members: the count to pass (default len(solutions))"""
    cds = [None if d is None else d.as_c() for d in solutions]
    arr = (C.POINTER(CDataset) * max(len(cds), 1))(*[C.pointer(c) if c is not None else None for c in cds])
    p = tracker_params(**kw)
    _check(lib().aar_tracker_bank_params_validate(len(cds) if n_members is None else int(n_members), arr, C.byref(p)))


class TrackerBank:
    """aar_tracker_bank: B live trackers, one per solution in `solutions`, with the same parameters, advanced in lockstep --
    one copy in, one launch of B workgroups, one copy out per push."""

    def __init__(self, solutions, lag=0, smooth=False, sigma_rot=0.0, sigma_trans=0.0, with_huber=False, huber_delta=None, max_obs_per_frame=None,
                 device=0, params=None, anchor="fixed", covariance=False, gate=None, motion=None):
        """gate: None, or a dict of tracker_gate_params' keywords: enable_gate(**gate) right after creation; motion: None, a
        model name ("cv") or a dict of tracker_motion_params' keywords: enable_motion(**motion) right after creation"""
        self.solutions = list(solutions)
        self._cds = [d.as_c() for d in self.solutions]
        arr = (C.POINTER(CDataset) * len(self._cds))(*[C.pointer(c) for c in self._cds])
        self.prm = tracker_params(lag, smooth, sigma_rot, sigma_trans, with_huber, huber_delta, max_obs_per_frame, device, anchor=anchor,
                                  covariance=covariance)
        self.handle = C.c_void_p()
        _check(lib().aar_tracker_bank_create(len(self._cds), arr, C.byref(self.prm), C.byref(params) if params is not None else None,
                                             C.byref(self.handle)))
        self.size = lib().aar_tracker_bank_size(self.handle)
        if gate is not None:
            self.enable_gate(**gate)
        if motion is not None:
            self.enable_motion(**(motion if isinstance(motion, dict) else dict(model=motion)))

    def close(self):
        if self.handle:
            lib().aar_tracker_bank_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __len__(self):
        return self.size

    def pack(self, frames, pose_init):
        """frames: [B] of (cam, marker, uv [n, 8]); pose_init: None, [B, 6], or a list of [6] / None per member"""
        B = self.size
        assert len(frames) == B
        n = np.array([len(np.reshape(f[0], -1)) for f in frames], dtype=np.int32)
        cam = np.ascontiguousarray(np.concatenate([np.reshape(f[0], -1) for f in frames]), dtype=np.int32)
        mk = np.ascontiguousarray(np.concatenate([np.reshape(f[1], -1) for f in frames]), dtype=np.int32)
        uv = np.ascontiguousarray(np.concatenate([np.reshape(f[2], -1) for f in frames]), dtype=np.float32)
        assert len(mk) == len(cam) and len(uv) == 8 * len(cam)
        init = has = None
        if pose_init is not None and any(z is not None for z in pose_init):
            assert len(pose_init) == B
            has = np.array([z is not None for z in pose_init], dtype=np.uint8)
            init = np.ascontiguousarray([np.zeros(6) if z is None else np.reshape(z, 6) for z in pose_init], dtype=np.float64)
        ip = C.POINTER(C.c_int32)
        return (n.ctypes.data_as(ip), cam.ctypes.data_as(ip), mk.ctypes.data_as(ip), uv.ctypes.data_as(C.POINTER(C.c_float)),
                _dptr(init) if init is not None else None, _u8ptr(has) if has is not None else None), (n, cam, mk, uv, init, has)

    def result_array(self):
        r = (CTrackerResult * self.size)()
        for x in r:
            x.struct_size = C.sizeof(CTrackerResult)
        return r

    def push(self, frame_time, frames, pose_init=None):
        """aar_tracker_bank_push: frames [B] of (obs_cam, obs_marker, obs_uv [n, 8]) in the member's own indices; pose_init None, or per member
        a pose [6] or None.  Returns the [B] result dicts of Tracker.push."""
        args, keep = self.pack(frames, pose_init)
        r = self.result_array()
        _check(lib().aar_tracker_bank_push(self.handle, float(frame_time), *args, r))
        return [_tracker_result(x) for x in r]

    def enable_detections(self, per_member=None):
        """aar_tracker_bank_enable_detections: per_member None or [B] of None / a dict of tracker_detection_params' keywords"""
        keep = [None if kw is None else tracker_detection_params(**kw) for kw in (per_member or [None] * self.size)]
        assert len(keep) == self.size
        arr = (C.POINTER(CTrackerDetectionParams) * self.size)(*[C.pointer(k[0]) if k is not None else None for k in keep])
        _check(lib().aar_tracker_bank_enable_detections(self.handle, arr))

    def push_detections(self, frame_time, frames, pose_init=None):
        """aar_tracker_bank_push_detections: as push() with RAW corners.  Returns ([B] results, [B] start infos)."""
        args, keep = self.pack(frames, pose_init)
        r = self.result_array()
        si = (CTrackerStartInfo * self.size)()
        for x in si:
            x.struct_size = C.sizeof(CTrackerStartInfo)
        _check(lib().aar_tracker_bank_push_detections(self.handle, float(frame_time), *args, r, si))
        return [_tracker_result(x) for x in r], [_tracker_start_info(x) for x in si]

    def window(self, member):
        """aar_tracker_bank_window: Tracker.window() of one member"""
        cap = TRACKER_MAX_LAG + 1
        n, has = C.c_int32(0), C.c_int32(0)
        idx = np.zeros(cap, dtype=np.int64)
        poses, fe, pe, anchor = np.zeros((cap, 6)), np.zeros(cap), np.zeros(cap), np.zeros(6)
        _check(lib().aar_tracker_bank_window(self.handle, int(member), C.byref(n), idx.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(poses), _dptr(fe),
                                             _dptr(pe), _dptr(anchor), C.byref(has)))
        w = n.value
        return dict(n=w, frame_index=idx[:w].copy(), poses=poses[:w].copy(), frame_err=fe[:w].copy(), pair_err=pe[:w].copy(),
                    anchor_pose=anchor if has.value else None)

    def uncertainty(self, member):
        """aar_tracker_bank_uncertainty: Tracker.uncertainty() of one member"""
        u = CTrackerUncertainty()
        u.struct_size = C.sizeof(CTrackerUncertainty)
        _check(lib().aar_tracker_bank_uncertainty(self.handle, int(member), C.byref(u)))
        return _tracker_uncertainty(u)

    def reset(self):
        _check(lib().aar_tracker_bank_reset(self.handle))

    def enable_gate(self, k_median=None, min_px=None, min_detections=None):
        """aar_tracker_gate_bank_enable: once after creation or reset; one parameter set for all members"""
        p = tracker_gate_params(k_median, min_px, min_detections)
        _check(lib().aar_tracker_gate_bank_enable(self.handle, C.byref(p)))

    def enable_motion(self, model=None, max_dt=None):
        """aar_tracker_motion_bank_enable: once after creation or reset; one parameter set for all members"""
        p = tracker_motion_params(model, max_dt)
        _check(lib().aar_tracker_motion_bank_enable(self.handle, C.byref(p)))

    def last_motion(self, member):
        """aar_tracker_motion_bank_last: Tracker.last_motion() of one member"""
        m = CTrackerMotionInfo()
        m.struct_size = C.sizeof(CTrackerMotionInfo)
        _check(lib().aar_tracker_motion_bank_last(self.handle, int(member), C.byref(m)))
        return _tracker_motion_info(m)

    def predict(self, member, time):
        """aar_tracker_motion_bank_predict: Tracker.predict() of one member"""
        pose = np.zeros(6)
        _check(lib().aar_tracker_motion_bank_predict(self.handle, int(member), float(time), _dptr(pose)))
        return pose

    def last_gate(self, member):
        """aar_tracker_gate_bank_last: Tracker.last_gate() of one member"""
        g = CTrackerGateInfo()
        g.struct_size = C.sizeof(CTrackerGateInfo)
        _check(lib().aar_tracker_gate_bank_last(self.handle, int(member), C.byref(g)))
        return _tracker_gate_info(g)

    def gate_detail(self, member):
        """aar_tracker_gate_bank_detail: Tracker.gate_detail() of one member"""
        cap = int(self.prm.max_obs_per_frame)
        n, e, k = C.c_int32(0), np.zeros(cap), np.zeros(cap, dtype=np.uint8)
        _check(lib().aar_tracker_gate_bank_detail(self.handle, int(member), C.byref(n), _dptr(e), _u8ptr(k)))
        return e[:n.value].copy(), k[:n.value].copy()

    def stats(self, struct_size=None):
        """aar_tracker_bank_get_stats: dict(members, pushes, launches, h2d_copies, h2d_bytes, d2h_copies, d2h_bytes) counted on the host"""
        st = CTrackerBankStats()
        st.struct_size = C.sizeof(CTrackerBankStats) if struct_size is None else int(struct_size)
        _check(lib().aar_tracker_bank_get_stats(self.handle, C.byref(st)))
        return {k: getattr(st, k) for k, _ in CTrackerBankStats._fields_}


class Tracker:
    """aar_tracker: the live tracker.  Built from a solution data set (its cameras, markers, cam_mats, marker_size and
    roots; its frames are ignored) and fed one frame per push."""

    def __init__(self, ds, lag=0, smooth=False, sigma_rot=0.0, sigma_trans=0.0, with_huber=False, huber_delta=None, max_obs_per_frame=None,
                 device=0, params=None, anchor="fixed", covariance=False, gate=None, motion=None):
        """params: aar_lm_params (lm_default_params(...)) or None for the defaults; anchor "fixed" | "marginal", covariance: DESIGN.md
        section 19 (uncertainty() after a push); gate: None, or a dict of tracker_gate_params' keywords:
        enable_gate(**gate) right after creation; motion: None, a model name ("cv") or a dict of tracker_motion_params' keywords (DESIGN.md
        section 25): enable_motion(**motion) right after creation"""
        self.ds = ds
        self._cds = ds.as_c()
        self.prm = tracker_params(lag, smooth, sigma_rot, sigma_trans, with_huber, huber_delta, max_obs_per_frame, device, anchor=anchor,
                                  covariance=covariance)
        self.handle = C.c_void_p()
        _check(lib().aar_tracker_create(C.byref(self._cds), C.byref(self.prm), C.byref(params) if params is not None else None,
                                        C.byref(self.handle)))
        if gate is not None:
            self.enable_gate(**gate)
        if motion is not None:
            self.enable_motion(**(motion if isinstance(motion, dict) else dict(model=motion)))

    def close(self):
        if self.handle:
            lib().aar_tracker_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def push(self, frame_time, obs_cam, obs_marker, obs_uv, pose_init=None):
        """aar_tracker_push: one frame's detections (camera / marker INDICES, undistorted corners [n, 8]).  Returns a dict of the
        aar_tracker_result fields (pose, lagged_pose as arrays; lagged_pose None until the window is full)."""
        cam = np.ascontiguousarray(obs_cam, dtype=np.int32).reshape(-1)
        mk = np.ascontiguousarray(obs_marker, dtype=np.int32).reshape(-1)
        uv = np.ascontiguousarray(obs_uv, dtype=np.float32).reshape(-1)
        n = len(cam)
        assert len(mk) == n and len(uv) == 8 * n
        init = None if pose_init is None else np.ascontiguousarray(pose_init, dtype=np.float64).reshape(6)
        r = CTrackerResult()
        r.struct_size = C.sizeof(CTrackerResult)
        ip = C.POINTER(C.c_int32)
        _check(lib().aar_tracker_push(self.handle, float(frame_time), n, cam.ctypes.data_as(ip), mk.ctypes.data_as(ip),
                                      uv.ctypes.data_as(C.POINTER(C.c_float)), _dptr(init) if init is not None else None, C.byref(r)))
        return _tracker_result(r)

    def enable_detections(self, Ks=None, dists=None, ippe_threshold=None, min_detections=None, start_policy=None):
        """aar_tracker_enable_detections: once after creation or reset (see tracker_detection_params)"""
        p, cams = tracker_detection_params(Ks, dists, ippe_threshold, min_detections, start_policy)
        _check(lib().aar_tracker_enable_detections(self.handle, C.byref(p)))

    def push_detections(self, frame_time, det_cam, det_marker, uv_raw, pose_init=None):
        """aar_tracker_push_detections: one frame's RAW detections (camera / marker INDICES, corners as detected [n, 8]).  Returns
        (result, info): push()'s dict and a dict of the aar_tracker_start_info fields (start_pose as an array)."""
        cam = np.ascontiguousarray(det_cam, dtype=np.int32).reshape(-1)
        mk = np.ascontiguousarray(det_marker, dtype=np.int32).reshape(-1)
        uv = np.ascontiguousarray(uv_raw, dtype=np.float32).reshape(-1)
        n = len(cam)
        assert len(mk) == n and len(uv) == 8 * n
        init = None if pose_init is None else np.ascontiguousarray(pose_init, dtype=np.float64).reshape(6)
        r, si = CTrackerResult(), CTrackerStartInfo()
        r.struct_size, si.struct_size = C.sizeof(CTrackerResult), C.sizeof(CTrackerStartInfo)
        ip = C.POINTER(C.c_int32)
        _check(lib().aar_tracker_push_detections(self.handle, float(frame_time), n, cam.ctypes.data_as(ip), mk.ctypes.data_as(ip),
                                                 uv.ctypes.data_as(C.POINTER(C.c_float)), _dptr(init) if init is not None else None, C.byref(r),
                                                 C.byref(si)))
        return _tracker_result(r), _tracker_start_info(si)

    def window(self):
        """aar_tracker_window: dict(n, frame_index [n], poses [n, 6], frame_err [n], pair_err [n] (entry i: the pair that ends at window
        frame i; entry 0 the anchor pair), anchor_pose [6] or None)"""
        cap = TRACKER_MAX_LAG + 1
        n, has = C.c_int32(0), C.c_int32(0)
        idx = np.zeros(cap, dtype=np.int64)
        poses, fe, pe, anchor = np.zeros((cap, 6)), np.zeros(cap), np.zeros(cap), np.zeros(6)
        _check(lib().aar_tracker_window(self.handle, C.byref(n), idx.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(poses), _dptr(fe), _dptr(pe),
                                        _dptr(anchor), C.byref(has)))
        w = n.value
        return dict(n=w, frame_index=idx[:w].copy(), poses=poses[:w].copy(), frame_err=fe[:w].copy(), pair_err=pe[:w].copy(),
                    anchor_pose=anchor if has.value else None)

    def uncertainty(self):
        """aar_tracker_uncertainty after the last push: dict(cov_valid, sigma2, window_frames, frame_index [W], cov [W, 6, 6] (unscaled blocks of
        H^-1, oldest first), has_marginal, marginal_index, marginal_info [6, 6], marginal_mean [6], marginal_dropped)"""
        u = CTrackerUncertainty()
        u.struct_size = C.sizeof(CTrackerUncertainty)
        _check(lib().aar_tracker_uncertainty(self.handle, C.byref(u)))
        return _tracker_uncertainty(u)

    def enable_gate(self, k_median=None, min_px=None, min_detections=None):
        """aar_tracker_enable_gate: once after creation or reset, before the first push (see tracker_gate_params)"""
        p = tracker_gate_params(k_median, min_px, min_detections)
        _check(lib().aar_tracker_enable_gate(self.handle, C.byref(p)))

    def last_gate(self):
        """aar_tracker_last_gate: dict(gated, n_in, n_kept, n_nonfinite, median, max, threshold) of the last accepted push"""
        g = CTrackerGateInfo()
        g.struct_size = C.sizeof(CTrackerGateInfo)
        _check(lib().aar_tracker_last_gate(self.handle, C.byref(g)))
        return _tracker_gate_info(g)

    def gate_detail(self):
        """aar_tracker_gate_detail: (e_d [n_in], keep [n_in] uint8) of the newest frame in the order it was pushed"""
        cap = int(self.prm.max_obs_per_frame)
        n, e, k = C.c_int32(0), np.zeros(cap), np.zeros(cap, dtype=np.uint8)
        _check(lib().aar_tracker_gate_detail(self.handle, C.byref(n), _dptr(e), _u8ptr(k)))
        return e[:n.value].copy(), k[:n.value].copy()

    def enable_motion(self, model=None, max_dt=None):
        """aar_tracker_enable_motion: once after creation or reset, before the first push (see tracker_motion_params)"""
        p = tracker_motion_params(model, max_dt)
        _check(lib().aar_tracker_enable_motion(self.handle, C.byref(p)))

    def last_motion(self):
        """aar_tracker_last_motion: dict(model, predicted, rel [6], velocity [6], newest_time) of the last accepted push"""
        m = CTrackerMotionInfo()
        m.struct_size = C.sizeof(CTrackerMotionInfo)
        _check(lib().aar_tracker_last_motion(self.handle, C.byref(m)))
        return _tracker_motion_info(m)

    def predict(self, time):
        """aar_tracker_predict: the newest pose carried to time with the last push's velocity, [6] (rvec, t)"""
        pose = np.zeros(6)
        _check(lib().aar_tracker_predict(self.handle, float(time), _dptr(pose)))
        return pose

    def reset(self):
        _check(lib().aar_tracker_reset(self.handle))


class Problem:
    """aar_problem: the bundle-adjustment problem resident on one GPU."""

    def __init__(self, ds, residual_mode=RES_F32, device=0, comm=None, optimize=None, with_huber=False, intrinsics=False,
                 solver=None, deterministic=None, pcg_eta=None, pcg_max_it=None, pcg_eta_loose=None, pcg_eta_switch=None, pcg_abs_tol=None,
                 fixed_cams=None, fixed_markers=None, priors=None, constrained=False, pair_priors=None):
        """intrinsics=True: Config::optimize_cam_intrinsics -- every vector ends with 9 per camera (x_with_intrinsics builds one)
        solver ("direct" | "spcg" | "pcg" | "auto"), deterministic, pcg_eta, pcg_max_it, pcg_eta_loose, pcg_eta_switch: aar_solver_options
        (None = the library's default: solver AUTO -- direct for one tile of unknowns, SPCG wherever it fits, PCG for many entities per frame x many frames -- with
        one pose-grade forcing term and an absolute tolerance; a forcing SEQUENCE only when pcg_eta_loose is given)
        fixed_cams, fixed_markers (indices), priors (list of (kind, index, x6, info)): aar_problem_constraints, created through
        aar_problem_create_constrained (also taken, with empty constraints, when constrained=True)
        pair_priors (list of (kind, index_a, index_b, x6_rel, info)): relative pose priors between two cameras / two markers"""
        self.ds = ds
        self._cds = ds.as_c()
        d = CProblemDesc()
        lib().aar_problem_desc_from_dataset(C.byref(self._cds), C.byref(d))
        if optimize is not None:
            d.optimize_cam_poses, d.optimize_marker_poses, d.optimize_object_poses = [int(b) for b in optimize]
        d.optimize_cam_intrinsics = int(intrinsics)
        d.residual_mode = residual_mode
        d.with_huber = int(with_huber)
        d.device_id = device
        d.comm = comm.handle if comm is not None else None
        self.optimize = (bool(d.optimize_cam_poses), bool(d.optimize_marker_poses), bool(d.optimize_object_poses))
        self.intrinsics = bool(intrinsics)
        self.handle = C.c_void_p()
        self._cons = Constraints(fixed_cams, fixed_markers, priors, pair_priors)
        self.n_priors = self._cons.n_priors
        self.n_pair_priors = self._cons.n_pair_priors
        if all(v is None for v in (solver, deterministic, pcg_eta, pcg_max_it, pcg_eta_loose, pcg_eta_switch, pcg_abs_tol)) and \
                self._cons.empty() and not constrained:
            _check(lib().aar_problem_create(C.byref(d), C.byref(self.handle)))
        else:
            so = CSolverOptions()
            lib().aar_solver_default_options(C.byref(so))
            if solver is not None:
                so.solver = SOLVERS[solver] if isinstance(solver, str) else int(solver)
            if deterministic is not None:
                so.deterministic = int(bool(deterministic))
            if pcg_eta is not None:
                so.pcg_eta = float(pcg_eta)
            if pcg_max_it is not None:
                so.pcg_max_it = int(pcg_max_it)
            if pcg_eta_loose is not None:
                so.pcg_eta_loose = float(pcg_eta_loose)
            if pcg_eta_switch is not None:
                so.pcg_eta_switch = float(pcg_eta_switch)
            if pcg_abs_tol is not None:
                so.pcg_abs_tol = float(pcg_abs_tol)
            if self._cons.empty() and not constrained:
                _check(lib().aar_problem_create_ex(C.byref(d), C.byref(so), C.byref(self.handle)))
            else:
                _check(lib().aar_problem_create_constrained(C.byref(d), C.byref(so), C.byref(self._cons.c), C.byref(self.handle)))
        self.full_len = lib().aar_problem_full_len(self.handle)
        self.num_vars = lib().aar_problem_num_vars(self.handle)
        self.local_obs = lib().aar_problem_local_obs(self.handle)

    def close(self):
        if self.handle:
            lib().aar_problem_destroy(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _x(self, x_full):
        x = np.ascontiguousarray(x_full, dtype=np.float64)
        assert x.shape == (self.full_len,)
        return x

    def x_with_intrinsics(self, x_pose):
        """pose vector + the data set's (fx cx fy cy d0..d4) per camera: the `.solution` vector (libs/multicam_mapper.cpp:1085-1089)"""
        K = np.asarray(self.ds.cam_mats, dtype=np.float64).reshape(-1, 9)
        d = np.asarray(self.ds.dist_coeffs, dtype=np.float64).reshape(-1, 5)
        intr = np.concatenate([np.stack([K[:, 0], K[:, 2], K[:, 4], K[:, 5]], axis=1), d], axis=1).reshape(-1)
        return np.concatenate([np.asarray(x_pose, dtype=np.float64), intr])

    def eval_residuals(self, x_full, want_vector=True):
        x = self._x(x_full)
        ss = C.c_double()
        r = np.zeros(8 * self.ds.num_obs) if want_vector else None
        _check(lib().aar_eval_residuals(self.handle, _dptr(x), _dptr(r) if want_vector else None, C.byref(ss)))
        return r, ss.value

    def eval_normal_equations(self, x_full):
        x = self._x(x_full)
        P = self.num_vars
        H = np.zeros((P, P))
        B = np.zeros(P)
        ss = C.c_double()
        _check(lib().aar_eval_normal_equations(self.handle, _dptr(x), _dptr(H), _dptr(B), C.byref(ss)))
        return H, B, ss.value

    def eval_priors(self, x_full):
        """aar_problem_eval_priors: (e [n_priors][6], summed cost e^T L e) at x_full"""
        x = self._x(x_full)
        e = np.zeros((max(self.n_priors, 1), 6))
        cost = C.c_double()
        _check(lib().aar_problem_eval_priors(self.handle, _dptr(x), _dptr(e), C.byref(cost)))
        return e[:self.n_priors], cost.value

    def eval_pair_priors(self, x_full):
        """aar_problem_eval_pair_priors: (e [n_pair_priors][6], summed cost e^T L e) at x_full"""
        x = self._x(x_full)
        e = np.zeros((max(self.n_pair_priors, 1), 6))
        cost = C.c_double()
        _check(lib().aar_problem_eval_pair_priors(self.handle, _dptr(x), _dptr(e), C.byref(cost)))
        return e[:self.n_pair_priors], cost.value

    def eval_damped_step(self, x_full, mu):
        x = self._x(x_full)
        delta = np.zeros(self.num_vars)
        _check(lib().aar_eval_damped_step(self.handle, _dptr(x), mu, _dptr(delta)))
        return delta

    def entity_block_sizes(self):
        """sizes of the z-order diagonal blocks of the non-frame unknowns: 6 per camera / marker, 9 per intrinsics entity"""
        oc, om, _ = self.optimize
        return [6] * ((self.ds.num_cams - 1) if oc else 0) + [6] * ((self.ds.num_markers - 1) if om else 0) + \
            [9] * (self.ds.num_cams if self.intrinsics else 0)

    def covariance(self, x_full, dense=False, frames=True):
        """aar_problem_covariance: (J^T J)^-1 at x_full, UNSCALED (times .sigma2 for the covariance), z ordering, NaN where a parameter has no
        unknown or is unobserved.  Returns a Covariance: sigma2, sum_sq, num_residuals, num_vars, min_pivot, max_pivot, frames_written,
        entity_diag (list of 6x6 / 9x9 blocks in z order), entity_cov (Pe x Pe, dense=True only), frames ([F][6][6] or None; on a sharded
        problem only this rank's frames are filled, the others NaN)."""
        x = self._x(x_full)
        sizes = self.entity_block_sizes()
        pe = sum(sizes)
        diag = np.full(sum(b * b for b in sizes), np.nan)
        ecov = np.full((pe, pe), np.nan) if dense else None
        want_fr = frames and self.optimize[2]
        fr = np.full((self.ds.num_frames, 36), np.nan) if want_fr else None
        rep = CCovarianceReport()
        rep.struct_size = C.sizeof(CCovarianceReport)
        _check(lib().aar_problem_covariance(self.handle, _dptr(x), _dptr(ecov) if dense else None, _dptr(diag),
                                            _dptr(fr) if want_fr else None, C.byref(rep)))
        blocks, o = [], 0
        for b in sizes:
            blocks.append(diag[o:o + b * b].reshape(b, b))
            o += b * b
        return Covariance(sigma2=rep.sigma2, sum_sq=rep.sum_sq, num_residuals=rep.num_residuals, num_vars=rep.num_vars,
                          min_pivot=rep.min_pivot, max_pivot=rep.max_pivot, frames_written=rep.frames_written,
                          entity_diag=blocks, entity_diag_flat=diag, entity_cov=ecov,
                          frames=fr.reshape(-1, 6, 6) if want_fr else None)

    def predict_corners(self, x_full, queries, covariance=True):
        """aar_problem_predict_corners at x_full for queries [Q, 3] = (camera index, marker index, frame index).  Returns (uv [Q, 4, 2],
        cov [Q, 8, 8] UNSCALED -- None with covariance=False, which runs no covariance chain --, status [Q] (PREDICT_BEHIND | PREDICT_UNDEFINED
        bits), report dict of the aar_predict_report fields).  A corner's a-posteriori covariance is report["sigma2"] * cov; the search
        window of a NEW detection is report["sigma2"] * (cov + I)."""
        x = self._x(x_full)
        qc, qm, qf = _queries(queries)
        n = len(qc)
        uv = np.full((max(n, 1), 8), np.nan)
        cov = np.full((max(n, 1), 64), np.nan) if covariance else None
        st = np.zeros(max(n, 1), dtype=np.uint8)
        rep = CPredictReport()
        rep.struct_size = C.sizeof(CPredictReport)
        _check(lib().aar_problem_predict_corners(self.handle, _dptr(x), n, _i32ptr(qc), _i32ptr(qm), _i32ptr(qf), _dptr(uv),
                                                 _dptr(cov) if covariance else None, _u8ptr(st), C.byref(rep)))
        return uv[:n].reshape(n, 4, 2), (cov[:n].reshape(n, 8, 8) if covariance else None), st[:n], _predict_report_dict(rep)

    def detection_leverage(self, x_full, rows=False):
        """aar_problem_detection_leverage at x_full: (leverage [local_obs] = tr(C_i) of this problem's detections in reference order,
        row_leverage [local_obs, 8] = diag(C_i) or None, report dict)"""
        x = self._x(x_full)
        n = self.local_obs
        lv = np.full(max(n, 1), np.nan)
        rw = np.full((max(n, 1), 8), np.nan) if rows else None
        rep = CPredictReport()
        rep.struct_size = C.sizeof(CPredictReport)
        _check(lib().aar_problem_detection_leverage(self.handle, _dptr(x), _dptr(lv), _dptr(rw) if rows else None, C.byref(rep)))
        return lv[:n], (rw[:n] if rows else None), _predict_report_dict(rep)

    def detection_loo(self, x_full, f_max=None):
        """aar_problem_detection_loo at x_full, with the rule F > f_max when f_max is given.  Returns a DetectionLoo: loo_resid [local_obs, 8],
        q, F, cook, leverage, margin [local_obs], status, keep [local_obs] (uint8) and report: the aar_loo_report fields as a dict, its
        "predict" entry the dict of the aar_predict_report inside.  q is UNSCALED: q / report["predict"]["sigma2"] is the chi-square."""
        x = self._x(x_full)
        n = self.local_obs
        m = max(n, 1)
        w = np.full((m, 8), np.nan)
        q, F, cook, lev, margin = (np.full(m, np.nan) for _ in range(5))
        st, keep = np.zeros(m, dtype=np.uint8), np.ones(m, dtype=np.uint8)
        rule = None
        if f_max is not None:
            rule = CLooRule()
            rule.struct_size = C.sizeof(CLooRule)
            rule.f_max = float(f_max)
        rep = CLooReport()
        rep.struct_size = C.sizeof(CLooReport)
        _check(lib().aar_problem_detection_loo(self.handle, _dptr(x), C.byref(rule) if rule is not None else None, _dptr(w), _dptr(q), _dptr(F),
                                               _dptr(cook), _dptr(lev), _dptr(margin), _u8ptr(st), _u8ptr(keep), C.byref(rep)))
        return DetectionLoo(loo_resid=w[:n], q=q[:n], F=F[:n], cook=cook[:n], leverage=lev[:n], margin=margin[:n], status=st[:n], keep=keep[:n],
                            report=_loo_report_dict(rep))

    def gate_detections(self, x_full, cams, markers, frames, uv_obs):
        """aar_problem_gate_detections at x_full for candidate detections (camera index, marker index, frame index) with observed corners
        uv_obs [Q, 4, 2] or [Q, 8] (undistorted pixels; stored as float32).  Returns (innovation [Q, 8] = uv_obs - predicted, m2 [Q] =
        e^T (I + C)^-1 e UNSCALED -- m2 / report["sigma2"] is chi-square with 8 degrees of freedom --, status [Q], report dict)."""
        x = self._x(x_full)
        qc, qm, qf = _queries(np.stack([np.asarray(cams).reshape(-1), np.asarray(markers).reshape(-1), np.asarray(frames).reshape(-1)], axis=1))
        n = len(qc)
        uv = np.ascontiguousarray(np.asarray(uv_obs, dtype=np.float32).reshape(-1, 8))
        if len(uv) != n:
            raise ValueError("gate_detections: %d queries, %d sets of corners" % (n, len(uv)))
        inn = np.full((max(n, 1), 8), np.nan)
        m2 = np.full(max(n, 1), np.nan)
        st = np.zeros(max(n, 1), dtype=np.uint8)
        rep = CPredictReport()
        rep.struct_size = C.sizeof(CPredictReport)
        _check(lib().aar_problem_gate_detections(self.handle, _dptr(x), n, _i32ptr(qc), _i32ptr(qm), _i32ptr(qf),
                                                 uv.ctypes.data_as(C.POINTER(C.c_float)) if n else None, _dptr(inn), _dptr(m2), _u8ptr(st),
                                                 C.byref(rep)))
        return inn[:n], m2[:n], st[:n], _predict_report_dict(rep)

    def residual_report(self, x_full, k_median=0.0, min_px=0.0, rule=None):
        """aar_problem_residual_report at x_full.  The rule's threshold is max(min_px, k_median * median) (k_median <= 0: min_px; both <= 0:
        +inf); rule=False passes no rule at all (the same threshold), rule=None passes one when k_median or min_px is set.  Returns a
        ResidualReport: det_err, keep ([local_obs], this rank's detections in reference order), cam_stats [C][4], marker_stats [M][4],
        frame_stats [F][4] ({detections, sum r^2, max e_d, rejected}; on a sharded problem only this rank's frames, the others NaN) and
        report (a dict of the aar_residual_report fields)."""
        x = self._x(x_full)
        n = self.local_obs
        e = np.zeros(max(n, 1))
        k = np.zeros(max(n, 1), dtype=np.uint8)
        cs = np.zeros((self.ds.num_cams, 4))
        ms = np.zeros((self.ds.num_markers, 4))
        fs = np.full((max(self.ds.num_frames, 1), 4), np.nan)
        use = (k_median != 0 or min_px != 0) if rule is None else bool(rule)
        r = COutlierRule()
        r.struct_size = C.sizeof(COutlierRule)
        r.k_median, r.min_px = float(k_median), float(min_px)
        rep = CResidualReport()
        rep.struct_size = C.sizeof(CResidualReport)
        _check(lib().aar_problem_residual_report(self.handle, _dptr(x), C.byref(r) if use else None, _dptr(e), _u8ptr(k), _dptr(cs), _dptr(ms),
                                                 _dptr(fs), C.byref(rep)))
        report = {name: getattr(rep, name) for name, _ in CResidualReport._fields_[1:]}
        return ResidualReport(det_err=e[:n], keep=k[:n].astype(bool), cam_stats=cs, marker_stats=ms, frame_stats=fs[:self.ds.num_frames],
                              report=report)

    def reproj_stats(self, x_full):
        x = self._x(x_full)
        rmse, ss = C.c_double(), C.c_double()
        _check(lib().aar_reproj_stats(self.handle, _dptr(x), C.byref(rmse), C.byref(ss)))
        return rmse.value, ss.value

    def lm_init(self, x_full, params=None):
        x = self._x(x_full)
        _check(lib().aar_lm_init(self.handle, _dptr(x), C.byref(params) if params is not None else None))

    def lm_step(self):
        it = CLmIter()
        _check(lib().aar_lm_step(self.handle, C.byref(it)))
        return dict(err=it.err, mu=it.mu, gain=it.gain, delta_norm=it.delta_norm, accepted=it.accepted, tries=it.tries)

    def lm_get_solution(self):
        x = np.array(self.ds.x_full, dtype=np.float64)
        err = C.c_double()
        _check(lib().aar_lm_get_solution(self.handle, _dptr(x), C.byref(err)))
        return x, err.value

    def lm_solve(self, x_full, params=None, trace_cap=256):
        x = np.array(self._x(x_full), dtype=np.float64)
        rep = CLmReport()
        tr = (CLmIter * trace_cap)()
        rep.trace = tr
        rep.trace_cap = trace_cap
        _check(lib().aar_lm_solve(self.handle, _dptr(x), C.byref(params) if params is not None else None, C.byref(rep)))
        n = min(rep.iterations, trace_cap)
        trace = [dict(err=tr[i].err, mu=tr[i].mu, gain=tr[i].gain, delta_norm=tr[i].delta_norm,
                      accepted=tr[i].accepted, tries=tr[i].tries) for i in range(n)]
        report = dict(iterations=rep.iterations, stop_code=rep.stop_code, initial_err=rep.initial_err,
                      final_err=rep.final_err, final_mu=rep.final_mu, solve_seconds=rep.solve_seconds,
                      trial_points=rep.trial_points, trace=trace)
        return x, report

    def track(self, x_full, params=None):
        """MultiCamMapper::track() for every frame at once: returns (x_full with refined frame poses, iterations[F], err[F])."""
        x = np.array(self._x(x_full), dtype=np.float64)
        it = np.zeros(self.ds.num_frames, dtype=np.int32)
        err = np.zeros(self.ds.num_frames)
        _check(lib().aar_track(self.handle, _dptr(x), C.byref(params) if params is not None else None,
                               it.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(err)))
        return x, it, err

    def track_smooth(self, x_full, sigma_rot, sigma_trans, frame_time=None, rel_motion=None, params=None, model=None, sigma_rot0=0.0, sigma_trans0=0.0):
        """aar_track_smooth: every frame's pose with a motion prior between consecutive frames, one joint LM on the device.  Returns
        (x_full with the smoothed frame poses, report dict, frame_err [F] = E_f, pair_err [F-1] = e_f^T L_f e_f)."""
        x = np.array(self._x(x_full), dtype=np.float64)
        F = self.ds.num_frames
        sp = SmoothParams(sigma_rot, sigma_trans, frame_time, rel_motion, None, model, sigma_rot0, sigma_trans0)
        sp.check_lengths(F)
        fe, pe = np.zeros(max(F, 1)), np.zeros(max(F - 1, 1))
        rep = CSmoothReport()
        rep.struct_size = C.sizeof(CSmoothReport)
        _check(lib().aar_track_smooth(self.handle, _dptr(x), C.byref(params) if params is not None else None, C.byref(sp.c),
                                      _dptr(fe), _dptr(pe), C.byref(rep)))
        report = {k: getattr(rep, k) for k, _ in CSmoothReport._fields_ if k != "struct_size"}
        return x, report, fe[:F], pe[:max(F - 1, 0)]

    # The smoother's entries come in pairs: aar_..., and aar_...2 with one more output (off2, lag2_cov, sums [6]) for either motion model.
    # Each pair shares one helper below; fn: the C function's name, two: it is the ...2 one.  sp_args: SmoothParams' arguments.
    def _smooth_call(self, x_full, sp_args, rep_type=None):
        """(x, F, SmoothParams, the zeroed report or None) that every helper starts from"""
        x = self._x(x_full)
        sp = SmoothParams(*sp_args)
        sp.check_lengths(self.ds.num_frames)
        rep = None
        if rep_type is not None:
            rep = rep_type()
            rep.struct_size = C.sizeof(rep_type)
        return x, self.ds.num_frames, sp, rep

    @staticmethod
    def _report(rep):
        return {k: getattr(rep, k) for k, _ in type(rep)._fields_ if k != "struct_size"}

    def _smooth_system(self, fn, two, x_full, mu, sp_args):
        x, F, sp, _ = self._smooth_call(x_full, sp_args)
        diag, off, off2 = np.zeros((max(F, 1), 6, 6)), np.zeros((max(F - 1, 1), 6, 6)), np.zeros((max(F - 2, 1), 6, 6))
        rhs, delta, cost = np.zeros(6 * max(F, 1)), np.zeros(6 * max(F, 1)), np.zeros(2)
        _check(getattr(lib(), fn)(self.handle, _dptr(x), C.byref(sp.c), float(mu), _dptr(diag), _dptr(off), *([_dptr(off2)] if two else []),
                                  _dptr(rhs), _dptr(delta), _dptr(cost)))
        return (diag[:F], off[:max(F - 1, 0)], *([off2[:max(F - 2, 0)]] if two else []), rhs[:6 * F], delta[:6 * F], (cost[0], cost[1]))

    def _smooth_covariance(self, fn, two, lag2, x_full, sp_args):
        x, F, sp, rep = self._smooth_call(x_full, sp_args, CSmoothCovarianceReport)
        fc, lc, l2 = np.zeros((max(F, 1), 6, 6)), np.zeros((max(F - 1, 1), 6, 6)), np.zeros((max(F - 2, 1), 6, 6))
        _check(getattr(lib(), fn)(self.handle, _dptr(x), C.byref(sp.c), _dptr(fc), _dptr(lc), *([_dptr(l2) if lag2 else None] if two else []),
                                  C.byref(rep)))
        return (fc[:F], lc[:max(F - 1, 0)], *([l2[:max(F - 2, 0)] if lag2 else None] if two else []), self._report(rep))

    def _smooth_fit(self, fn, x_full, params, fit, sp_args):
        x, _, sp, rep = self._smooth_call(x_full, sp_args, CSmoothFitReport)
        x = np.array(x, dtype=np.float64)
        fp = fit if isinstance(fit, CSmoothFitParams) else smooth_fit_params(**(fit or {}))
        path = np.zeros((max(int(fp.max_iters), 0) + 1, 3))
        _check(getattr(lib(), fn)(self.handle, _dptr(x), C.byref(params) if params is not None else None, C.byref(sp.c), C.byref(fp), _dptr(path),
                                  C.byref(rep)))
        report = self._report(rep)
        return x, report, path[:report["iterations"] + 1]

    def _smooth_fit_terms(self, fn, two, x_full, sp_args):
        x, F, sp, _ = self._smooth_call(x_full, sp_args)
        terms, sums = np.zeros((max(F - 1, 1), 4)), np.zeros(6 if two else 4)
        _check(getattr(lib(), fn)(self.handle, _dptr(x), C.byref(sp.c), _dptr(terms), _dptr(sums)))
        return terms[:max(F - 1, 0)], sums

    def _smooth_query(self, fn, x_full, query_time, covariance, sp_args):
        x, _, sp, rep = self._smooth_call(x_full, sp_args, CSmoothQueryReport)
        qt = np.ascontiguousarray(query_time, dtype=np.float64).reshape(-1)
        Q = len(qt)
        pose, seg = np.zeros((max(Q, 1), 6)), np.zeros(max(Q, 1), dtype=np.int32)
        cov = np.zeros((max(Q, 1), 6, 6)) if covariance else None
        _check(getattr(lib(), fn)(self.handle, _dptr(x), C.byref(sp.c), Q, _dptr(qt) if Q else None, _dptr(pose), _dptr(cov) if covariance else None,
                                  seg.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(rep)))
        return pose[:Q], cov[:Q] if covariance else None, seg[:Q], self._report(rep)

    def track_smooth_system(self, x_full, sigma_rot, sigma_trans, mu, frame_time=None, rel_motion=None, model=None, sigma_rot0=0.0, sigma_trans0=0.0):
        """aar_track_smooth_system: (diag [F, 6, 6], off [F-1, 6, 6], rhs [6F], delta [6F], (data cost, prior cost)) of one try at x_full"""
        return self._smooth_system("aar_track_smooth_system", False, x_full, mu,
                                   (sigma_rot, sigma_trans, frame_time, rel_motion, None, model, sigma_rot0, sigma_trans0))

    def track_smooth_system2(self, x_full, sigma_rot, sigma_trans, mu, frame_time=None, rel_motion=None, model=None, sigma_rot0=0.0, sigma_trans0=0.0):
        """aar_track_smooth_system2, either model: (diag [F, 6, 6], off [F-1, 6, 6], off2 [F-2, 6, 6], rhs [6F], delta [6F], (data cost, prior
        cost)) of one try at x_full; off2 is zero under the random walk"""
        return self._smooth_system("aar_track_smooth_system2", True, x_full, mu,
                                   (sigma_rot, sigma_trans, frame_time, rel_motion, None, model, sigma_rot0, sigma_trans0))

    def track_smooth_covariance(self, x_full, sigma_rot, sigma_trans, frame_time=None, rel_motion=None, model=None, sigma_rot0=0.0, sigma_trans0=0.0):
        """aar_track_smooth_covariance: (frame_cov [F, 6, 6] = (H^-1)_ff, lag_cov [F-1, 6, 6] = (H^-1)_{f,f+1}, report dict) at x_full, H the
        matrix of track_smooth_system at mu = 0.  Both UNSCALED: multiply by report["sigma2"]."""
        return self._smooth_covariance("aar_track_smooth_covariance", False, False, x_full,
                                       (sigma_rot, sigma_trans, frame_time, rel_motion, None, model, sigma_rot0, sigma_trans0))

    def track_smooth_covariance2(self, x_full, sigma_rot, sigma_trans, frame_time=None, rel_motion=None, model=None, sigma_rot0=0.0, sigma_trans0=0.0,
                                 lag2=True):
        """aar_track_smooth_covariance2, either model: (frame_cov [F, 6, 6] = (H^-1)_ff, lag_cov [F-1, 6, 6] = (H^-1)_{f,f+1}, lag2_cov
        [F-2, 6, 6] = (H^-1)_{f,f+2}, report dict) at x_full, H the matrix of track_smooth_system2 at mu = 0.  All UNSCALED: multiply by
        report["sigma2"].  lag2=False passes NULL for lag2_cov (the random walk refuses it otherwise) and returns None in its place."""
        return self._smooth_covariance("aar_track_smooth_covariance2", True, lag2, x_full,
                                       (sigma_rot, sigma_trans, frame_time, rel_motion, None, model, sigma_rot0, sigma_trans0))

    def track_smooth_fit(self, x_full, sigma_rot, sigma_trans, frame_time=None, rel_motion=None, params=None, fit=None, model=None, sigma_rot0=0.0, sigma_trans0=0.0):
        """aar_track_smooth_fit: the pixel noise and the motion sigmas fitted to the sequence by EM, from the effective start values
        sigma_rot, sigma_trans.  fit: None (the defaults), a dict of aar_smooth_fit_params fields, or a CSmoothFitParams.  Returns (x_full with
        the track at the fitted values, report dict, path [iterations + 1, 3] = (sigma_px, sigma_rot, sigma_trans) per iteration).  Hand
        report["sigma_rot_eff"], report["sigma_trans_eff"] to track_smooth / tracker_params."""
        return self._smooth_fit("aar_track_smooth_fit", x_full, params, fit,
                                (sigma_rot, sigma_trans, frame_time, rel_motion, None, model, sigma_rot0, sigma_trans0))

    def track_smooth_fit_terms(self, x_full, sigma_rot, sigma_trans, frame_time=None, rel_motion=None, model=None, sigma_rot0=0.0, sigma_trans0=0.0):
        """aar_track_smooth_fit_terms: one E-step at x_full and the given effective sigmas, no smoothing.  Returns (pair_terms [F-1, 4] =
        a_r, u_r, a_t, u_t, sums [4] = A_r, U_r, A_t, U_t)."""
        return self._smooth_fit_terms("aar_track_smooth_fit_terms", False, x_full,
                                      (sigma_rot, sigma_trans, frame_time, rel_motion, None, model, sigma_rot0, sigma_trans0))

    def track_smooth_fit2(self, x_full, sigma_rot, sigma_trans, frame_time=None, rel_motion=None, params=None, fit=None, model=None, sigma_rot0=0.0, sigma_trans0=0.0):
        """aar_track_smooth_fit2, either model: track_smooth_fit's arguments and returns.  Under constant velocity sigma_rot0, sigma_trans0 are
        physical and held; smooth afterwards with report["sigma_rot_eff"], report["sigma_trans_eff"] and sigma_rot0 / report["sigma_px"],
        sigma_trans0 / report["sigma_px"]."""
        return self._smooth_fit("aar_track_smooth_fit2", x_full, params, fit,
                                (sigma_rot, sigma_trans, frame_time, rel_motion, None, model, sigma_rot0, sigma_trans0))

    def track_smooth_fit_terms2(self, x_full, sigma_rot, sigma_trans, frame_time=None, rel_motion=None, model=None, sigma_rot0=0.0, sigma_trans0=0.0):
        """aar_track_smooth_fit_terms2, either model: one E-step at x_full and the given effective sigmas, no smoothing.  Returns (pair_terms
        [F-1, 4] = a_r, u_r, a_t, u_t with entry 0 = pair 0, sums [6] = A_r, U_r, A_t, U_t over the terms 1 .. F-2, u_0, pair 0's cost; the
        last two are zero under the random walk, whose sums run over every pair)."""
        return self._smooth_fit_terms("aar_track_smooth_fit_terms2", True, x_full,
                                      (sigma_rot, sigma_trans, frame_time, rel_motion, None, model, sigma_rot0, sigma_trans0))

    def track_smooth_query(self, x_full, sigma_rot, sigma_trans, query_time, frame_time=None, covariance=True, model=None, sigma_rot0=0.0, sigma_trans0=0.0):
        """aar_track_smooth_query: the smoothed track at the times query_time [Q] (any order, duplicates allowed).  Returns (pose [Q, 6],
        cov [Q, 6, 6] UNSCALED -- multiply by report["sigma2"] -- or None without covariance, segment [Q], report dict)."""
        return self._smooth_query("aar_track_smooth_query", x_full, query_time, covariance,
                                  (sigma_rot, sigma_trans, frame_time, None, None, model, sigma_rot0, sigma_trans0))

    def track_smooth_query2(self, x_full, sigma_rot, sigma_trans, query_time, frame_time=None, covariance=True, model=None, sigma_rot0=0.0, sigma_trans0=0.0):
        """aar_track_smooth_query2, either model: track_smooth_query's arguments and returns.  Under constant velocity the answer is one
        Gauss-Newton step of the smoother for a frame without detections inserted at the query's time; covariance=False runs the same chain and
        saves the copy of the blocks alone."""
        return self._smooth_query("aar_track_smooth_query2", x_full, query_time, covariance,
                                  (sigma_rot, sigma_trans, frame_time, None, None, model, sigma_rot0, sigma_trans0))

    def track_smooth_query2_step(self, x_full, sigma_rot, sigma_trans, query_time, frame_time=None, model="cv", sigma_rot0=0.0, sigma_trans0=0.0):
        """aar_track_smooth_query2_step (constant velocity, for checking): (start_pose [Q, 6], step [Q, 6]), the two summands of
        track_smooth_query2's pose"""
        x = self._x(x_full)
        sp = SmoothParams(sigma_rot, sigma_trans, frame_time, None, None, model, sigma_rot0, sigma_trans0)
        sp.check_lengths(self.ds.num_frames)
        qt = np.ascontiguousarray(query_time, dtype=np.float64).reshape(-1)
        Q = len(qt)
        start, step = np.zeros((max(Q, 1), 6)), np.zeros((max(Q, 1), 6))
        _check(lib().aar_track_smooth_query2_step(self.handle, _dptr(x), C.byref(sp.c), Q, _dptr(qt) if Q else None, _dptr(start), _dptr(step)))
        return start[:Q], step[:Q]

    def track_smooth_lag3(self, x_full, sigma_rot, sigma_trans, frame_time=None, model="cv", sigma_rot0=0.0, sigma_trans0=0.0):
        """aar_track_smooth_lag3 (constant velocity, for checking): lag3_cov [F-3, 6, 6] = (H^-1)_{f,f+3}, UNSCALED"""
        x = self._x(x_full)
        F = self.ds.num_frames
        sp = SmoothParams(sigma_rot, sigma_trans, frame_time, None, None, model, sigma_rot0, sigma_trans0)
        sp.check_lengths(F)
        l3 = np.zeros((max(F - 3, 1), 6, 6))
        _check(lib().aar_track_smooth_lag3(self.handle, _dptr(x), C.byref(sp.c), _dptr(l3)))
        return l3[:max(F - 3, 0)]

    def track_smooth_relative(self, x_full, sigma_rot, sigma_trans, pairs, frame_time=None, rel_motion=None, model=None, sigma_rot0=0.0,
                              sigma_trans0=0.0, cross=True, motion=True, covariance=True):
        """aar_track_smooth_relative, either model: the covariance between any two frames and the relative motion between them.  pairs [Q, 2] =
        (a, b), any order, duplicates allowed.  Returns (cross_cov [Q, 6, 6] = (H^-1)_ab with the rows of frame a, rel [Q, 6] =
        [log(R_a^T R_b); t_b - t_a], rel_cov [Q, 6, 6], report dict); the covariances UNSCALED -- multiply by report["sigma2"].  A velocity over
        the baseline is rel / (t_b - t_a) with rel_cov / (t_b - t_a)^2.  cross / motion / covariance = False pass NULL for that output and
        return None in its place."""
        x = self._x(x_full)
        sp = SmoothParams(sigma_rot, sigma_trans, frame_time, rel_motion, None, model, sigma_rot0, sigma_trans0)
        sp.check_lengths(self.ds.num_frames)
        fa, fb = _pairs(pairs)
        Q = len(fa)
        cc = np.zeros((max(Q, 1), 6, 6)) if cross else None
        rel = np.zeros((max(Q, 1), 6)) if motion else None
        rc = np.zeros((max(Q, 1), 6, 6)) if covariance else None
        rep = CSmoothRelativeReport()
        rep.struct_size = C.sizeof(CSmoothRelativeReport)
        ip = C.POINTER(C.c_int32)
        _check(lib().aar_track_smooth_relative(self.handle, _dptr(x), C.byref(sp.c), Q, fa.ctypes.data_as(ip) if Q else None,
                                               fb.ctypes.data_as(ip) if Q else None, _dptr(cc) if cross else None, _dptr(rel) if motion else None,
                                               _dptr(rc) if covariance else None, C.byref(rep)))
        report = {k: getattr(rep, k) for k, _ in CSmoothRelativeReport._fields_ if k != "struct_size"}
        return cc[:Q] if cross else None, rel[:Q] if motion else None, rc[:Q] if covariance else None, report

    def track_smooth_detection_leverage(self, x_full, sigma_rot, sigma_trans, frame_time=None, rel_motion=None, model=None, sigma_rot0=0.0,
                                        sigma_trans0=0.0, rows=False):
        """aar_track_smooth_detection_leverage, either model: (leverage [local_obs] = tr(C_i) with C_i = G_i (H^-1)_ff G_i^T of the smoothed
        track, row_leverage [local_obs, 8] = diag(C_i) or None, report dict).  UNSCALED, reference detection order."""
        x, _, sp, rep = self._smooth_call(x_full, (sigma_rot, sigma_trans, frame_time, rel_motion, None, model, sigma_rot0, sigma_trans0),
                                          CSmoothPredictReport)
        n = self.local_obs
        lv = np.full(max(n, 1), np.nan)
        rw = np.full((max(n, 1), 8), np.nan) if rows else None
        _check(lib().aar_track_smooth_detection_leverage(self.handle, _dptr(x), C.byref(sp.c), _dptr(lv), _dptr(rw) if rows else None, C.byref(rep)))
        return lv[:n], (rw[:n] if rows else None), self._report(rep)

    def track_smooth_detection_loo(self, x_full, sigma_rot, sigma_trans, frame_time=None, rel_motion=None, model=None, sigma_rot0=0.0,
                                   sigma_trans0=0.0, f_max=None):
        """aar_track_smooth_detection_loo, either model, with the rule F > f_max when f_max is given.  Returns a DetectionLoo: loo_resid
        [local_obs, 8], q, F, cook, leverage, margin [local_obs], status, keep [local_obs] (uint8) and report: the aar_smooth_loo_report
        fields as a dict.  q is UNSCALED: q / report["sigma2"] is the chi-square."""
        x, _, sp, rep = self._smooth_call(x_full, (sigma_rot, sigma_trans, frame_time, rel_motion, None, model, sigma_rot0, sigma_trans0),
                                          CSmoothLooReport)
        n = self.local_obs
        m = max(n, 1)
        w = np.full((m, 8), np.nan)
        q, F, cook, lev, margin = (np.full(m, np.nan) for _ in range(5))
        st, keep = np.zeros(m, dtype=np.uint8), np.ones(m, dtype=np.uint8)
        rule = None
        if f_max is not None:
            rule = CLooRule()
            rule.struct_size = C.sizeof(CLooRule)
            rule.f_max = float(f_max)
        _check(lib().aar_track_smooth_detection_loo(self.handle, _dptr(x), C.byref(sp.c), C.byref(rule) if rule is not None else None, _dptr(w),
                                                    _dptr(q), _dptr(F), _dptr(cook), _dptr(lev), _dptr(margin), _u8ptr(st), _u8ptr(keep),
                                                    C.byref(rep)))
        return DetectionLoo(loo_resid=w[:n], q=q[:n], F=F[:n], cook=cook[:n], leverage=lev[:n], margin=margin[:n], status=st[:n], keep=keep[:n],
                            report=self._report(rep))

    @staticmethod
    def _time_queries(cams, markers, times):
        qc = np.ascontiguousarray(np.asarray(cams, dtype=np.int64).reshape(-1), dtype=np.int32)
        qm = np.ascontiguousarray(np.asarray(markers, dtype=np.int64).reshape(-1), dtype=np.int32)
        qt = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        if not len(qc) == len(qm) == len(qt):
            raise ValueError("time queries: %d cameras, %d markers, %d times" % (len(qc), len(qm), len(qt)))
        return qc, qm, qt

    def track_smooth_predict_corners(self, x_full, sigma_rot, sigma_trans, cams, markers, times, frame_time=None, model=None, sigma_rot0=0.0,
                                     sigma_trans0=0.0, covariance=True):
        """aar_track_smooth_predict_corners, either model: the corners of (camera index, marker index) at the smoothed track's pose at a
        TIME.  Returns (uv [Q, 4, 2], cov [Q, 8, 8] UNSCALED or None with covariance=False, status [Q], segment [Q], report dict).  A
        corner's covariance is report["sigma2"] * cov; the search window of a new detection is report["sigma2"] * (cov + I)."""
        x, _, sp, rep = self._smooth_call(x_full, (sigma_rot, sigma_trans, frame_time, None, None, model, sigma_rot0, sigma_trans0),
                                          CSmoothPredictReport)
        qc, qm, qt = self._time_queries(cams, markers, times)
        n = len(qc)
        uv = np.full((max(n, 1), 8), np.nan)
        cov = np.full((max(n, 1), 64), np.nan) if covariance else None
        st, seg = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.int32)
        _check(lib().aar_track_smooth_predict_corners(self.handle, _dptr(x), C.byref(sp.c), n, _i32ptr(qc), _i32ptr(qm), _dptr(qt) if n else None,
                                                      _dptr(uv), _dptr(cov) if covariance else None, _u8ptr(st),
                                                      seg.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(rep)))
        return uv[:n].reshape(n, 4, 2), (cov[:n].reshape(n, 8, 8) if covariance else None), st[:n], seg[:n], self._report(rep)

    def track_smooth_gate_detections(self, x_full, sigma_rot, sigma_trans, cams, markers, times, uv_obs, frame_time=None, model=None,
                                     sigma_rot0=0.0, sigma_trans0=0.0):
        """aar_track_smooth_gate_detections, either model: candidate detections (camera index, marker index, time) with observed corners
        uv_obs [Q, 4, 2] or [Q, 8] (stored as float32).  Returns (innovation [Q, 8] = uv_obs - predicted, m2 [Q] = e^T (I + C)^-1 e UNSCALED
        -- m2 / report["sigma2"] is chi-square with 8 degrees of freedom --, status [Q], segment [Q], report dict)."""
        x, _, sp, rep = self._smooth_call(x_full, (sigma_rot, sigma_trans, frame_time, None, None, model, sigma_rot0, sigma_trans0),
                                          CSmoothPredictReport)
        qc, qm, qt = self._time_queries(cams, markers, times)
        n = len(qc)
        uv = np.ascontiguousarray(np.asarray(uv_obs, dtype=np.float32).reshape(-1, 8))
        if len(uv) != n:
            raise ValueError("track_smooth_gate_detections: %d queries, %d sets of corners" % (n, len(uv)))
        inn = np.full((max(n, 1), 8), np.nan)
        m2 = np.full(max(n, 1), np.nan)
        st, seg = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.int32)
        _check(lib().aar_track_smooth_gate_detections(self.handle, _dptr(x), C.byref(sp.c), n, _i32ptr(qc), _i32ptr(qm), _dptr(qt) if n else None,
                                                      uv.ctypes.data_as(C.POINTER(C.c_float)) if n else None, _dptr(inn), _dptr(m2), _u8ptr(st),
                                                      seg.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(rep)))
        return inn[:n], m2[:n], st[:n], seg[:n], self._report(rep)

    def set_step_callback(self, fn, want_z=True):
        """SparseLevMarq::setStepCallBackFunc: fn(z) after every step (z = numpy copy of curr_z, or None when want_z is False)."""
        if fn is None:
            self._step_cb = None
            _check(lib().aar_lm_set_step_callback(self.handle, C.cast(None, STEP_CB), None, 0))
            return
        def tramp(ctx, zp, n):
            fn(np.ctypeslib.as_array(zp, shape=(n,)).copy() if zp else None)
        self._step_cb = STEP_CB(tramp)          # keep the trampoline alive
        _check(lib().aar_lm_set_step_callback(self.handle, self._step_cb, None, int(want_z)))

    def set_stop_function(self, fn):
        """SparseLevMarq::setStopFunction: fn(z) -> True stops the loop (no iteration cap while it is set)."""
        if fn is None:
            self._stop_fn = None
            _check(lib().aar_lm_set_stop_function(self.handle, C.cast(None, STOP_FN), None))
            return
        def tramp(ctx, zp, n):
            return 1 if fn(np.ctypeslib.as_array(zp, shape=(n,)).copy()) else 0
        self._stop_fn = STOP_FN(tramp)
        _check(lib().aar_lm_set_stop_function(self.handle, self._stop_fn, None))

    def extract_z(self, x_full):
        x = self._x(x_full)
        z = np.zeros(self.num_vars)
        _check(lib().aar_problem_extract_z(self.handle, _dptr(x), _dptr(z)))
        return z

    def set_huber_delta(self, delta):
        _check(lib().aar_problem_set_huber_delta(self.handle, float(delta)))

    def get_huber_delta(self):
        return float(lib().aar_problem_get_huber_delta(self.handle))

    def set_kernel_profiling(self, on):
        _check(lib().aar_set_kernel_profiling(self.handle, int(on)))

    def kernel_times(self):
        """{kernel name: (total seconds, launches)} accumulated since profiling was switched on."""
        sec = np.zeros(NUM_KERNELS)
        cnt = np.zeros(NUM_KERNELS, dtype=np.int64)
        _check(lib().aar_get_kernel_times(self.handle, _dptr(sec), cnt.ctypes.data_as(C.POINTER(C.c_int64))))
        return {lib().aar_kernel_name(i).decode(): (float(sec[i]), int(cnt[i])) for i in range(NUM_KERNELS)}

    def pcg_iterations(self):
        """(CG iterations of the last damped solve, running total) of the pcg / spcg solvers; zeros for direct"""
        out = (C.c_int32 * 2)()
        _check(lib().aar_problem_pcg_iterations(self.handle, out))
        return int(out[0]), int(out[1])

    def solver_stats(self):
        """aar_problem_get_solver_stats: the solver the problem runs with (AUTO resolved) and what its inner CG has done so far"""
        st = CSolverStats()
        st.struct_size = C.sizeof(CSolverStats)
        _check(lib().aar_problem_get_solver_stats(self.handle, C.byref(st)))
        return dict(solver=SOLVER_NAMES[st.solver], deterministic=bool(st.deterministic), last_iterations=st.last_iterations,
                    total_iterations=st.total_iterations, solves=st.solves, fallbacks=st.fallbacks, pcg_eta=st.pcg_eta, pcg_max_it=st.pcg_max_it,
                    same_xcd_solves=st.same_xcd_solves, pcg_eta_loose=st.pcg_eta_loose, pcg_eta_switch=st.pcg_eta_switch, pcg_abs_tol=st.pcg_abs_tol, env_overrides=st.env_overrides)

    def set_test_hook(self, hook, value):
        """aar_problem_set_test_hook (testing only): fault injection for the solvers' fall-back paths"""
        _check(lib().aar_problem_set_test_hook(self.handle, int(hook), int(value)))

    def set_stage_timers(self, on):
        _check(lib().aar_set_stage_timers(self.handle, int(on)))

    def stage_times(self):
        t = CStageTimes()
        _check(lib().aar_get_stage_times(self.handle, C.byref(t)))
        return {n: getattr(t, n) for n, _ in CStageTimes._fields_}
