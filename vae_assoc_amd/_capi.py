"""ctypes binding of libavae.so (C ABI declared in include/avae.h).

There is no CPU fallback: if the HIP library is missing or cannot be loaded, importing a
symbol from here raises.  ``import torch`` happens first on purpose: the PyTorch-ROCm wheel
bundles its own libamdhip64.so.7, and loading it first makes libavae (linked against the same
soname) resolve to that single HIP runtime, so device pointers of torch tensors are valid
inside the library.
"""
import ctypes as C
import os
import threading

import torch  # noqa: F401  (must precede the CDLL below, see module docstring)

AVAE_ABI_VERSION = 4
AVAE_MAX_MODALITIES = 4
AVAE_MAX_HIDDEN = 8
AVAE_MAX_WORLD = 8
AVAE_IPC_HANDLE_BYTES = 128
COMM_NONE, COMM_RCCL, COMM_IPC = 0, 1, 2
SCORE_CROSS = 1
METRIC_SYMKL, METRIC_L2 = 0, 1
METRIC_IDS = {"symkl": METRIC_SYMKL, "l2": METRIC_L2}
TOPK_MAX = 64
GMM_MAX_COMPONENTS = 64
EMBED_MAX_ROWS = 65536
MOTION_MAX_DOF, MOTION_MAX_KB, MOTION_MAX_POINTS, MOTION_MAX_ANCHORS = 16, 64, 1024, 4
RENDER_MAX_SIZE, RENDER_SUPERSAMPLES = 64, (1, 2, 4, 8)
IK_MAX_ITERS = 1000
LOGNORMAL_MAX_COMPONENTS, LOGNORMAL_MAX_POINTS, LOGNORMAL_MAX_ITERS = 16, 1024, 10000
TRACK_MAX_ITERS = 1000
THUMB_MAX_FRAME, THUMB_MAX_SIZE, THUMB_INVERT, THUMB_BGR = 4096, 64, 1, 2

ACT_IDS = {"identity": 0, "relu": 1, "softplus": 2, "sigmoid": 3, "tanh": 4}
DTYPE_IDS = {"fp32": 0, "f32": 0, "float32": 0, "bf16": 1, "bfloat16": 1}

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libavae.so")

# every symbol include/avae.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "avae_workspace_bytes", "avae_create", "avae_destroy", "avae_last_error", "avae_param_count",
    "avae_get_params", "avae_set_params", "avae_get_grads", "avae_get_opt_state", "avae_set_opt_state",
    "avae_train_step", "avae_train_steps", "avae_stage_batches", "avae_grad_buffer", "avae_cost_history",
    "avae_dp_plan", "avae_dp_backward", "avae_dp_apply", "avae_comm_unique_id", "avae_comm_ipc_handle", "avae_comm_ipc_attach",
    "avae_eval_cost", "avae_encode", "avae_decode", "avae_generate", "avae_reconstruct", "avae_save", "avae_load",
    "avae_score_width", "avae_score", "avae_loglik", "avae_score_masked", "avae_loglik_masked", "avae_train_steps_masked", "avae_eval_cost_masked", "avae_complete", "avae_impute",
    "avae_set_corruption", "avae_train_steps_in", "avae_eval_cost_in", "avae_stage_batches_in",
    "avae_set_grad_clip", "avae_grad_norm_history",
    "avae_set_schedule", "avae_schedule_value", "avae_hyper_history",
    "avae_set_ema", "avae_get_ema", "avae_set_ema_params", "avae_use_averaged",
    "avae_latent_topk", "avae_latent_topk_plan",
    "avae_latent_stats", "avae_latent_stats_plan",
    "avae_agg_logpdf", "avae_agg_logpdf_plan",
    "avae_gmm_fit", "avae_gmm_score", "avae_gmm_plan",
    "avae_embed_calibrate", "avae_embed_iterate", "avae_embed_plan",
    "avae_motion_eval", "avae_motion_fit", "avae_motion_moments",
    "avae_motion_fk", "avae_stroke_render",
    "avae_stroke_render_vjp", "avae_motion_fk_vjp", "avae_motion_eval_vjp", "avae_rows_adam",
    "avae_letter_thumbnail", "avae_letter_thumbnail_plan",
    "avae_motion_pose", "avae_motion_ik", "avae_motion_dynamics",
    "avae_lognormal_eval", "avae_lognormal_sample", "avae_lognormal_fit",
    "avae_motion_track", "avae_motion_track_plan",
    "avae_search_sample", "avae_search_update",
    "avae_synchronize", "avae_timing_enable", "avae_timing_report", "avae_debug_fetch", "avae_comm_allreduce",
]


class Modality(C.Structure):
    _fields_ = [("n_input", C.c_int32), ("n_hidden_layers", C.c_int32),
                ("n_hidden", C.c_int32 * AVAE_MAX_HIDDEN), ("binary", C.c_int32),
                ("weight", C.c_float), ("hidden_conv", C.c_int32), ("conv_gener", C.c_int32 * 2),
                ("reserved", C.c_int32)]


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("n_modalities", C.c_int32),
                ("mod", Modality * AVAE_MAX_MODALITIES),
                ("n_z", C.c_int32), ("batch_size", C.c_int32), ("batch_global", C.c_int32),
                ("row_offset", C.c_int32), ("activation", C.c_int32), ("compute_dtype", C.c_int32),
                ("device", C.c_int32), ("use_graph", C.c_int32),
                ("assoc_lambda", C.c_float), ("learning_rate", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("adam_eps", C.c_float),
                ("seed", C.c_uint64), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("use_comm", C.c_int32), ("world_size", C.c_int32), ("rank", C.c_int32), ("comm_buckets", C.c_int32),
                ("nccl_id", C.c_uint8 * 128), ("wire_dtype", C.c_int32), ("reserved2", C.c_int32 * 3)]


class Corruption(C.Structure):
    _fields_ = [("drop_prob", C.c_float * AVAE_MAX_MODALITIES), ("drop_value", C.c_float * AVAE_MAX_MODALITIES),
                ("noise_std", C.c_float * AVAE_MAX_MODALITIES)]


SCHED_NONE, SCHED_PIECEWISE, SCHED_EXP = 0, 1, 2
SCHED_MAX_KNOTS = 8


class Schedule(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_knots", C.c_int32), ("period", C.c_int64),
                ("knot_step", C.c_int64 * SCHED_MAX_KNOTS), ("knot_value", C.c_float * SCHED_MAX_KNOTS),
                ("decay_rate", C.c_float), ("staircase", C.c_int32), ("decay_steps", C.c_int64)]


class LatentStatsOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("count", "mean", "var", "xcov", "assoc", "post_var", "kl", "cov")]


SEARCH_MAX_DIMS, SEARCH_MAX_ROLLOUTS, SEARCH_MAX_GROUP = 1024, 1024, 64
ROWS_ADAM_MAX_DIMS = 1024
SEARCH_IDS = {"PI-BB": 0, "CEM": 1, "CMA-ES": 2}


class SearchOptions(C.Structure):
    _fields_ = [("weighting", C.c_int32), ("cov_update", C.c_int32), ("eliteness", C.c_double), ("learning_rate", C.c_double),
                ("rel_lower", C.c_double), ("abs_lower", C.c_double), ("abs_upper", C.c_double), ("tol", C.c_double)]


_lib = None
_lock = threading.Lock()


def lib():
    """The loaded library; raises (never falls back) when it is absent."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    "libavae.so is missing (%s): build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "-- vae_assoc_amd has no CPU fallback" % LIB_PATH)
            L = C.CDLL(LIB_PATH)
            fp, vp, i32, sz = C.POINTER(C.c_float), C.c_void_p, C.c_int32, C.c_size_t
            L.avae_workspace_bytes.argtypes = [C.POINTER(Config), C.POINTER(sz)]
            L.avae_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
            L.avae_destroy.argtypes = [vp]
            L.avae_destroy.restype = None
            L.avae_last_error.argtypes = [vp]
            L.avae_last_error.restype = C.c_char_p
            L.avae_param_count.argtypes = [vp, C.POINTER(sz)]
            L.avae_get_params.argtypes = [vp, vp]
            L.avae_set_params.argtypes = [vp, vp]
            L.avae_get_grads.argtypes = [vp, vp]
            L.avae_get_opt_state.argtypes = [vp, vp, vp, C.POINTER(C.c_int64)]
            L.avae_set_opt_state.argtypes = [vp, vp, vp, C.c_int64]
            L.avae_train_step.argtypes = [vp, C.POINTER(vp), C.POINTER(i32), vp, fp, vp]
            L.avae_train_steps.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), vp, fp, vp]
            L.avae_stage_batches.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), vp, vp]
            L.avae_grad_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
            L.avae_cost_history.argtypes = [vp, i32, vp, C.POINTER(C.c_int64)]
            L.avae_dp_plan.argtypes = [C.POINTER(Config), C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
            L.avae_dp_backward.argtypes = [vp, i32, i32, vp]
            L.avae_dp_apply.argtypes = [vp, i32, fp, vp]
            L.avae_comm_unique_id.argtypes = [vp]
            L.avae_comm_ipc_handle.argtypes = [vp, vp]
            L.avae_comm_ipc_attach.argtypes = [vp, vp]
            L.avae_eval_cost.argtypes = [vp, C.POINTER(vp), C.POINTER(i32), vp, fp, vp]
            L.avae_train_steps_masked.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), vp, vp, fp, vp]
            L.avae_eval_cost_masked.argtypes = [vp, C.POINTER(vp), C.POINTER(i32), vp, vp, fp, vp]
            L.avae_set_corruption.argtypes = [vp, C.POINTER(Corruption)]
            L.avae_train_steps_in.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(vp), C.POINTER(i32), vp, vp, fp, vp]
            L.avae_eval_cost_in.argtypes = [vp, C.POINTER(vp), C.POINTER(i32), C.POINTER(vp), C.POINTER(i32), vp, vp, fp, vp]
            L.avae_stage_batches_in.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(vp), C.POINTER(i32), vp, vp]
            L.avae_set_grad_clip.argtypes = [vp, C.c_float, i32]
            L.avae_grad_norm_history.argtypes = [vp, i32, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
            L.avae_set_schedule.argtypes = [vp, C.POINTER(Schedule), C.POINTER(Schedule), C.POINTER(Schedule)]
            L.avae_schedule_value.argtypes = [C.POINTER(Schedule), C.c_int64, fp]
            L.avae_hyper_history.argtypes = [vp, i32, vp, C.POINTER(C.c_int64)]
            L.avae_set_ema.argtypes = [vp, C.c_float, i32]
            L.avae_get_ema.argtypes = [vp, vp]
            L.avae_set_ema_params.argtypes = [vp, vp]
            L.avae_use_averaged.argtypes = [vp, i32]
            L.avae_encode.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp]
            L.avae_decode.argtypes = [vp, i32, vp, i32, vp, vp]
            L.avae_generate.argtypes = [vp, vp, i32, C.POINTER(vp), vp]
            L.avae_reconstruct.argtypes = [vp, i32, vp, i32, vp, i32, vp, vp]
            L.avae_score_width.argtypes = [C.POINTER(Config), i32, C.POINTER(i32)]
            L.avae_score.argtypes = [vp, C.POINTER(vp), C.POINTER(i32), i32, vp, i32, vp, vp]
            L.avae_loglik.argtypes = [vp, C.POINTER(vp), C.POINTER(i32), i32, i32, vp, vp, vp]
            L.avae_score_masked.argtypes = [vp, C.POINTER(vp), C.POINTER(i32), vp, i32, vp, i32, vp, vp]
            L.avae_loglik_masked.argtypes = [vp, C.POINTER(vp), C.POINTER(i32), vp, i32, i32, vp, vp, vp]
            L.avae_complete.argtypes = [vp, C.POINTER(vp), C.POINTER(i32), C.POINTER(vp), vp, i32, i32, C.c_float, C.c_float,
                                        vp, vp, vp, C.POINTER(vp), vp]
            L.avae_impute.argtypes = [vp, C.POINTER(vp), C.POINTER(i32), vp, i32, i32, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), vp]
            L.avae_latent_topk.argtypes = [vp, vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp]
            L.avae_latent_topk_plan.argtypes = [C.POINTER(Config), i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32),
                                                C.POINTER(sz)]
            L.avae_latent_stats.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), vp, i32, C.POINTER(LatentStatsOut), vp]
            L.avae_latent_stats_plan.argtypes = [C.POINTER(Config), i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(sz)]
            L.avae_agg_logpdf.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp]
            L.avae_agg_logpdf_plan.argtypes = [C.POINTER(Config), i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32),
                                               C.POINTER(i32), C.POINTER(sz)]
            L.avae_gmm_fit.argtypes = [vp, vp, vp, i32, i32, i32, C.c_float, vp, vp, vp, vp, vp, vp]
            L.avae_gmm_score.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
            L.avae_gmm_plan.argtypes = [C.POINTER(Config), i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(sz)]
            L.avae_embed_calibrate.argtypes = [vp, vp, vp, i32, i32, C.c_double, C.c_double, i32, vp, vp, vp, vp, vp, vp]
            L.avae_embed_iterate.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, C.c_float, C.c_float, i32,
                                             C.c_float, C.c_float, i32, vp, vp, vp]
            L.avae_embed_plan.argtypes = [C.POINTER(Config), i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(sz)]
            L.avae_motion_eval.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
            L.avae_motion_fit.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
            L.avae_motion_moments.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
            L.avae_motion_fk.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp]
            L.avae_stroke_render.argtypes = [vp, vp, i32, i32, vp, C.c_float, C.c_float, i32, i32, vp, vp, vp, vp, vp, vp, vp]
            L.avae_stroke_render_vjp.argtypes = [vp, vp, i32, i32, vp, C.c_float, C.c_float, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                 vp, vp]
            L.avae_motion_fk_vjp.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
            L.avae_motion_eval_vjp.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
            L.avae_rows_adam.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                         vp, vp, vp, vp]
            L.avae_letter_thumbnail_plan.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(sz)]
            L.avae_letter_thumbnail.argtypes = [vp, vp, i32, i32, i32, i32, C.c_int64, C.c_int64, i32, i32, i32, vp, sz, vp, vp, vp, vp, vp]
            L.avae_motion_pose.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]
            L.avae_motion_ik.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, i32, C.c_float, C.c_float, C.c_float,
                                         C.c_float, vp, vp, vp, vp, vp, vp]
            L.avae_motion_dynamics.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, C.POINTER(C.c_float), vp, vp, vp, vp, vp]
            L.avae_lognormal_eval.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_float, vp, vp, vp]
            L.avae_lognormal_sample.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, C.c_float, C.c_uint64, C.c_int64, C.c_float,
                                                C.c_float, C.c_float, i32, vp, vp, vp]
            L.avae_lognormal_fit.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, C.c_float, i32, C.c_double, C.c_double, C.c_double,
                                             vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
            L.avae_motion_track_plan.argtypes = [i32, i32, i32, C.POINTER(sz)]
            L.avae_motion_track.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, C.c_float, C.POINTER(C.c_float), C.c_float, vp, vp,
                                            C.c_float, i32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, vp, sz,
                                            vp, vp, vp, vp, vp, vp, vp, vp, vp]
            L.avae_search_sample.argtypes =[vp, vp, vp, i32, i32, i32, C.c_uint64, i32, C.c_int64, vp, vp, i32, i32, vp, vp]
            L.avae_search_update.argtypes = [vp, vp, vp, i32, i32, i32, C.POINTER(SearchOptions), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
            L.avae_save.argtypes = [vp, C.c_char_p]
            L.avae_load.argtypes = [vp, C.c_char_p]
            L.avae_synchronize.argtypes = [vp]
            L.avae_timing_enable.argtypes = [vp, i32]
            L.avae_timing_report.argtypes = [vp, C.c_char_p, sz]
            L.avae_debug_fetch.argtypes = [vp, C.c_char_p, vp, sz, C.POINTER(sz)]
            L.avae_comm_allreduce.argtypes = [vp, i32, vp]
            for name in SYMBOLS:
                if name not in ("avae_destroy", "avae_last_error"):
                    getattr(L, name).restype = C.c_int
            _lib = L
        return _lib


def check(handle, rc, what):
    if rc != 0:
        msg = lib().avae_last_error(handle)
        raise RuntimeError("%s failed (%d): %s" % (what, rc, msg.decode("utf-8", "replace") if msg else "?"))
