"""ctypes binding of include/cpprob_hip.h (harness for tests and bench; not a compute path)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libcpprob_hip.so")

ALG_SIS, ALG_SMC = 2, 4
MODEL_GAUSSIAN_UNKNOWN_MEAN, MODEL_GAUSSIAN_README, MODEL_LINEAR_GAUSSIAN_1D, MODEL_HMM3, MODEL_GAUSSIAN_2D_UNKNOWN_MEAN, MODEL_HMM_TABLE = 0, 1, 2, 3, 4, 5
RESAMPLE_SYSTEMATIC, RESAMPLE_STRATIFIED, RESAMPLE_MULTINOMIAL = 0, 1, 2
SCOPE_GLOBAL, SCOPE_ISLAND, SCOPE_EXCHANGE = 0, 1, 2
VARIATE_SMALLINT, VARIATE_DISCRETE, VARIATE_UNIFORM_REAL, VARIATE_POISSON, VARIATE_NORMAL = 0, 1, 2, 3, 4   # cpprob_hip_variate_from_bits
POISSON_MAX_MEAN = 1.0e4                      # CPPROB_HIP_POISSON_MAX_MEAN: draw_poisson refuses a larger mean
# cpprob_hip_config::flags (A/B forms; 0 = the measured optimum)
FLAG_FLOATING_POINT_STEP, FLAG_NO_SKIP_ROWS, FLAG_SIS_PER_TILE, FLAG_SIS_SEPARATE_READOUT, FLAG_WREL_STORED, FLAG_FP_TILE_PARTIALS, FLAG_WALK_READOUT = 1, 2, 4, 8, 16, 32, 64
FLAG_MULTINOMIAL_LITERAL, FLAG_REPEAT_IN_FLOATING_POINT, FLAG_PAIRED_STEP_LAUNCH = 128, 256, 512
FLAG_SEPARATE_TRACE_READOUT = 1024      # the trace-word / filtering-only read-out as a launch after the last step, not folded into it
FLAG_SERIAL_RUNS = 2048                 # run lanes off: every run of the context on its one stream (A/B of cpprob_hip_infer_lanes)
SERIAL_STREAM, SERIAL_PROFILE, SERIAL_SHARD, SERIAL_FLAG, SERIAL_MEMORY, SERIAL_SIZE = 1, 2, 3, 4, 5, 6      # cpprob_hip_infer_lanes: serial_reason
N_KERNEL_CLASSES = 6
KERNEL_CLASS_NAMES = ["smc_step", "scan_partials", "smooth", "finalize", "sis", "resample"]

# every symbol include/cpprob_hip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "cpprob_hip_abi_version", "cpprob_hip_build_id", "cpprob_hip_device_count", "cpprob_hip_create", "cpprob_hip_destroy", "cpprob_hip_last_error",
    "cpprob_hip_stream", "cpprob_hip_sync", "cpprob_hip_set_hmm", "cpprob_hip_infer_begin", "cpprob_hip_infer_run", "cpprob_hip_infer_lanes", "cpprob_hip_infer_summary",
    "cpprob_hip_infer_stats", "cpprob_hip_infer_results", "cpprob_hip_infer_results_device", "cpprob_hip_infer_step_trace", "cpprob_hip_copy_values", "cpprob_hip_copy_ancestors",
    "cpprob_hip_copy_logw", "cpprob_hip_copy_paths", "cpprob_hip_smc_step_begin", "cpprob_hip_smc_step_end",
    "cpprob_hip_smc_finish", "cpprob_hip_smc_first_bad_generation", "cpprob_hip_smc_repair_begin", "cpprob_hip_smc_repair_end", "cpprob_hip_filter_masses", "cpprob_hip_exchange_plan", "cpprob_hip_exchange_pack", "cpprob_hip_exchange_commit", "cpprob_hip_exchange_setup", "cpprob_hip_exchange_transport",
    "cpprob_hip_exchange_pack_async", "cpprob_hip_exchange_commit_async", "cpprob_hip_exchange_status", "cpprob_hip_exchange_direct", "cpprob_hip_exchange_traffic", "cpprob_hip_exchange_store", "cpprob_hip_exchange_remote",
    "cpprob_hip_group_create_external", "cpprob_hip_group_traffic", "cpprob_hip_group_profile", "cpprob_hip_group_profile_read", "cpprob_hip_group_note", "cpprob_hip_group_unique_id", "cpprob_hip_group_create", "cpprob_hip_group_destroy",
    "cpprob_hip_group_last_error", "cpprob_hip_group_begin", "cpprob_hip_group_transport", "cpprob_hip_group_run", "cpprob_hip_group_sync", "cpprob_hip_group_size",
    "cpprob_hip_group_context", "cpprob_hip_group_results", "cpprob_hip_philox_blocks", "cpprob_hip_draw_normal", "cpprob_hip_draw_uniform_smallint",
    "cpprob_hip_draw_discrete", "cpprob_hip_draw_uniform_real", "cpprob_hip_draw_poisson", "cpprob_hip_logpdf_normal", "cpprob_hip_logpdf_uniform_real",
    "cpprob_hip_logpdf_poisson", "cpprob_hip_logpdf_uniform_smallint", "cpprob_hip_logpdf_discrete", "cpprob_hip_logsumexp_ess",
    "cpprob_hip_weighted_moments", "cpprob_hip_weighted_hist", "cpprob_hip_weighted_moments_columns", "cpprob_hip_weighted_hist_columns", "cpprob_hip_resample", "cpprob_hip_smc_bookkeep", "cpprob_hip_smc_bookkeep_fixed", "cpprob_hip_smc_bookkeep_fixed_rs", "cpprob_hip_generic_begin", "cpprob_hip_generic_begin_tiles", "cpprob_hip_generic_quantize", "cpprob_hip_generic_max", "cpprob_hip_generic_quantize_ref", "cpprob_hip_generic_totals", "cpprob_hip_generic_finish", "cpprob_hip_systematic_offset", "cpprob_hip_lineage_gather", "cpprob_hip_lineage_prepare", "cpprob_hip_readback_with_next_result", "cpprob_hip_lineage_moments", "cpprob_hip_lineage_hist", "cpprob_hip_gather_f64",
    "cpprob_hip_gather_i32", "cpprob_hip_profile_enable", "cpprob_hip_profile_read", "cpprob_hip_fastmath", "cpprob_hip_variate_from_bits",
    "cpprob_hip_batch_workspace_bytes", "cpprob_hip_batch_begin", "cpprob_hip_batch_run", "cpprob_hip_batch_results", "cpprob_hip_batch_results_device",
    "cpprob_hip_batch_copy_store", "cpprob_hip_batch_copy_masses", "cpprob_hip_batch_problems_workspace_bytes", "cpprob_hip_batch_begin_problems",
    "cpprob_hip_batch_online_workspace_bytes", "cpprob_hip_batch_begin_online", "cpprob_hip_batch_advance", "cpprob_hip_batch_lengths",
    "cpprob_hip_batch_paths_layout", "cpprob_hip_batch_paths", "cpprob_hip_batch_paths_device",
    "cpprob_hip_batch_smooth_layout", "cpprob_hip_batch_smooth", "cpprob_hip_batch_smooth_device",
    "cpprob_hip_batch_smooth_lag", "cpprob_hip_batch_smooth_lag_device", "cpprob_hip_batch_smooth_grid",
    "cpprob_hip_batch_smooth_stats", "cpprob_hip_batch_smooth_stats_device",
    "cpprob_hip_batch_online_stats", "cpprob_hip_batch_online_stats_device", "cpprob_hip_batch_online_stats_progress",
    "cpprob_hip_batch_traj_stats", "cpprob_hip_batch_traj_stats_device", "cpprob_hip_batch_traj_stats_grid",
    "cpprob_hip_batch_forecast", "cpprob_hip_batch_forecast_device", "cpprob_hip_batch_predictive", "cpprob_hip_batch_predictive_device",
    "cpprob_hip_batch_decode", "cpprob_hip_batch_decode_device", "cpprob_hip_batch_decode_lag", "cpprob_hip_batch_decode_lag_device",
    "cpprob_hip_batch_decode_logp", "cpprob_hip_batch_pass_grid",
    "cpprob_hip_batch_run_conditional", "cpprob_hip_batch_run_conditional_device",
    "cpprob_hip_batch_retable", "cpprob_hip_batch_retable_device", "cpprob_hip_batch_retable_status", "cpprob_hip_batch_retable_grid",
    "cpprob_hip_batch_mstep_device", "cpprob_hip_batch_copy_step_tables", "cpprob_hip_batch_summaries_device",
    "cpprob_hip_batch_learn_begin", "cpprob_hip_batch_advance_learn", "cpprob_hip_batch_advance_learn_device", "cpprob_hip_batch_online_tables",
    "cpprob_hip_batch_learn_tables", "cpprob_hip_batch_learn_tables_device", "cpprob_hip_batch_learn_record",
    "cpprob_hip_table_log", "cpprob_hip_batch_begin_problems_scaled", "cpprob_hip_batch_begin_online_scaled",
    "cpprob_hip_batch_retable_scaled", "cpprob_hip_batch_retable_scaled_device", "cpprob_hip_batch_mstep_scaled_device",
    "cpprob_hip_batch_online_tables_scaled", "cpprob_hip_batch_copy_scales",
    "cpprob_hip_batch_begin_problems_poisson", "cpprob_hip_batch_begin_online_poisson", "cpprob_hip_batch_retable_poisson",
    "cpprob_hip_batch_retable_poisson_device", "cpprob_hip_batch_mstep_poisson_device", "cpprob_hip_batch_online_tables_poisson",
    "cpprob_hip_batch_copy_rates",
    "cpprob_hip_batch_learn_begin_scaled", "cpprob_hip_batch_learn_tables_scaled", "cpprob_hip_batch_learn_tables_scaled_device",
    "cpprob_hip_batch_tie", "cpprob_hip_batch_tie_get", "cpprob_hip_batch_pool_stats", "cpprob_hip_batch_pool_stats_device",
    "cpprob_hip_batch_learn_tie", "cpprob_hip_batch_learn_pooled_record",
]


class CpprobHipError(RuntimeError):
    pass


EPRECISION = -5


class Config(C.Structure):
    _fields_ = [("algorithm", C.c_int32), ("model", C.c_int32), ("resampler", C.c_int32), ("resample_scope", C.c_int32),
                ("keep_history", C.c_int32), ("annex_kcols", C.c_int32), ("flags", C.c_uint32), ("fuse_max_tiles", C.c_int32),
                ("ess_threshold", C.c_double), ("seed", C.c_uint64), ("n_particles", C.c_uint64),
                ("particle_offset", C.c_uint64), ("n_global", C.c_uint64)]


class Summary(C.Structure):
    _fields_ = [("log_evidence", C.c_double), ("ess_final", C.c_double), ("log_norm", C.c_double), ("max_logw", C.c_double),
                ("n_predict", C.c_int32), ("stats_per_predict", C.c_int32), ("is_int", C.c_int32), ("n_resampled", C.c_int32),
                ("step_form", C.c_int32), ("n_requantised", C.c_int32)]


FORM_FLOAT, FORM_COUNTS, FORM_FIXED = 0, 1, 2


class BatchConfig(C.Structure):
    _fields_ = [("algorithm", C.c_int32), ("model", C.c_int32), ("resampler", C.c_int32), ("keep_history", C.c_int32),
                ("flags", C.c_uint32), ("ess_threshold", C.c_double), ("n_particles", C.c_uint64), ("n_problems", C.c_uint64)]


BATCH_MAX_PARTICLES = 8192
BATCH_KEEP_MASSES = 2                         # cpprob_hip_batch_config::flags: a filtering-only batch keeps the smoother's m table


def _batch_flags(flags, keep_masses):
    return int(flags) | (BATCH_KEEP_MASSES if keep_masses else 0)


def _poisson(emission, tables):
    """True for emission="poisson", whose tables are (rates [B, k], transition [B, k, k]); False for "normal"."""
    if emission not in ("normal", "poisson"):
        raise ValueError('emission is "normal" or "poisson"')
    if emission == "poisson" and (tables is None or len(tables) != 2 or tables[0] is None or tables[1] is None):
        raise ValueError('emission="poisson" takes tables = (rates [B, k], transition [B, k, k]): a batch is unit, scaled or Poisson')
    return emission == "poisson"


def batch_workspace_bytes(model, n_particles, n_problems, T, resampler=RESAMPLE_SYSTEMATIC, ess_threshold=2.0, keep_history=True, algorithm=ALG_SMC, flags=0,
                          keep_masses=False):
    """cpprob_hip_batch_workspace_bytes: validates a batch configuration and returns its device bytes; no GPU needed.  keep_masses
    (with keep_history=False): the batch keeps the backward smoother's m table, 64 bytes a problem and step."""
    L = load_library()
    cfg = BatchConfig(int(algorithm), int(model), int(resampler), 1 if keep_history else 0, _batch_flags(flags, keep_masses), float(ess_threshold), int(n_particles), int(n_problems))
    out = C.c_uint64()
    rc = L.cpprob_hip_batch_workspace_bytes(C.byref(cfg), int(T), C.byref(out))
    if rc:
        msg = L.cpprob_hip_last_error(None)
        e = CpprobHipError("cpprob_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
        e.code = rc
        raise e
    return out.value


def _problem_shapes(T, n_particles):
    """(h_T uint32 [B], h_n uint32 [B]) of a batch of problems; n_particles an int (every problem's) or one value a problem."""
    h_T = np.ascontiguousarray(T, np.uint32).reshape(-1)
    h_n = np.ascontiguousarray(n_particles, np.uint32).reshape(-1)
    if h_n.size == 1 and h_T.size != 1:
        h_n = np.full(h_T.size, h_n[0], np.uint32)
    if h_n.shape != h_T.shape:
        raise ValueError("one particle count per problem (or one for all)")
    return h_T, h_n


def batch_problems_workspace_bytes(model, T, n_particles, max_particles=None, resampler=RESAMPLE_SYSTEMATIC, ess_threshold=2.0, keep_history=True, algorithm=ALG_SMC, flags=0,
                                   keep_masses=False):
    """cpprob_hip_batch_problems_workspace_bytes: the device bytes of a batch whose problem b has T[b] observes and n_particles[b]
    particles (an int: every problem's); max_particles is cfg.n_particles (default: the largest of n_particles).  No GPU needed."""
    L = load_library()
    h_T, h_n = _problem_shapes(T, n_particles)
    top = int(h_n.max()) if (max_particles is None and h_n.size) else int(max_particles or 0)
    cfg = BatchConfig(int(algorithm), int(model), int(resampler), 1 if keep_history else 0, _batch_flags(flags, keep_masses), float(ess_threshold), top, int(h_T.size))
    out = C.c_uint64()
    rc = L.cpprob_hip_batch_problems_workspace_bytes(C.byref(cfg), h_T.ctypes.data_as(C.POINTER(C.c_uint32)), h_n.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(out))
    if rc:
        msg = L.cpprob_hip_last_error(None)
        e = CpprobHipError("cpprob_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
        e.code = rc
        raise e
    return out.value


def batch_online_workspace_bytes(model, capacity, n_particles, max_particles=None, resampler=RESAMPLE_SYSTEMATIC, ess_threshold=2.0, keep_history=True, algorithm=ALG_SMC, flags=0,
                                 keep_masses=False):
    """cpprob_hip_batch_online_workspace_bytes: the device bytes of a batch advanced in pieces, whose problem b may reach capacity[b]
    observes with n_particles[b] particles (an int: every problem's); max_particles is cfg.n_particles.  No GPU needed."""
    L = load_library()
    h_T, h_n = _problem_shapes(capacity, n_particles)
    top = int(h_n.max()) if (max_particles is None and h_n.size) else int(max_particles or 0)
    cfg = BatchConfig(int(algorithm), int(model), int(resampler), 1 if keep_history else 0, _batch_flags(flags, keep_masses), float(ess_threshold), top, int(h_T.size))
    out = C.c_uint64()
    rc = L.cpprob_hip_batch_online_workspace_bytes(C.byref(cfg), h_T.ctypes.data_as(C.POINTER(C.c_uint32)), h_n.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(out))
    if rc:
        msg = L.cpprob_hip_last_error(None)
        e = CpprobHipError("cpprob_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
        e.code = rc
        raise e
    return out.value


def batch_paths_layout(T, n, max_particles=0):
    """cpprob_hip_batch_paths_layout: where problem b's traces sit in the packed output of Engine.batch_paths /
    batch_paths_device.  T[b], n[b]: its length (0 allowed) and particle count (an int: every problem's).  Returns (first, wfirst),
    uint64 [B + 1]: problem b owns entries first[b]:first[b + 1] ([T_b, m_b], m_b = n_b or min(n_b, max_particles)) and weights
    wfirst[b]:wfirst[b + 1].  No GPU needed."""
    L = load_library()
    h_T, h_n = _problem_shapes(T, n)
    first = np.zeros(h_T.size + 1, np.uint64)
    wfirst = np.zeros(h_T.size + 1, np.uint64)
    rc = L.cpprob_hip_batch_paths_layout(h_T.ctypes.data_as(C.POINTER(C.c_uint32)), h_n.ctypes.data_as(C.POINTER(C.c_uint32)), int(h_T.size), int(max_particles),
                                         first.ctypes.data_as(C.POINTER(C.c_uint64)), wfirst.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc:
        msg = L.cpprob_hip_last_error(None)
        e = CpprobHipError("cpprob_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
        e.code = rc
        raise e
    return first, wfirst


def batch_smooth_layout(T, n_traj):
    """cpprob_hip_batch_smooth_layout: where problem b's backward trajectories sit in the packed output of Engine.batch_smooth /
    batch_smooth_device.  T[b]: its length (0 allowed).  Returns first, uint64 [B + 1]: problem b owns entries first[b]:first[b + 1]
    ([T_b, n_traj]).  No GPU needed."""
    L = load_library()
    h_T = np.ascontiguousarray(T, np.uint32).reshape(-1)
    first = np.zeros(h_T.size + 1, np.uint64)
    rc = L.cpprob_hip_batch_smooth_layout(h_T.ctypes.data_as(C.POINTER(C.c_uint32)), int(h_T.size), int(n_traj), first.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc:
        msg = L.cpprob_hip_last_error(None)
        e = CpprobHipError("cpprob_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
        e.code = rc
        raise e
    return first


FORECAST_MAX_HORIZON, FORECAST_MAX_TRAJ, FORECAST_MAX_DRAWS = 1 << 24, 1 << 20, 1 << 16      # cpprob_hip_batch_forecast: horizon <, n_traj <=, draw_index <
DECODE_MAX_LAG = 1 << 24                      # cpprob_hip_batch_decode_lag: lag <=
STATS_PER_PROBLEM = 88                        # doubles a problem of cpprob_hip_batch_smooth_stats: xi[8][8], occ[8], occ_y[8], occ_yy[8]


TRAJ_STATS_TILE = 256                         # trajectories a workgroup of cpprob_hip_batch_traj_stats: its grid holds ceil(n_traj / this) tiles a problem
TRAJ_STATS_MAX_TRAJ, TRAJ_STATS_MAX_DRAWS = 1 << 20, 1 << 16     # cpprob_hip_batch_traj_stats: n_traj in 1 ..=, draw_index <


def split_stats(rec):
    """The records [B, 88] of cpprob_hip_batch_smooth_stats as a dict of views: xi [B, 8, 8], occ, occ_y, occ_yy [B, 8]."""
    rec = np.asarray(rec).reshape(-1, STATS_PER_PROBLEM)
    return {"xi": rec[:, :64].reshape(-1, 8, 8), "occ": rec[:, 64:72], "occ_y": rec[:, 72:80], "occ_yy": rec[:, 80:88]}


def split_traj_stats(rec):
    """The records [B, n_traj, 88] of cpprob_hip_batch_traj_stats as a dict of views: xi [B, n_traj, 8, 8], occ, occ_y, occ_yy
    [B, n_traj, 8]."""
    rec = np.asarray(rec)
    B, M = rec.shape[0], rec.shape[1]
    return {"xi": rec[:, :, :64].reshape(B, M, 8, 8), "occ": rec[:, :, 64:72], "occ_y": rec[:, :, 72:80], "occ_yy": rec[:, :, 80:88]}


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)


class Collectives(C.Structure):
    _fields_ = [("user", C.c_void_p), ("allgather", ALLGATHER_FN)]


class Traffic(C.Structure):
    _fields_ = [("records", C.c_uint64), ("payload_bytes", C.c_uint64), ("wire_bytes", C.c_uint64), ("collective_bytes", C.c_uint64),
                ("transport", C.c_int32), ("remote_lineages", C.c_int32), ("mailbox_collectives", C.c_int32), ("reserved", C.c_int32)]


GROUP_SENDRECV, GROUP_WORLD1_COLLECTIVES, GROUP_SHIP_LINEAGES, GROUP_LIBRARY_COLLECTIVES, GROUP_MAILBOX_COLLECTIVES = 1, 2, 4, 8, 16
TRANSPORT_NONE, TRANSPORT_DIRECT, TRANSPORT_SENDRECV = 0, 1, 2

_lib = None


def load_library(path=None):
    """Loads libcpprob_hip.so.  Import torch first when both live in one process so that the
    already-loaded libamdhip64.so.7 (same SONAME) is shared."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("CPPROB_HIP_LIB") or LIB_PATH      # CPPROB_HIP_LIB: alternative build of the library (A/B runs)
    if not os.path.exists(p):
        raise CpprobHipError("%s is missing: run `python -m cpprob_amd.build` (there is no CPU fallback)" % p)
    L = C.CDLL(p, mode=C.RTLD_GLOBAL)
    vp, u64, i64, i32, dbl, sz = C.c_void_p, C.c_uint64, C.c_int64, C.c_int32, C.c_double, C.c_size_t
    sig = {
        "cpprob_hip_abi_version": (C.c_int, []),
        "cpprob_hip_build_id": (C.c_char_p, []),
        "cpprob_hip_device_count": (C.c_int, []),
        "cpprob_hip_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "cpprob_hip_destroy": (None, [vp]),
        "cpprob_hip_last_error": (C.c_char_p, [vp]),
        "cpprob_hip_stream": (vp, [vp]),
        "cpprob_hip_sync": (C.c_int, [vp]),
        "cpprob_hip_set_hmm": (C.c_int, [vp, i32, C.POINTER(dbl), C.POINTER(dbl)]),
        "cpprob_hip_infer_begin": (C.c_int, [vp, C.POINTER(Config), C.POINTER(dbl), sz]),
        "cpprob_hip_infer_run": (C.c_int, [vp, u64]),
        "cpprob_hip_infer_lanes": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(u64), C.POINTER(i32)]),
        "cpprob_hip_infer_summary": (C.c_int, [vp, C.POINTER(Summary)]),
        "cpprob_hip_infer_stats": (C.c_int, [vp, C.POINTER(dbl), sz]),
        "cpprob_hip_infer_results": (C.c_int, [vp, vp, vp, sz, vp, vp]),
        "cpprob_hip_infer_results_device": (C.c_int, [vp, vp, sz]),
        "cpprob_hip_infer_step_trace": (C.c_int, [vp, C.POINTER(dbl), C.POINTER(i32)]),
        "cpprob_hip_copy_values": (C.c_int, [vp, vp, sz]),
        "cpprob_hip_copy_ancestors": (C.c_int, [vp, vp, sz]),
        "cpprob_hip_copy_logw": (C.c_int, [vp, vp, sz]),
        "cpprob_hip_copy_paths": (C.c_int, [vp, vp, sz]),
        "cpprob_hip_smc_step_begin": (C.c_int, [vp, i32, u64, vp]),
        "cpprob_hip_smc_step_end": (C.c_int, [vp, i32, vp, i32, i32]),
        "cpprob_hip_smc_finish": (C.c_int, [vp]),
        "cpprob_hip_smc_first_bad_generation": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
        "cpprob_hip_smc_repair_begin": (C.c_int, [vp, C.c_int32, vp]),
        "cpprob_hip_smc_repair_end": (C.c_int, [vp, C.c_int32, vp, C.c_int32, C.c_int32, vp]),
        "cpprob_hip_filter_masses": (C.c_int, [vp, C.POINTER(vp), C.POINTER(i32)]),
        "cpprob_hip_exchange_plan": (C.c_int, [vp, i32, i32, i32, vp, vp, vp, C.POINTER(i32)]),
        "cpprob_hip_exchange_pack": (C.c_int, [vp, i32, vp]),
        "cpprob_hip_exchange_commit": (C.c_int, [vp, i32, vp]),
        "cpprob_hip_exchange_setup": (C.c_int, [vp, i32, i32, vp, i32, u64]),
        "cpprob_hip_exchange_transport": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), C.POINTER(u64), C.POINTER(u64)]),
        "cpprob_hip_exchange_pack_async": (C.c_int, [vp, i32]),
        "cpprob_hip_exchange_commit_async": (C.c_int, [vp, i32]),
        "cpprob_hip_exchange_status": (C.c_int, [vp, C.POINTER(i32), C.POINTER(u64)]),
        "cpprob_hip_group_unique_id": (C.c_int, [vp, sz]),
        "cpprob_hip_group_create": (C.c_int, [C.POINTER(i32), i32, i32, i32, vp, C.POINTER(vp)]),
        "cpprob_hip_group_destroy": (None, [vp]),
        "cpprob_hip_group_last_error": (C.c_char_p, [vp]),
        "cpprob_hip_group_begin": (C.c_int, [vp, C.POINTER(Config), C.POINTER(dbl), sz, vp]),
        "cpprob_hip_group_transport": (C.c_int, [vp, u64, i32, C.c_uint32]),
        "cpprob_hip_group_create_external": (C.c_int, [i32, i32, i32, C.POINTER(Collectives), C.POINTER(vp)]),
        "cpprob_hip_group_traffic": (C.c_int, [vp, C.POINTER(Traffic)]),
        "cpprob_hip_group_profile": (C.c_int, [vp, i32]),
        "cpprob_hip_group_profile_read": (C.c_int, [vp, C.POINTER(dbl)]),
        "cpprob_hip_group_note": (C.c_char_p, [vp]),
        "cpprob_hip_exchange_direct": (C.c_int, [vp, vp]),
        "cpprob_hip_exchange_store": (C.c_int, [vp, vp]),
        "cpprob_hip_exchange_remote": (C.c_int, [vp, vp]),
        "cpprob_hip_exchange_traffic": (C.c_int, [vp, vp, sz, C.POINTER(u64), C.POINTER(u64)]),
        "cpprob_hip_group_run": (C.c_int, [vp, u64]),
        "cpprob_hip_group_sync": (C.c_int, [vp]),
        "cpprob_hip_group_size": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "cpprob_hip_group_context": (vp, [vp, i32]),
        "cpprob_hip_group_results": (C.c_int, [vp, C.POINTER(Summary), C.POINTER(dbl), sz, C.POINTER(i32)]),
        "cpprob_hip_philox_blocks": (C.c_int, [vp, u64, u64, u64, sz, vp]),
        "cpprob_hip_draw_normal": (C.c_int, [vp, u64, u64, u64, dbl, dbl, sz, vp]),
        "cpprob_hip_draw_uniform_smallint": (C.c_int, [vp, u64, u64, u64, i64, i64, sz, vp]),
        "cpprob_hip_draw_discrete": (C.c_int, [vp, u64, u64, u64, C.POINTER(dbl), i32, sz, vp]),
        "cpprob_hip_draw_uniform_real": (C.c_int, [vp, u64, u64, u64, dbl, dbl, sz, vp]),
        "cpprob_hip_draw_poisson": (C.c_int, [vp, u64, u64, u64, dbl, sz, vp]),
        "cpprob_hip_logpdf_normal": (C.c_int, [vp, vp, vp, vp, sz, vp]),
        "cpprob_hip_logpdf_uniform_real": (C.c_int, [vp, vp, vp, vp, sz, vp]),
        "cpprob_hip_logpdf_poisson": (C.c_int, [vp, vp, vp, sz, vp]),
        "cpprob_hip_logpdf_uniform_smallint": (C.c_int, [vp, vp, i64, i64, sz, vp]),
        "cpprob_hip_logpdf_discrete": (C.c_int, [vp, vp, C.POINTER(dbl), i32, sz, vp]),
        "cpprob_hip_fastmath": (C.c_int, [vp, i32, vp, sz, vp, vp]),
        "cpprob_hip_variate_from_bits": (C.c_int, [vp, i32, C.POINTER(dbl), i32, vp, sz, vp, vp]),
        "cpprob_hip_logsumexp_ess": (C.c_int, [vp, vp, sz, C.POINTER(dbl)]),
        "cpprob_hip_weighted_moments": (C.c_int, [vp, vp, vp, sz, C.POINTER(dbl)]),
        "cpprob_hip_weighted_hist": (C.c_int, [vp, vp, vp, sz, i32, C.POINTER(dbl)]),
        "cpprob_hip_weighted_moments_columns": (C.c_int, [vp, vp, sz, sz, vp, sz, C.POINTER(dbl)]),
        "cpprob_hip_weighted_hist_columns": (C.c_int, [vp, vp, sz, sz, vp, sz, i32, C.POINTER(dbl), C.POINTER(dbl)]),
        "cpprob_hip_resample": (C.c_int, [vp, i32, vp, sz, u64, u64, u64, sz, u64, vp]),
        "cpprob_hip_smc_bookkeep": (C.c_int, [vp, i32, vp, sz, u64, i32, i32, dbl, vp, vp, vp, vp]),
        "cpprob_hip_smc_bookkeep_fixed": (C.c_int, [vp, vp, sz, u64, i32, i32, dbl, vp, vp, vp, vp]),
        "cpprob_hip_smc_bookkeep_fixed_rs": (C.c_int, [vp, i32, vp, sz, u64, i32, i32, dbl, vp, vp, vp, vp]),
        "cpprob_hip_generic_begin": (C.c_int, [vp, sz, vp]),
        "cpprob_hip_generic_begin_tiles": (C.c_int, [vp, sz, vp]),
        "cpprob_hip_generic_quantize": (C.c_int, [vp, i32, vp, sz]),
        "cpprob_hip_generic_max": (C.c_int, [vp, i32, vp, sz]),
        "cpprob_hip_generic_quantize_ref": (C.c_int, [vp, i32, vp, sz, dbl]),
        "cpprob_hip_generic_totals": (C.c_int, [vp, i32, sz, vp]),
        "cpprob_hip_generic_finish": (C.c_int, [vp, i32, sz, dbl, vp, vp, vp, vp]),
        "cpprob_hip_systematic_offset": (dbl, [u64, u64]),
        "cpprob_hip_lineage_gather": (C.c_int, [vp, vp, vp, i32, sz, vp, i32, vp, i32, vp]),
        "cpprob_hip_lineage_prepare": (C.c_int, [vp, vp, i32, i32]),
        "cpprob_hip_readback_with_next_result": (C.c_int, [vp, vp, vp, sz]),
        "cpprob_hip_lineage_moments": (C.c_int, [vp, vp, vp, i32, sz, vp, vp, i32, vp, vp]),
        "cpprob_hip_lineage_hist": (C.c_int, [vp, vp, vp, i32, sz, vp, vp, i32, vp, i32, vp, vp]),
        "cpprob_hip_gather_f64": (C.c_int, [vp, vp, vp, sz, vp]),
        "cpprob_hip_gather_i32": (C.c_int, [vp, vp, vp, sz, vp]),
        "cpprob_hip_profile_enable": (C.c_int, [vp, i32]),
        "cpprob_hip_profile_read": (C.c_int, [vp, C.POINTER(dbl), C.POINTER(i64), i32]),
        "cpprob_hip_batch_workspace_bytes": (C.c_int, [C.POINTER(BatchConfig), sz, C.POINTER(u64)]),
        "cpprob_hip_batch_begin": (C.c_int, [vp, C.POINTER(BatchConfig), C.POINTER(dbl), sz]),
        "cpprob_hip_batch_run": (C.c_int, [vp, C.POINTER(u64)]),
        "cpprob_hip_batch_results": (C.c_int, [vp, C.POINTER(Summary), vp, sz, vp, vp]),
        "cpprob_hip_batch_results_device": (C.c_int, [vp, vp, sz]),
        "cpprob_hip_batch_copy_store": (C.c_int, [vp, u64, vp, vp, vp]),
        "cpprob_hip_batch_copy_masses": (C.c_int, [vp, u64, vp, sz]),
        "cpprob_hip_batch_problems_workspace_bytes": (C.c_int, [C.POINTER(BatchConfig), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(u64)]),
        "cpprob_hip_batch_begin_problems": (C.c_int, [vp, C.POINTER(BatchConfig), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(dbl), C.c_int32, vp, vp]),
        "cpprob_hip_batch_online_workspace_bytes": (C.c_int, [C.POINTER(BatchConfig), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(u64)]),
        "cpprob_hip_batch_begin_online": (C.c_int, [vp, C.POINTER(BatchConfig), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int32, vp, vp, C.POINTER(u64)]),
        "cpprob_hip_batch_advance": (C.c_int, [vp, C.POINTER(C.c_uint32), vp, C.c_int32]),
        "cpprob_hip_batch_lengths": (C.c_int, [vp, C.POINTER(C.c_uint32)]),
        "cpprob_hip_batch_paths_layout": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), u64, u64, C.POINTER(u64), C.POINTER(u64)]),
        "cpprob_hip_batch_paths": (C.c_int, [vp, u64, vp, sz, vp, sz]),
        "cpprob_hip_batch_paths_device": (C.c_int, [vp, u64, vp, sz, vp, sz]),
        "cpprob_hip_batch_smooth_layout": (C.c_int, [C.POINTER(C.c_uint32), u64, u64, C.POINTER(u64)]),
        "cpprob_hip_batch_smooth": (C.c_int, [vp, u64, u64, vp, sz, vp, sz]),
        "cpprob_hip_batch_smooth_device": (C.c_int, [vp, u64, u64, vp, sz, vp, sz]),
        "cpprob_hip_batch_smooth_lag": (C.c_int, [vp, u64, C.POINTER(C.c_uint32), u64, u64, u64, vp, sz, vp, sz]),
        "cpprob_hip_batch_smooth_lag_device": (C.c_int, [vp, u64, C.POINTER(C.c_uint32), u64, u64, u64, vp, sz, vp, sz]),
        "cpprob_hip_batch_smooth_grid": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "cpprob_hip_batch_smooth_stats": (C.c_int, [vp, vp, sz, vp, sz]),
        "cpprob_hip_batch_smooth_stats_device": (C.c_int, [vp, vp, sz, vp, sz]),
        "cpprob_hip_batch_online_stats": (C.c_int, [vp, vp, sz, vp, sz]),
        "cpprob_hip_batch_online_stats_device": (C.c_int, [vp, vp, sz, vp, sz]),
        "cpprob_hip_batch_online_stats_progress": (C.c_int, [vp, C.POINTER(C.c_uint32)]),
        "cpprob_hip_batch_traj_stats": (C.c_int, [vp, u64, u64, vp, sz, vp, sz]),
        "cpprob_hip_batch_traj_stats_device": (C.c_int, [vp, u64, u64, vp, sz, vp, sz]),
        "cpprob_hip_batch_traj_stats_grid": (C.c_int, [vp, C.POINTER(C.c_uint32)]),
        "cpprob_hip_batch_forecast": (C.c_int, [vp, u64, u64, u64, vp, sz, vp, sz]),
        "cpprob_hip_batch_forecast_device": (C.c_int, [vp, u64, u64, u64, vp, sz, vp, sz]),
        "cpprob_hip_batch_predictive": (C.c_int, [vp, C.POINTER(C.c_uint32), u64, vp, sz]),
        "cpprob_hip_batch_predictive_device": (C.c_int, [vp, C.POINTER(C.c_uint32), u64, vp, sz]),
        "cpprob_hip_batch_decode": (C.c_int, [vp, vp, sz, vp, sz]),
        "cpprob_hip_batch_decode_device": (C.c_int, [vp, vp, sz, vp, sz]),
        "cpprob_hip_batch_decode_lag": (C.c_int, [vp, u64, C.POINTER(C.c_uint32), u64, vp, sz, vp, sz]),
        "cpprob_hip_batch_decode_lag_device": (C.c_int, [vp, u64, C.POINTER(C.c_uint32), u64, vp, sz, vp, sz]),
        "cpprob_hip_batch_decode_logp": (C.c_int, [vp, u64, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "cpprob_hip_batch_pass_grid": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "cpprob_hip_batch_run_conditional": (C.c_int, [vp, C.POINTER(u64), vp, sz]),
        "cpprob_hip_batch_run_conditional_device": (C.c_int, [vp, C.POINTER(u64), vp, sz]),
        "cpprob_hip_batch_retable": (C.c_int, [vp, vp, vp, vp, sz]),
        "cpprob_hip_batch_retable_device": (C.c_int, [vp, vp, vp, vp, sz]),
        "cpprob_hip_batch_retable_status": (C.c_int, [vp, C.POINTER(i32)]),
        "cpprob_hip_batch_retable_grid": (C.c_int, [vp, C.POINTER(C.c_uint32)]),
        "cpprob_hip_batch_mstep_device": (C.c_int, [vp, vp, sz, vp, vp]),
        "cpprob_hip_batch_copy_step_tables": (C.c_int, [vp, u64, vp, sz, vp]),
        "cpprob_hip_batch_summaries_device": (C.c_int, [vp, vp]),
        "cpprob_hip_batch_learn_begin": (C.c_int, [vp, vp, sz, C.c_uint32]),
        "cpprob_hip_batch_advance_learn": (C.c_int, [vp, C.POINTER(C.c_uint32), vp]),
        "cpprob_hip_batch_advance_learn_device": (C.c_int, [vp, C.POINTER(C.c_uint32), vp, sz]),
        "cpprob_hip_batch_online_tables": (C.c_int, [vp, vp, vp]),
        "cpprob_hip_batch_learn_tables": (C.c_int, [vp, vp, vp, C.POINTER(i32)]),
        "cpprob_hip_batch_learn_tables_device": (C.c_int, [vp, vp, vp]),
        "cpprob_hip_batch_learn_record": (C.c_int, [vp, vp, sz]),
        "cpprob_hip_table_log": (dbl, [dbl]),
        "cpprob_hip_batch_begin_problems_scaled": (C.c_int, [vp, C.POINTER(BatchConfig), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(dbl), C.c_int32, vp, vp, vp]),
        "cpprob_hip_batch_begin_online_scaled": (C.c_int, [vp, C.POINTER(BatchConfig), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int32, vp, vp, vp, C.POINTER(u64)]),
        "cpprob_hip_batch_retable_scaled": (C.c_int, [vp, vp, vp, vp, vp, sz]),
        "cpprob_hip_batch_retable_scaled_device": (C.c_int, [vp, vp, vp, vp, vp, sz]),
        "cpprob_hip_batch_mstep_scaled_device": (C.c_int, [vp, vp, sz, vp, vp, vp, vp, dbl]),
        "cpprob_hip_batch_online_tables_scaled": (C.c_int, [vp, vp, vp, vp]),
        "cpprob_hip_batch_copy_scales": (C.c_int, [vp, u64, vp, vp]),
        "cpprob_hip_batch_begin_problems_poisson": (C.c_int, [vp, C.POINTER(BatchConfig), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(dbl), C.c_int32, vp, vp]),
        "cpprob_hip_batch_begin_online_poisson": (C.c_int, [vp, C.POINTER(BatchConfig), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int32, vp, vp, C.POINTER(u64)]),
        "cpprob_hip_batch_retable_poisson": (C.c_int, [vp, vp, vp, vp, sz]),
        "cpprob_hip_batch_retable_poisson_device": (C.c_int, [vp, vp, vp, vp, sz]),
        "cpprob_hip_batch_mstep_poisson_device": (C.c_int, [vp, vp, sz, vp, vp, vp, dbl]),
        "cpprob_hip_batch_online_tables_poisson": (C.c_int, [vp, vp, vp]),
        "cpprob_hip_batch_copy_rates": (C.c_int, [vp, u64, vp, vp]),
        "cpprob_hip_batch_learn_begin_scaled": (C.c_int, [vp, vp, sz, C.c_uint32, dbl]),
        "cpprob_hip_batch_learn_tables_scaled": (C.c_int, [vp, vp, vp, vp, C.POINTER(i32)]),
        "cpprob_hip_batch_learn_tables_scaled_device": (C.c_int, [vp, vp, vp, vp]),
        "cpprob_hip_batch_tie": (C.c_int, [vp, C.POINTER(i32), sz]),
        "cpprob_hip_batch_tie_get": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "cpprob_hip_batch_pool_stats": (C.c_int, [vp, vp, sz, C.c_uint32, C.c_int, vp, sz]),
        "cpprob_hip_batch_pool_stats_device": (C.c_int, [vp, vp, sz, C.c_uint32, C.c_int, vp, sz]),
        "cpprob_hip_batch_learn_tie": (C.c_int, [vp]),
        "cpprob_hip_batch_learn_pooled_record": (C.c_int, [vp, vp, sz]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.cpprob_hip_abi_version() != 3:
        raise CpprobHipError("ABI version mismatch")
    if p == LIB_PATH:
        # the in-tree binary must be the build of the sources next to it (a stale .so that merely looks newer is refused)
        from . import build as B
        have, want = L.cpprob_hip_build_id().decode(), B.source_hash()
        if have != want:
            raise CpprobHipError("%s was built from other sources (build id %s, sources %s): run `python -m cpprob_amd.build`" % (p, have, want))
    if path is None:
        _lib = L
    return L


def _dptr(t):
    """Device pointer of a torch tensor (contiguous), or None.

    Stream contract (include/cpprob_hip.h): the engine's stream is non-blocking, so work torch queued on ITS stream for a
    tensor (the fill of torch.zeros, an H2D copy) is not ordered before what the engine then does with that memory.  The
    caller completes its tensors first -- torch.cuda.current_stream().synchronize() after creating them, once."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


class Engine:
    """One context = one device, one stream, one particle shard (include/cpprob_hip.h)."""

    def __init__(self, device=0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.cpprob_hip_create(int(device), C.byref(h))
        if rc:
            msg = self.L.cpprob_hip_last_error(None)
            raise CpprobHipError("cpprob_hip_create failed (%d): %s" % (rc, msg.decode() if msg else "?"))
        self.h = h
        self.device = device
        self.cfg = None
        self.T = 0
        self.is_int = False
        self.K = 0
        self.batch_shapes = None              # (h_T, h_n) of a batch begun by batch_begin_problems
        self.batch_k = 0                      # the states of the tables batch_begin_online / batch_online_tables took last

    def close(self):
        if getattr(self, "h", None):
            self.L.cpprob_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            msg = self.L.cpprob_hip_last_error(self.h)
            e = CpprobHipError("cpprob_hip error %d: %s" % (rc, msg.decode() if msg else "?"))
            e.code = rc
            raise e

    @property
    def stream_ptr(self):
        """The context's hipStream_t.  Reading it pins the context to that one stream until it is closed: no run lanes (lanes())."""
        return self.L.cpprob_hip_stream(self.h)

    def sync(self):
        self._chk(self.L.cpprob_hip_sync(self.h))

    def set_hmm(self, means, trans):
        """The table of MODEL_HMM_TABLE: k = len(means) states (2..8), emission N(means[s], 1), transition rows trans[s] (weights)."""
        m = np.ascontiguousarray(means, np.float64)
        tr = np.ascontiguousarray(trans, np.float64)
        assert tr.shape == (len(m), len(m))
        self._chk(self.L.cpprob_hip_set_hmm(self.h, len(m), m.ctypes.data_as(C.POINTER(C.c_double)), tr.ctypes.data_as(C.POINTER(C.c_double))))

    # ---- cpprob::inference --------------------------------------------------------------
    def begin(self, algorithm, model, observes, n_particles, seed=12345, resampler=RESAMPLE_SYSTEMATIC, ess_threshold=2.0,
              particle_offset=0, n_global=None, scope=SCOPE_GLOBAL, keep_history=True, flags=0, fuse_max_tiles=0):
        """keep_history=False: filtering only -- two rows of the particle store and no ancestors (memory O(N) instead of
        O(N T)); stats() then holds every predict hit's statistics under ITS generation's weights, and values() / ancestors() /
        paths() raise."""
        obs = np.ascontiguousarray(observes, np.float64)
        self._begin_args = dict(algorithm=algorithm, model=model, observes=obs.copy(), n_particles=n_particles, seed=seed, resampler=resampler, ess_threshold=ess_threshold,
                                particle_offset=particle_offset, n_global=n_global, scope=scope, keep_history=keep_history, flags=flags, fuse_max_tiles=fuse_max_tiles)
        cfg = Config(algorithm, model, resampler, scope, 1 if keep_history else 0, 0, int(flags), int(fuse_max_tiles), float(ess_threshold), int(seed),
                     int(n_particles), int(particle_offset), int(n_particles if n_global is None else n_global))
        self._chk(self.L.cpprob_hip_infer_begin(self.h, C.byref(cfg), obs.ctypes.data_as(C.POINTER(C.c_double)), len(obs)))
        self.cfg = cfg
        gauss = model in (MODEL_GAUSSIAN_UNKNOWN_MEAN, MODEL_GAUSSIAN_README)
        self.T = 1 if gauss else len(obs)
        self.is_int = model in (MODEL_HMM3, MODEL_HMM_TABLE)
        self.K = 8 if model == MODEL_HMM_TABLE else (3 if self.is_int else 2)
        self.n = int(n_particles)
        return self

    def rebegin(self, extra_flags):
        """begin() again with the same arguments and further cpprob_hip_config::flags."""
        a = dict(self._begin_args)
        a["flags"] = int(a["flags"]) | int(extra_flags)
        return self.begin(**a)

    def run(self, run_index=0):
        self._chk(self.L.cpprob_hip_infer_run(self.h, int(run_index)))

    def lanes(self):
        """Run lanes of this context (cpprob_hip_infer_lanes): depth = lanes begun (1: the context alone), last_lane = lane of the
        last run, lane_bytes = device bytes the further lanes hold, serial_reason = 0 or SERIAL_*.  Changes nothing."""
        d, last, nbytes, why = C.c_int32(), C.c_int32(), C.c_uint64(), C.c_int32()
        self._chk(self.L.cpprob_hip_infer_lanes(self.h, C.byref(d), C.byref(last), C.byref(nbytes), C.byref(why)))
        return {"depth": d.value, "last_lane": last.value, "lane_bytes": nbytes.value, "serial_reason": why.value}

    def summary(self):
        s = Summary()
        self._chk(self.L.cpprob_hip_infer_summary(self.h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in Summary._fields_}

    def stats(self):
        out = np.zeros((self.T, self.K))
        self._chk(self.L.cpprob_hip_infer_stats(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), out.size))
        return out

    def results(self):
        """summary, stats and step trace in one call and one stream synchronisation (cpprob_hip_infer_results)."""
        s = Summary()
        out = np.zeros((self.T, self.K))
        ess = np.zeros(self.T)
        res = np.zeros(self.T, np.int32)
        self._chk(self.L.cpprob_hip_infer_results(self.h, C.byref(s), out.ctypes.data, out.size, ess.ctypes.data, res.ctypes.data))
        return {f: getattr(s, f) for f, _ in Summary._fields_}, out, ess, res

    def results_device(self, out):
        """{log_evidence, ess, log_norm, max_logw, stats...} of the enqueued run into a device tensor; no host sync."""
        self._chk(self.L.cpprob_hip_infer_results_device(self.h, _dptr(out), out.numel()))

    def step_trace(self):
        ess = np.zeros(self.T)
        res = np.zeros(self.T, np.int32)
        self._chk(self.L.cpprob_hip_infer_step_trace(self.h, ess.ctypes.data_as(C.POINTER(C.c_double)),
                                                     res.ctypes.data_as(C.POINTER(C.c_int32))))
        return ess, res

    def values(self):
        out = np.zeros((self.T, self.n), np.int32 if self.is_int else np.float64)
        self._chk(self.L.cpprob_hip_copy_values(self.h, out.ctypes.data, out.nbytes))
        return out

    def ancestors(self):
        out = np.zeros((self.T, self.n), np.int32)
        self._chk(self.L.cpprob_hip_copy_ancestors(self.h, out.ctypes.data, out.nbytes))
        return out

    def logw(self):
        out = np.zeros(self.n)
        self._chk(self.L.cpprob_hip_copy_logw(self.h, out.ctypes.data, out.nbytes))
        return out

    def paths(self):
        out = np.zeros((self.T, self.n), np.int32 if self.is_int else np.float64)
        self._chk(self.L.cpprob_hip_copy_paths(self.h, out.ctypes.data, out.nbytes))
        return out

    # ---- batched SMC: many small problems, one launch (include/cpprob_hip.h: cpprob_hip_batch_*) --------------------
    @staticmethod
    def batch_config(model, n_particles, n_problems, resampler=RESAMPLE_SYSTEMATIC, ess_threshold=2.0, keep_history=True, algorithm=ALG_SMC, flags=0):
        return BatchConfig(int(algorithm), int(model), int(resampler), 1 if keep_history else 0, int(flags), float(ess_threshold), int(n_particles), int(n_problems))

    @staticmethod
    def batch_workspace_bytes(model, n_particles, n_problems, T, **kw):
        """Device bytes a batch of n_problems problems of T observes needs: a pure host function (no device, no context)."""
        return batch_workspace_bytes(model, n_particles, n_problems, T, **kw)

    def batch_begin(self, model, observes, n_particles, resampler=RESAMPLE_SYSTEMATIC, ess_threshold=2.0, keep_history=True, algorithm=ALG_SMC, flags=0,
                    keep_masses=False):
        """observes [B, T]: problem b's observation sequence in row b.  keep_masses (with keep_history=False, here and in the other
        two begins): the run keeps the backward smoother's m table, 64 bytes a problem and step, and batch_smooth, batch_smooth_lag and
        batch_smooth_stats serve the filtering-only batch; batch_masses(b) reads the table."""
        obs = np.ascontiguousarray(observes, np.float64)
        if obs.ndim != 2:
            raise ValueError("observes must be [n_problems, T]")
        cfg = self.batch_config(model, n_particles, obs.shape[0], resampler, ess_threshold, keep_history, algorithm, _batch_flags(flags, keep_masses))
        self._chk(self.L.cpprob_hip_batch_begin(self.h, C.byref(cfg), obs.ctypes.data_as(C.POINTER(C.c_double)), obs.shape[1]))
        self.batch_B, self.batch_T, self.batch_n = obs.shape[0], obs.shape[1], int(n_particles)
        self.batch_K = 3 if model == MODEL_HMM3 else 8
        self.batch_shapes = None
        return self

    def batch_begin_problems(self, model, observes, n_particles, tables=None, resampler=RESAMPLE_SYSTEMATIC, ess_threshold=2.0, keep_history=True, algorithm=ALG_SMC, flags=0,
                             max_particles=None, keep_masses=False, emission="normal"):
        """A batch whose problems differ.  observes: a list of 1-D arrays, problem b's own sequence (any lengths); n_particles: an int
        or one count a problem; tables (MODEL_HMM_TABLE): None (the set_hmm table for every problem) or (means [B, k], transition
        [B, k, k]), problem b's own table, or (means, transition, sigmas [B, k]): state s of problem b emits N(means[b, s],
        sigmas[b, s]) (cpprob_hip_batch_begin_problems_scaled).  emission="poisson": tables = (rates [B, k], transition), state s of
        problem b emits Poisson(rates[b, s]) and the observes are counts 0 .. 4095 (cpprob_hip_batch_begin_problems_poisson).
        batch_results() then returns arrays padded to the longest problem (rows t >= T_b zero) and batch_store(b) problem b's own
        [T_b, n_b]."""
        poisson = _poisson(emission, tables)
        seqs = [np.ascontiguousarray(o, np.float64).reshape(-1) for o in observes]
        h_T, h_n = _problem_shapes([len(o) for o in seqs], n_particles)
        flat = np.ascontiguousarray(np.concatenate(seqs) if seqs else np.zeros(0))
        top = int(h_n.max()) if (max_particles is None and h_n.size) else int(max_particles or 0)
        cfg = self.batch_config(model, top, len(seqs), resampler, ess_threshold, keep_history, algorithm, _batch_flags(flags, keep_masses))
        k, means, trans, sigmas = 0, None, None, None
        if tables is not None:
            means = np.ascontiguousarray(tables[0], np.float64)
            trans = np.ascontiguousarray(tables[1], np.float64)
            if means.ndim != 2 or trans.shape != (means.shape[0], means.shape[1], means.shape[1]) or means.shape[0] != len(seqs):
                raise ValueError("tables = (means [B, k], transition [B, k, k])")
            k = means.shape[1]
            sigmas = self._batch_sigmas(tables, means)
        if poisson:
            self._chk(self.L.cpprob_hip_batch_begin_problems_poisson(self.h, C.byref(cfg), h_T.ctypes.data_as(C.POINTER(C.c_uint32)), h_n.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                                     flat.ctypes.data_as(C.POINTER(C.c_double)), k, means.ctypes.data, trans.ctypes.data))
            self.batch_k = k                                 # (batch_copy_rates reads it)
        elif sigmas is not None:
            self._chk(self.L.cpprob_hip_batch_begin_problems_scaled(self.h, C.byref(cfg), h_T.ctypes.data_as(C.POINTER(C.c_uint32)), h_n.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                                    flat.ctypes.data_as(C.POINTER(C.c_double)), k, means.ctypes.data, trans.ctypes.data, sigmas.ctypes.data))
            self.batch_k = k                                 # (batch_scales reads it)
        else:
            self._chk(self.L.cpprob_hip_batch_begin_problems(self.h, C.byref(cfg), h_T.ctypes.data_as(C.POINTER(C.c_uint32)), h_n.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                             flat.ctypes.data_as(C.POINTER(C.c_double)), k, None if means is None else means.ctypes.data,
                                                             None if trans is None else trans.ctypes.data))
        self.batch_B, self.batch_T, self.batch_n = len(seqs), int(h_T.max()), top
        self.batch_K = 3 if model == MODEL_HMM3 else 8
        self.batch_shapes = (h_T, h_n)
        return self

    @staticmethod
    def _batch_sigmas(tables, means):
        """The third array of a tables tuple, [B, k] as the means, or None for a 2-tuple."""
        if len(tables) < 3 or tables[2] is None:
            return None
        sigmas = np.ascontiguousarray(tables[2], np.float64)
        if sigmas.shape != means.shape:
            raise ValueError("tables = (means [B, k], transition [B, k, k], sigmas [B, k])")
        return sigmas

    def batch_begin_online(self, model, capacity, n_particles, seeds, tables=None, resampler=RESAMPLE_SYSTEMATIC, ess_threshold=2.0, keep_history=True, algorithm=ALG_SMC,
                           flags=0, max_particles=None, keep_masses=False, emission="normal"):
        """A batch whose observes arrive over time.  capacity: the most observes problem b may reach, one a problem; n_particles and
        tables as for batch_begin_problems; seeds: one Philox key a problem, for the life of the batch.  Every problem starts at
        length 0; batch_advance() feeds it.  batch_results() returns arrays padded to the largest capacity and batch_store(b) the
        [L_b, n_b] rows reached.  A 3-tuple of tables carries the emission scales (cpprob_hip_batch_begin_online_scaled);
        emission="poisson": tables = (rates, transition) (cpprob_hip_batch_begin_online_poisson)."""
        poisson = _poisson(emission, tables)
        h_T, h_n = _problem_shapes(capacity, n_particles)
        sd = np.ascontiguousarray(seeds, np.uint64)
        if sd.shape != h_T.shape:
            raise ValueError("one seed per problem")
        top = int(h_n.max()) if (max_particles is None and h_n.size) else int(max_particles or 0)
        cfg = self.batch_config(model, top, h_T.size, resampler, ess_threshold, keep_history, algorithm, _batch_flags(flags, keep_masses))
        k, means, trans, sigmas = 0, None, None, None
        if tables is not None:
            means = np.ascontiguousarray(tables[0], np.float64)
            trans = np.ascontiguousarray(tables[1], np.float64)
            if means.ndim != 2 or trans.shape != (means.shape[0], means.shape[1], means.shape[1]) or means.shape[0] != h_T.size:
                raise ValueError("tables = (means [B, k], transition [B, k, k])")
            k = means.shape[1]
            sigmas = self._batch_sigmas(tables, means)
        self.batch_k = k
        if poisson:
            self._chk(self.L.cpprob_hip_batch_begin_online_poisson(self.h, C.byref(cfg), h_T.ctypes.data_as(C.POINTER(C.c_uint32)), h_n.ctypes.data_as(C.POINTER(C.c_uint32)), k,
                                                                   means.ctypes.data, trans.ctypes.data, sd.ctypes.data_as(C.POINTER(C.c_uint64))))
        elif sigmas is not None:
            self._chk(self.L.cpprob_hip_batch_begin_online_scaled(self.h, C.byref(cfg), h_T.ctypes.data_as(C.POINTER(C.c_uint32)), h_n.ctypes.data_as(C.POINTER(C.c_uint32)), k,
                                                                  means.ctypes.data, trans.ctypes.data, sigmas.ctypes.data, sd.ctypes.data_as(C.POINTER(C.c_uint64))))
        else:
            self._chk(self.L.cpprob_hip_batch_begin_online(self.h, C.byref(cfg), h_T.ctypes.data_as(C.POINTER(C.c_uint32)), h_n.ctypes.data_as(C.POINTER(C.c_uint32)), k,
                                                           None if means is None else means.ctypes.data, None if trans is None else trans.ctypes.data,
                                                           sd.ctypes.data_as(C.POINTER(C.c_uint64))))
        self.batch_B, self.batch_T, self.batch_n = int(h_T.size), int(h_T.max()), top
        self.batch_K = 3 if model == MODEL_HMM3 else 8
        self.batch_shapes = (np.zeros(h_T.size, np.uint32), h_n)
        return self

    def batch_advance(self, new_observes, readout=True):
        """new_observes: a list of 1-D arrays, problem b's new observes (possibly none).  One launch over the new steps, enqueued
        without waiting.  readout=False (keep_history only) leaves the smoothed statistics to a later advance with readout=True,
        which may carry no observes at all."""
        seqs = [np.ascontiguousarray(o, np.float64).reshape(-1) for o in new_observes]
        if len(seqs) != self.batch_B:
            raise ValueError("one (possibly empty) sequence per problem")
        h_dT = np.array([len(o) for o in seqs], np.uint32)
        flat = np.ascontiguousarray(np.concatenate(seqs)) if seqs else np.zeros(0)
        self._chk(self.L.cpprob_hip_batch_advance(self.h, h_dT.ctypes.data_as(C.POINTER(C.c_uint32)), flat.ctypes.data if flat.size else None, 1 if readout else 0))
        self.batch_shapes = (self.batch_lengths(), self.batch_shapes[1])

    def batch_lengths(self):
        """The observes every problem of an online batch has seen so far (uint32 [B])."""
        out = np.zeros(self.batch_B, np.uint32)
        self._chk(self.L.cpprob_hip_batch_lengths(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def batch_run(self, seeds):
        """One launch; problem b runs with Philox key seeds[b]."""
        sd = np.ascontiguousarray(seeds, np.uint64)
        if sd.shape != (self.batch_B,):
            raise ValueError("one seed per problem")
        self._chk(self.L.cpprob_hip_batch_run(self.h, sd.ctypes.data_as(C.POINTER(C.c_uint64))))

    def _conditional_seeds(self, seeds):
        sd = np.ascontiguousarray(seeds, np.uint64)
        if sd.shape != (self.batch_B,):
            raise ValueError("one seed per problem")
        return sd

    def batch_run_conditional(self, seeds, ref):
        """A conditional SMC run in place of batch_run (cpprob_hip_batch_run_conditional): slot 0 of problem b follows its reference
        path.  ref: a list of B integer arrays of lengths T_b, or one packed array (problem after problem, as
        batch_smooth_layout(T, 1) packs trajectories); every entry a state 0 .. k - 1.  The batch: MODEL_HMM_TABLE, keep_history=False,
        keep_masses=True; the resampling is multinomial whatever the batch's resampler.  The run keeps the m table only:
        batch_masses, batch_smooth*, batch_traj_stats*, batch_forecast*, batch_predictive* and batch_decode* serve it, batch_results
        waits for the next batch_run."""
        sd = self._conditional_seeds(seeds)
        h_T, _ = self._batch_problem_shapes()
        if isinstance(ref, np.ndarray) and ref.ndim == 1:
            flat = np.ascontiguousarray(ref, np.int32)
        else:
            paths = [np.ascontiguousarray(r, np.int32).reshape(-1) for r in ref]
            if len(paths) != self.batch_B:
                raise ValueError("one reference path per problem")
            if any(len(r) != int(T) for r, T in zip(paths, h_T)):
                raise ValueError("problem b's reference path holds T_b states")
            flat = np.ascontiguousarray(np.concatenate(paths), np.int32)
        if flat.size != int(np.sum(h_T, dtype=np.int64)):
            raise ValueError("the reference paths hold one state per problem and step: %d entries" % int(np.sum(h_T, dtype=np.int64)))
        self._chk(self.L.cpprob_hip_batch_run_conditional(self.h, sd.ctypes.data_as(C.POINTER(C.c_uint64)), flat.ctypes.data, flat.size))

    def batch_run_conditional_device(self, seeds, ref_i8):
        """The same with the reference paths in a torch int8 device tensor packed as batch_smooth_layout(T, 1) says -- what
        batch_smooth_device(traj_i8=..., n_traj=1) writes --, enqueued without a host synchronisation."""
        sd = self._conditional_seeds(seeds)
        h_T, _ = self._batch_problem_shapes()
        if ref_i8 is None or ref_i8.numel() != int(np.sum(h_T, dtype=np.int64)):
            raise ValueError("the reference paths hold one state per problem and step: %d entries" % int(np.sum(h_T, dtype=np.int64)))
        self._chk(self.L.cpprob_hip_batch_run_conditional_device(self.h, sd.ctypes.data_as(C.POINTER(C.c_uint64)), _dptr(ref_i8), ref_i8.numel()))

    # ---- re-tabling a begun batch (include/cpprob_hip.h: cpprob_hip_batch_retable*) ----------------------------------
    def batch_retable(self, tables, observes=None, emission="normal"):
        """New tables for the begun MODEL_HMM_TABLE batch of problems where it stands (cpprob_hip_batch_retable): tables = (means
        [B, k], transition [B, k, k]) on the host, validated as batch_begin_problems validates them.  observes: the problems'
        sequences as batch_begin_problems took them, or None once a previous batch_retable of this begun batch has staged them.
        Everything the batch returns afterwards is what a fresh batch_begin_problems with these tables returns, bit for bit; like a
        begin, the read-outs wait for the next batch_run / batch_run_conditional.  A 3-tuple (means, transition, sigmas [B, k])
        re-tables a batch begun with emission scales (cpprob_hip_batch_retable_scaled); emission="poisson": tables = (rates,
        transition) re-table a batch begun with Poisson emissions (cpprob_hip_batch_retable_poisson)."""
        poisson = _poisson(emission, tables)
        means = np.ascontiguousarray(tables[0], np.float64)
        trans = np.ascontiguousarray(tables[1], np.float64)
        if means.ndim != 2 or trans.shape != (means.shape[0], means.shape[1], means.shape[1]) or means.shape[0] != self.batch_B:
            raise ValueError("tables = (means [B, k], transition [B, k, k])")
        h_T, _ = self._batch_problem_shapes()
        flat = None if observes is None else self._batch_packed_observes(observes)
        sigmas = self._batch_sigmas(tables, means)
        h_obs, n_obs = None if flat is None or flat.size == 0 else flat.ctypes.data, int(np.sum(h_T, dtype=np.int64)) if flat is None else flat.size
        if poisson:
            self._chk(self.L.cpprob_hip_batch_retable_poisson(self.h, means.ctypes.data, trans.ctypes.data, h_obs, n_obs))
        elif sigmas is not None:
            self._chk(self.L.cpprob_hip_batch_retable_scaled(self.h, means.ctypes.data, trans.ctypes.data, sigmas.ctypes.data, h_obs, n_obs))
        else:
            self._chk(self.L.cpprob_hip_batch_retable(self.h, means.ctypes.data, trans.ctypes.data, h_obs, n_obs))

    def batch_retable_device(self, means, trans, observes, sigmas=None, emission="normal"):
        """The same between torch float64 device tensors (means [B, k], trans [B, k, k], observes packed problem after problem),
        enqueued without a host synchronisation; the tables are checked on the device (batch_retable_status).  sigmas [B, k]: the
        emission scales of a batch begun with them (cpprob_hip_batch_retable_scaled_device).  emission="poisson": means holds the
        rates of a batch begun with Poisson emissions (cpprob_hip_batch_retable_poisson_device)."""
        n_obs = 0 if observes is None else observes.numel()
        if _poisson(emission, (means, trans) if sigmas is None else (means, trans, sigmas)):
            self._chk(self.L.cpprob_hip_batch_retable_poisson_device(self.h, _dptr(means), _dptr(trans), _dptr(observes), n_obs))
        elif sigmas is not None:
            self._chk(self.L.cpprob_hip_batch_retable_scaled_device(self.h, _dptr(means), _dptr(trans), _dptr(sigmas), _dptr(observes), n_obs))
        else:
            self._chk(self.L.cpprob_hip_batch_retable_device(self.h, _dptr(means), _dptr(trans), _dptr(observes), n_obs))

    def batch_retable_status(self):
        """int32 [B] of the last re-table: 0, or bits 1 (a weight not finite or < 0), 2 (a transition row without mass), 4 (a mean
        not finite), 8 (a scaled re-table: a sigma not finite, not > 0, or with a 2 pi sigma^2 that is not a normal number), 16 (a
        Poisson re-table: a rate not > 0, not finite or not a normal number; bit 4 is not used there) -- such a problem kept its
        previous table.  Synchronises."""
        out = np.zeros(self.batch_B, np.int32)
        self._chk(self.L.cpprob_hip_batch_retable_status(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def batch_retable_grid(self):
        """gridDim.y of the last re-table launch (0: none)."""
        g = C.c_uint32()
        self._chk(self.L.cpprob_hip_batch_retable_grid(self.h, C.byref(g)))
        return int(g.value)

    def batch_mstep_device(self, stats, means, trans, sigmas=None, sigma_floor=1e-3, log_norms=None, emission="normal", rate_floor=1e-6, log_rates=None):
        """em.m_step on the device (cpprob_hip_batch_mstep_device): stats torch float64 [B, 88] as batch_smooth_stats_device leaves
        them; means [B, k] and trans [B, k, k] torch float64, updated in place.  Enqueued without a host synchronisation.
        sigmas [B, k]: the emission scales, updated in place too, none below sigma_floor (cpprob_hip_batch_mstep_scaled_device);
        log_norms [B, k], if given, takes the new sigmas' log(2 pi sigma^2): for tests, a fitting loop has no use for it.
        emission="poisson": means holds the rates, none left below rate_floor (cpprob_hip_batch_mstep_poisson_device); log_rates
        [B, k], if given, takes the new rates' logarithms, for tests."""
        if _poisson(emission, (means, trans) if sigmas is None else (means, trans, sigmas)):
            self._chk(self.L.cpprob_hip_batch_mstep_poisson_device(self.h, _dptr(stats), stats.numel(), _dptr(means), _dptr(trans), _dptr(log_rates), float(rate_floor)))
        elif sigmas is not None:
            self._chk(self.L.cpprob_hip_batch_mstep_scaled_device(self.h, _dptr(stats), stats.numel(), _dptr(means), _dptr(trans), _dptr(sigmas), _dptr(log_norms),
                                                                  float(sigma_floor)))
        else:
            self._chk(self.L.cpprob_hip_batch_mstep_device(self.h, _dptr(stats), stats.numel(), _dptr(means), _dptr(trans)))

    # ---- tied tables (include/cpprob_hip.h: cpprob_hip_batch_tie, _pool_stats*) --------------------------------------
    def batch_tie(self, groups):
        """Partitions the begun batch's problems into groups that share one table (cpprob_hip_batch_tie): groups int [B], ids in
        0 .. G-1, every id used.  A re-table keeps the tie, any begin forgets it, a second call replaces it."""
        g = np.ascontiguousarray(groups, np.int32).reshape(-1)
        self._chk(self.L.cpprob_hip_batch_tie(self.h, g.ctypes.data_as(C.POINTER(C.c_int32)), g.size))

    def batch_tie_get(self):
        """(groups int32 [B], G) of the begun batch's tie (cpprob_hip_batch_tie_get); without one the call raises (ESTATE)."""
        G = C.c_int32()
        self._chk(self.L.cpprob_hip_batch_tie_get(self.h, None, C.byref(G)))
        g = np.zeros(self.batch_B, np.int32)
        self._chk(self.L.cpprob_hip_batch_tie_get(self.h, g.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(G)))
        return g, int(G.value)

    def batch_pool_stats(self, records, per_problem=1, broadcast=True, out=None):
        """The tied groups' pooled records (cpprob_hip_batch_pool_stats; cpprob_amd.em.pool_stats states the sum): records float64
        [B, 88] or [B, per_problem, 88] on the host, staged and pooled by the device's kernel.  broadcast=True: the records' shape,
        every member holding its group's sum; False: [G, ...].  out: a contiguous float64 array to fill (default: a new one).
        Synchronises."""
        rec = np.ascontiguousarray(records, np.float64)
        R = int(per_problem)
        if out is None:
            rows = self.batch_B if broadcast else self.batch_tie_get()[1]
            out = np.zeros((rows, STATS_PER_PROBLEM) if rec.ndim == 2 and R == 1 else (rows, R, STATS_PER_PROBLEM))
        if not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous):
            raise ValueError("out: a contiguous float64 array")
        self._chk(self.L.cpprob_hip_batch_pool_stats(self.h, rec.ctypes.data, rec.size, R, 1 if broadcast else 0, out.ctypes.data, out.size))
        return out

    def batch_pool_stats_device(self, records, out, per_problem=1, broadcast=True):
        """batch_pool_stats on torch float64 tensors of the engine's device (cpprob_hip_batch_pool_stats_device), enqueued without a
        host synchronisation: records [B, per_problem, 88] (or [B, 88]), out [B, ...] (broadcast; may be records itself: the pooling
        is then in place) or [G, ...]."""
        self._chk(self.L.cpprob_hip_batch_pool_stats_device(self.h, _dptr(records), records.numel(), int(per_problem), 1 if broadcast else 0, _dptr(out), out.numel()))

    def batch_scales(self, b, k=None):
        """(sigmas [k], log_norms [k]) of problem b of a batch begun with emission scales, as the device holds them
        (cpprob_hip_batch_copy_scales).  Synchronises.  For tests."""
        k = int(k if k is not None else self.batch_k)
        sg, ln = np.zeros(k), np.zeros(k)
        self._chk(self.L.cpprob_hip_batch_copy_scales(self.h, int(b), sg.ctypes.data, ln.ctypes.data))
        return sg, ln

    def batch_copy_rates(self, b, k=None):
        """(rates [k], log_rates [k]) of problem b of a batch begun with Poisson emissions, as the device holds them
        (cpprob_hip_batch_copy_rates).  Synchronises.  For tests."""
        k = int(k if k is not None else self.batch_k)
        rt, lr = np.zeros(k), np.zeros(k)
        self._chk(self.L.cpprob_hip_batch_copy_rates(self.h, int(b), rt.ctypes.data, lr.ctypes.data))
        return rt, lr

    # ---- online EM of an online batch (include/cpprob_hip.h: cpprob_hip_batch_learn_*) ------------------------------
    def _batch_tables(self, tables):
        means = np.ascontiguousarray(tables[0], np.float64)
        trans = np.ascontiguousarray(tables[1], np.float64)
        if means.ndim != 2 or trans.shape != (means.shape[0], means.shape[1], means.shape[1]) or means.shape[0] != self.batch_B:
            raise ValueError("tables = (means [B, k], transition [B, k, k])")
        self.batch_k = means.shape[1]
        return means, trans

    def batch_learn_begin(self, gamma, t_min, sigma_floor=None, tied=False):
        """Arms the online MODEL_HMM_TABLE batch just begun (per-problem tables; before its first advance) for online EM
        (cpprob_hip_batch_learn_begin): gamma[t] in (0, 1], the step size of a problem's absolute step t, at least as long as the
        largest capacity; t_min: the length a problem must have reached before its first M-step.  sigma_floor (a batch begun with
        emission scales): the learner fits the sigmas too, none below it (cpprob_hip_batch_learn_begin_scaled); None on such a batch:
        means and transition rows are learned and the sigmas stay.  tied=True (a batch with a tie, batch_tie): the learner pools over
        the tie -- the streams of a group learn one table, t_min counts the group's observes (cpprob_hip_batch_learn_tie)."""
        g = np.ascontiguousarray(gamma, np.float64).reshape(-1)
        if sigma_floor is not None:
            self._chk(self.L.cpprob_hip_batch_learn_begin_scaled(self.h, g.ctypes.data if g.size else None, g.size, int(t_min), float(sigma_floor)))
        else:
            self._chk(self.L.cpprob_hip_batch_learn_begin(self.h, g.ctypes.data if g.size else None, g.size, int(t_min)))
        if tied:
            self._chk(self.L.cpprob_hip_batch_learn_tie(self.h))

    def _batch_new_observes(self, new_observes):
        seqs = [np.ascontiguousarray(o, np.float64).reshape(-1) for o in new_observes]
        if len(seqs) != self.batch_B:
            raise ValueError("one (possibly empty) sequence per problem")
        return np.array([len(o) for o in seqs], np.uint32), (np.ascontiguousarray(np.concatenate(seqs)) if seqs else np.zeros(0))

    def batch_advance_learn(self, new_observes):
        """batch_advance on an armed batch (cpprob_hip_batch_advance_learn): the new rows are written on the device from the tables
        in force, the new steps run, and the learn step pushes the discounted statistics, stores the record and -- where a problem
        received observes and has reached t_min -- replaces its table and threshold words by the M-step's.  Enqueued without waiting."""
        h_dT, flat = self._batch_new_observes(new_observes)
        self._chk(self.L.cpprob_hip_batch_advance_learn(self.h, h_dT.ctypes.data_as(C.POINTER(C.c_uint32)), flat.ctypes.data if flat.size else None))
        self.batch_shapes = (self.batch_lengths(), self.batch_shapes[1])

    def batch_advance_learn_device(self, dT, observes):
        """The same with the new observes in a torch float64 device tensor, packed problem after problem (dT: how many each problem
        receives); no host synchronisation."""
        h_dT = np.ascontiguousarray(dT, np.uint32)
        if h_dT.shape != (self.batch_B,):
            raise ValueError("one count per problem")
        self._chk(self.L.cpprob_hip_batch_advance_learn_device(self.h, h_dT.ctypes.data_as(C.POINTER(C.c_uint32)), _dptr(observes), 0 if observes is None else observes.numel()))
        self.batch_shapes = (self.batch_lengths(), self.batch_shapes[1])

    def batch_online_tables(self, tables, emission="normal"):
        """New tables (means [B, k], transition [B, k, k]) for the FUTURE steps of an online MODEL_HMM_TABLE batch, armed or not
        (cpprob_hip_batch_online_tables): validated as the begin validates them; past rows stay.  emission="poisson": (rates,
        transition) for a batch begun with Poisson emissions (cpprob_hip_batch_online_tables_poisson)."""
        poisson = _poisson(emission, tables)
        means, trans = self._batch_tables(tables)
        sigmas = self._batch_sigmas(tables, means)
        if poisson:
            self._chk(self.L.cpprob_hip_batch_online_tables_poisson(self.h, means.ctypes.data, trans.ctypes.data))
        elif sigmas is not None:                               # (a batch begun with emission scales: cpprob_hip_batch_online_tables_scaled)
            self._chk(self.L.cpprob_hip_batch_online_tables_scaled(self.h, means.ctypes.data, trans.ctypes.data, sigmas.ctypes.data))
        else:
            self._chk(self.L.cpprob_hip_batch_online_tables(self.h, means.ctypes.data, trans.ctypes.data))

    def batch_learn_tables(self, k=None, scales=False):
        """(means [B, k], transition [B, k, k], status int32 [B]) of an armed batch as the device holds them: status 0, or the bits
        of batch_retable_status of the last M-step that was dropped.  k: the batch's states (default: those of the last
        batch_begin_online of this engine).  Synchronises.  scales=True (a batch with emission scales): (means, transition, sigmas
        [B, k], status) (cpprob_hip_batch_learn_tables_scaled)."""
        k = int(k if k is not None else self.batch_k)
        means, trans, status = np.zeros((self.batch_B, k)), np.zeros((self.batch_B, k, k)), np.zeros(self.batch_B, np.int32)
        if scales:
            sigmas = np.zeros((self.batch_B, k))
            self._chk(self.L.cpprob_hip_batch_learn_tables_scaled(self.h, means.ctypes.data, trans.ctypes.data, sigmas.ctypes.data, status.ctypes.data_as(C.POINTER(C.c_int32))))
            return means, trans, sigmas, status
        self._chk(self.L.cpprob_hip_batch_learn_tables(self.h, means.ctypes.data, trans.ctypes.data, status.ctypes.data_as(C.POINTER(C.c_int32))))
        return means, trans, status

    def batch_learn_tables_device(self, means, trans, sigmas=None):
        """The same tables into torch float64 device tensors (means [B, k], trans [B, k, k]; sigmas [B, k] of a batch with emission
        scales): a stream-ordered copy."""
        if sigmas is not None:
            self._chk(self.L.cpprob_hip_batch_learn_tables_scaled_device(self.h, _dptr(means), _dptr(trans), _dptr(sigmas)))
        else:
            self._chk(self.L.cpprob_hip_batch_learn_tables_device(self.h, _dptr(means), _dptr(trans)))

    def batch_learn_record(self):
        """float64 [B, 88]: the records of the last learning advance (cpprob_hip_batch_learn_record).  Synchronises."""
        out = np.zeros((self.batch_B, 88))
        self._chk(self.L.cpprob_hip_batch_learn_record(self.h, out.ctypes.data, out.size))
        return out

    def batch_learn_pooled_record(self):
        """float64 [G, 88]: the groups' pooled records of the last tied learning advance (cpprob_hip_batch_learn_pooled_record).
        Synchronises."""
        out = np.zeros((self.batch_tie_get()[1], 88))
        self._chk(self.L.cpprob_hip_batch_learn_pooled_record(self.h, out.ctypes.data, out.size))
        return out

    def batch_step_tables(self, b):
        """Problem b's per-step table as the device holds it: (rows float64 [T_b, 8], threshold words uint64 [64] -- None for
        MODEL_HMM3).  Synchronises."""
        inside = 0 <= int(b) < self.batch_B                  # (an index out of range: the library's own refusal)
        T = self.batch_T if self.batch_shapes is None or not inside else int(self.batch_shapes[0][int(b)])
        rows = np.zeros((T, 8))
        thr = np.zeros(64, np.uint64) if self.batch_K == 8 else None
        self._chk(self.L.cpprob_hip_batch_copy_step_tables(self.h, int(b), rows.ctypes.data, rows.size, None if thr is None else thr.ctypes.data))
        return rows, thr

    def batch_summaries_device(self, out):
        """[B, 4] = {log_evidence, ess_final, log_norm, max_logw} per problem into a torch float64 device tensor; no host sync."""
        if out is None or out.numel() < 4 * self.batch_B:
            raise ValueError("out holds 4 doubles a problem")
        self._chk(self.L.cpprob_hip_batch_summaries_device(self.h, _dptr(out)))

    def batch_results(self, with_stats=True):
        """[summary dict] * B, stats [B, T, spp], ess [B, T], resampled [B, T] in one call and one synchronisation.  with_stats=False:
        stats is None (what an online batch serves between an advance without read-out and the next one with it)."""
        B, T, K = self.batch_B, self.batch_T, self.batch_K
        sums = (Summary * B)()
        stats = np.zeros((B, T, K)) if with_stats else None
        ess = np.zeros((B, T))
        res = np.zeros((B, T), np.int32)
        self._chk(self.L.cpprob_hip_batch_results(self.h, sums, stats.ctypes.data if with_stats else None, stats.size if with_stats else 0, ess.ctypes.data, res.ctypes.data))
        return [{f: getattr(s, f) for f, _ in Summary._fields_} for s in sums], stats, ess, res

    def batch_results_device(self, out):
        """[B, 4 + T spp] = {log_evidence, ess, log_norm, max_logw, stats...} per problem into a device tensor; no host sync."""
        self._chk(self.L.cpprob_hip_batch_results_device(self.h, _dptr(out), out.numel()))

    def batch_store(self, b):
        """Problem b's particle store: (values [T, n] int32, ancestors [T, n] int32, final log-weights [n]); after batch_begin_problems
        T and n are problem b's own."""
        T, n = self.batch_T, self.batch_n
        if self.batch_shapes is not None:
            if not 0 <= int(b) < self.batch_B:
                raise ValueError("problem index out of range")
            T, n = int(self.batch_shapes[0][int(b)]), int(self.batch_shapes[1][int(b)])
        vals = np.zeros((T, n), np.int32)
        anc = np.zeros((T, n), np.int32)
        logw = np.zeros(n)
        self._chk(self.L.cpprob_hip_batch_copy_store(self.h, int(b), vals.ctypes.data, anc.ctypes.data, logw.ctypes.data))
        return vals, anc, logw

    def batch_masses(self, b):
        """Problem b's rows of the m table (cpprob_hip_batch_copy_masses), float64 [T_b, 8]: m_t[s] = cnt_t[s] * fix_weight(ll_t[s], M_t),
        integers below 2^45; a batch begun with keep_masses=True only."""
        inside = 0 <= int(b) < self.batch_B                  # (an index out of range: the library's own refusal)
        T = self.batch_T if self.batch_shapes is None or not inside else int(self.batch_shapes[0][int(b)])
        out = np.zeros((T, 8))
        self._chk(self.L.cpprob_hip_batch_copy_masses(self.h, int(b), out.ctypes.data, out.size))
        return out

    def _batch_problem_shapes(self):
        """(T uint32 [B], n uint32 [B]) of the batch last begun / advanced."""
        if self.batch_shapes is not None:
            return self.batch_shapes
        return np.full(self.batch_B, self.batch_T, np.uint32), np.full(self.batch_B, self.batch_n, np.uint32)

    def batch_paths(self, max_particles=0):
        """The surviving lineages of every problem, resolved on the device in one launch (cpprob_hip_batch_paths): (paths, logw), two
        lists with one entry per problem -- paths[b] int32 [T_b, m_b], the trajectory that ends in final particle i in column i, and
        logw[b] float64 [m_b], its final log-weight; m_b = n_b, or min(n_b, max_particles).  A problem of length 0 (online batch)
        returns [0, m_b] and [0]."""
        h_T, h_n = self._batch_problem_shapes()
        first, wfirst = batch_paths_layout(h_T, h_n, max_particles)
        flat = np.zeros(int(first[-1]), np.int32)
        w = np.zeros(int(wfirst[-1]))
        self._chk(self.L.cpprob_hip_batch_paths(self.h, int(max_particles), flat.ctypes.data, flat.size, w.ctypes.data, w.size))
        paths, logw = [], []
        for b in range(self.batch_B):
            m = int(h_n[b]) if not max_particles else min(int(h_n[b]), int(max_particles))
            paths.append(flat[int(first[b]):int(first[b + 1])].reshape(int(h_T[b]), m))
            logw.append(w[int(wfirst[b]):int(wfirst[b + 1])])
        return paths, logw

    def batch_paths_device(self, paths_i8, logw=None, max_particles=0):
        """The same left in device tensors, enqueued behind the run / advance without a host synchronisation: paths_i8 torch int8,
        logw torch float64 or None, packed as batch_paths_layout(T, n, max_particles) says (their numel() are the capacities)."""
        self._chk(self.L.cpprob_hip_batch_paths_device(self.h, int(max_particles), _dptr(paths_i8), paths_i8.numel(), _dptr(logw), 0 if logw is None else logw.numel()))

    def batch_smooth(self, n_traj=0, draw_index=0):
        """Backward smoothing of every problem (cpprob_hip_batch_smooth): (marginals [B, T_max, spp], the layout of batch_results'
        stats, and a list of int32 [T_b, n_traj] arrays, problem b's backward-simulated trajectories in its columns).  draw_index
        (< 2^16) selects the trajectories' Philox draws: another index, other trajectories; the marginals do not depend on it."""
        h_T, _ = self._batch_problem_shapes()
        first = batch_smooth_layout(h_T, n_traj)
        marg = np.zeros((self.batch_B, self.batch_T, self.batch_K))
        flat = np.zeros(int(first[-1]), np.int32)
        self._chk(self.L.cpprob_hip_batch_smooth(self.h, int(n_traj), int(draw_index), marg.ctypes.data, marg.size, flat.ctypes.data if n_traj else None, flat.size))
        return marg, [flat[int(first[b]):int(first[b + 1])].reshape(int(h_T[b]), int(n_traj)) for b in range(self.batch_B)]

    def batch_smooth_device(self, marginals=None, traj_i8=None, n_traj=0, draw_index=0):
        """The same left in device tensors, enqueued behind the run / advance without a host synchronisation: marginals torch float64
        [B, T_max, spp] or None, traj_i8 torch int8 packed as batch_smooth_layout(T, n_traj) says or None (their numel() are the
        capacities)."""
        self._chk(self.L.cpprob_hip_batch_smooth_device(self.h, int(n_traj), int(draw_index), _dptr(marginals), 0 if marginals is None else marginals.numel(),
                                                        _dptr(traj_i8), 0 if traj_i8 is None else traj_i8.numel()))

    def _batch_lag_shapes(self, lag, from_steps):
        """(L uint32 [B], from uint32 [B] or None, W uint32 [B], n_rows) of a fixed-lag call on the batch last begun / advanced."""
        h_T, _ = self._batch_problem_shapes()
        h_T = np.ascontiguousarray(h_T, np.uint32)
        h_from = None if from_steps is None else np.ascontiguousarray(from_steps, np.uint32)
        if h_from is not None and h_from.shape != h_T.shape:
            raise ValueError("one first step per problem")
        left = h_T.astype(np.int64) - (0 if h_from is None else h_from.astype(np.int64))
        W = np.minimum(int(lag) + 1, h_T.astype(np.int64)).astype(np.uint32)
        return h_T, h_from, W, max(int(left.max()) if left.size else 0, 0)

    def batch_smooth_lag(self, lag, from_steps=None, n_traj=0, draw_index=0):
        """Fixed-lag smoothing of every problem (cpprob_hip_batch_smooth_lag): (marginals [B, n_rows, spp], a list of int32
        [W_b, n_traj] arrays).  Row r of problem b is G_{from_b + r} = P(x_t | y_0 .. y_min(t + lag, L_b - 1)) at t = from_b + r, zero
        past its length; from_steps None: every problem from step 0; n_rows = max(L_b - from_b).  The trajectories are the last
        W_b = min(lag + 1, L_b) rows of batch_smooth(n_traj, draw_index)'s.  On an online batch the call costs the rows asked for,
        whatever length the stream has reached."""
        h_T, h_from, W, n_rows = self._batch_lag_shapes(lag, from_steps)
        first = batch_smooth_layout(W, n_traj)
        marg = np.zeros((self.batch_B, n_rows, self.batch_K))
        flat = np.zeros(int(first[-1]), np.int32)
        self._chk(self.L.cpprob_hip_batch_smooth_lag(self.h, int(lag), None if h_from is None else h_from.ctypes.data_as(C.POINTER(C.c_uint32)), n_rows, int(n_traj),
                                                     int(draw_index), marg.ctypes.data if marg.size else None, marg.size, flat.ctypes.data if n_traj else None, flat.size))
        return marg, [flat[int(first[b]):int(first[b + 1])].reshape(int(W[b]), int(n_traj)) for b in range(self.batch_B)]

    def batch_smooth_lag_device(self, lag, from_steps=None, marginals=None, traj_i8=None, n_traj=0, draw_index=0):
        """The same left in device tensors, enqueued behind the run / advance without a host synchronisation: marginals torch float64
        [B, n_rows, spp] (n_rows = its second dimension) or None, traj_i8 torch int8 packed as batch_smooth_layout(W, n_traj) says or
        None (their numel() are the capacities)."""
        _, h_from, _, n_rows = self._batch_lag_shapes(lag, from_steps)
        if marginals is not None:
            if marginals.dim() != 3:
                raise ValueError("marginals must be [B, n_rows, spp]")
            n_rows = int(marginals.shape[1])
        self._chk(self.L.cpprob_hip_batch_smooth_lag_device(self.h, int(lag), None if h_from is None else h_from.ctypes.data_as(C.POINTER(C.c_uint32)), n_rows, int(n_traj),
                                                            int(draw_index), _dptr(marginals), 0 if marginals is None else marginals.numel(),
                                                            _dptr(traj_i8), 0 if traj_i8 is None else traj_i8.numel()))

    def _batch_packed_observes(self, observes):
        """observes as the statistics calls take them: one flat float64 array, problem after problem by the lengths reached.  A list
        of 1-D arrays (one a problem) or an array [B, T] of a uniform batch."""
        if isinstance(observes, np.ndarray):
            return np.ascontiguousarray(observes, np.float64).reshape(-1)
        seqs = [np.ascontiguousarray(o, np.float64).reshape(-1) for o in observes]
        return np.ascontiguousarray(np.concatenate(seqs)) if seqs else np.zeros(0)

    def batch_smooth_stats(self, observes=None):
        """Expected sufficient statistics of every problem (cpprob_hip_batch_smooth_stats), the E-step of cpprob_amd.em: a dict of
        xi [B, 8, 8] (expected transitions s -> s'), occ [B, 8] (expected visits), occ_y and occ_yy [B, 8] (visits weighted by y_t
        and y_t^2; zero without observes).  observes: a list of 1-D arrays, problem b's sequence up to the length it has reached, or
        an array [B, T] of a uniform batch."""
        rec = np.zeros((self.batch_B, STATS_PER_PROBLEM))
        flat = None if observes is None else self._batch_packed_observes(observes)
        self._chk(self.L.cpprob_hip_batch_smooth_stats(self.h, None if flat is None or flat.size == 0 else flat.ctypes.data, 0 if flat is None else flat.size,
                                                       rec.ctypes.data, rec.size))
        return split_stats(rec)

    def batch_smooth_stats_device(self, stats, observes=None):
        """The same left in a device tensor, enqueued behind the run / advance without a host synchronisation: stats torch float64
        [B, 88] (split_stats names its columns), observes a torch float64 tensor packed as above or None."""
        self._chk(self.L.cpprob_hip_batch_smooth_stats_device(self.h, _dptr(observes), 0 if observes is None else observes.numel(), _dptr(stats), stats.numel()))

    def batch_online_stats(self, new_observes=None):
        """Running sufficient statistics of an online batch (cpprob_hip_batch_online_stats), forward-only: batch_smooth_stats' dict
        -- xi [B, 8, 8], occ, occ_y, occ_yy [B, 8] -- at the lengths reached, for the cost of the steps that arrived since the last
        call (the backward walk of batch_smooth_stats pays every step on every call; in exact arithmetic the two records are equal,
        in doubles they differ by rounding).  new_observes: the observes of the steps the call consumes -- called after every
        batch_advance, that advance's own list of 1-D arrays (or one packed array); None: those steps take y = 0 and add nothing to
        occ_y, occ_yy.  The bits do not depend on how the stream was cut into advances and calls; a call without new steps returns
        the same record again.  cpprob_amd.em.m_step on the result is the running M-step estimate of the tables:

            eng.batch_begin_online(MODEL_HMM_TABLE, capacity, n, seeds, tables=(means, trans))
            for piece in stream:                                   # piece: a list of B arrays
                eng.batch_advance(piece)
                means_now, trans_now = em.m_step(eng.batch_online_stats(piece), means, trans)
        """
        rec = np.zeros((self.batch_B, STATS_PER_PROBLEM))
        flat = None if new_observes is None else self._batch_packed_observes(new_observes)
        self._chk(self.L.cpprob_hip_batch_online_stats(self.h, None if flat is None or flat.size == 0 else flat.ctypes.data, 0 if flat is None else flat.size,
                                                       rec.ctypes.data, rec.size))
        return split_stats(rec)

    def batch_online_stats_device(self, stats, new_observes=None):
        """The same left in a device tensor, enqueued behind the advance without a host synchronisation: stats torch float64 [B, 88]
        (split_stats names its columns), new_observes a torch float64 tensor packed as above or None."""
        self._chk(self.L.cpprob_hip_batch_online_stats_device(self.h, _dptr(new_observes), 0 if new_observes is None else new_observes.numel(), _dptr(stats),
                                                              0 if stats is None else stats.numel()))

    def batch_online_stats_progress(self):
        """The steps of every problem the running statistics have consumed (uint32 [B]); 0 after any begin."""
        out = np.zeros(self.batch_B, np.uint32)
        self._chk(self.L.cpprob_hip_batch_online_stats_progress(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    @staticmethod
    def _traj_stats_args(n_traj, draw_index):
        """The ranges cpprob_hip_batch_traj_stats refuses, checked before anything is allocated."""
        n_traj, draw_index = int(n_traj), int(draw_index)
        if not 1 <= n_traj <= TRAJ_STATS_MAX_TRAJ:
            raise ValueError("n_traj must lie in 1 .. 2^20")
        if not 0 <= draw_index < TRAJ_STATS_MAX_DRAWS:
            raise ValueError("draw_index must lie in 0 .. 2^16 - 1")
        return n_traj, draw_index

    def batch_traj_stats(self, n_traj, draw_index=0, observes=None):
        """Complete-data sufficient statistics of backward-simulated trajectories (cpprob_hip_batch_traj_stats), counted on the
        device: a dict of xi [B, n_traj, 8, 8] (transitions s -> s' of the trajectory), occ [B, n_traj, 8] (visits), occ_y and occ_yy
        [B, n_traj, 8] (the sums of y_t and y_t^2 over the visits; zero without observes).  Trajectory j of problem b is column j of
        batch_smooth(n_traj, draw_index)'s trajectories; it is not stored.  observes: as batch_smooth_stats takes them.
        cpprob_amd.gibbs samples the tables from these records."""
        n_traj, draw_index = self._traj_stats_args(n_traj, draw_index)
        rec = np.zeros((self.batch_B, n_traj, STATS_PER_PROBLEM))
        flat = None if observes is None else self._batch_packed_observes(observes)
        self._chk(self.L.cpprob_hip_batch_traj_stats(self.h, n_traj, draw_index, None if flat is None or flat.size == 0 else flat.ctypes.data,
                                                     0 if flat is None else flat.size, rec.ctypes.data, rec.size))
        return split_traj_stats(rec)

    def batch_traj_stats_device(self, stats, n_traj, draw_index=0, observes=None):
        """The same left in a device tensor, enqueued behind the run / advance without a host synchronisation: stats torch float64
        [B, n_traj, 88] (split_traj_stats names its columns), observes a torch float64 tensor packed as above or None."""
        n_traj, draw_index = self._traj_stats_args(n_traj, draw_index)
        self._chk(self.L.cpprob_hip_batch_traj_stats_device(self.h, n_traj, draw_index, _dptr(observes), 0 if observes is None else observes.numel(),
                                                            _dptr(stats), stats.numel()))

    def batch_traj_stats_grid(self):
        """gridDim.y of the last trajectory statistics launch (cpprob_hip_batch_traj_stats_grid): the tiles of TRAJ_STATS_TILE
        trajectories a problem, 0 where none happened."""
        gy = C.c_uint32(0)
        self._chk(self.L.cpprob_hip_batch_traj_stats_grid(self.h, C.byref(gy)))
        return int(gy.value)

    @staticmethod
    def _forecast_args(horizon, n_traj, draw_index):
        """The ranges cpprob_hip_batch_forecast refuses, checked before anything is allocated."""
        horizon, n_traj, draw_index = int(horizon), int(n_traj), int(draw_index)
        if not 1 <= horizon < FORECAST_MAX_HORIZON:
            raise ValueError("horizon must lie in 1 .. 2^24 - 1")
        if not 0 <= n_traj <= FORECAST_MAX_TRAJ:
            raise ValueError("n_traj must lie in 0 .. 2^20")
        if not 0 <= draw_index < FORECAST_MAX_DRAWS:
            raise ValueError("draw_index must lie in 0 .. 2^16 - 1")
        return horizon, n_traj, draw_index

    def batch_forecast(self, horizon, n_traj=0, draw_index=0):
        """Forecasts of every problem (cpprob_hip_batch_forecast): (marginals [B, horizon, spp], row h - 1 the law of the state h
        steps past the last observe, P(x_{L-1+h} | y_0 .. y_{L-1}); trajectories int32 [B, horizon + 1, n_traj], simulated futures
        whose row 0 is the present state).  A problem of length 0 has rows of zeros.  draw_index (< 2^16) selects the trajectories'
        Philox draws; the marginals do not depend on it.  cpprob_amd.forecast.observation_forecast turns the marginals into the
        forecast of the observe itself."""
        horizon, n_traj, draw_index = self._forecast_args(horizon, n_traj, draw_index)
        marg = np.zeros((self.batch_B, horizon, self.batch_K))
        traj = np.zeros((self.batch_B, horizon + 1, n_traj), np.int32)
        self._chk(self.L.cpprob_hip_batch_forecast(self.h, horizon, n_traj, draw_index, marg.ctypes.data, marg.size, traj.ctypes.data if n_traj else None, traj.size))
        return marg, traj

    def batch_forecast_device(self, horizon, marginals=None, traj_i8=None, n_traj=0, draw_index=0):
        """The same left in device tensors, enqueued behind the run / advance without a host synchronisation: marginals torch float64
        [B, horizon, spp] or None, traj_i8 torch int8 [B, horizon + 1, n_traj] or None (their numel() are the capacities)."""
        horizon, n_traj, draw_index = self._forecast_args(horizon, n_traj, draw_index)
        self._chk(self.L.cpprob_hip_batch_forecast_device(self.h, horizon, n_traj, draw_index, _dptr(marginals), 0 if marginals is None else marginals.numel(),
                                                          _dptr(traj_i8), 0 if traj_i8 is None else traj_i8.numel()))

    def _batch_predictive_shapes(self, from_steps):
        """(from uint32 [B] or None, n_rows) of a predictive call on the batch last begun / advanced."""
        h_T, _ = self._batch_problem_shapes()
        h_T = np.ascontiguousarray(h_T, np.uint32)
        if from_steps is None:
            return None, (int(h_T.max()) if h_T.size else 0) + 1
        f = np.asarray(from_steps)
        if f.shape != h_T.shape:
            raise ValueError("one first step per problem")
        if f.size and (f.min() < 0 or f.max() >= 1 << 32):
            raise ValueError("from_steps must be steps, 0 .. 2^32 - 1")
        h_from = np.ascontiguousarray(f, np.uint32)
        left = h_T.astype(np.int64) + 1 - h_from.astype(np.int64)
        return h_from, max(int(left.max()) if left.size else 0, 0)

    def batch_predictive(self, from_steps=None):
        """One-step predictive rows of every problem (cpprob_hip_batch_predictive): [B, n_rows, spp]; row r of problem b is
        P(x_t | y_0 .. y_{t-1}) at t = from_b + r <= L_b (t = 0: the uniform initial law; t = L_b: the forecast's first row), zero
        past it.  from_steps None: every problem from step 0; n_rows = max(L_b + 1 - from_b).
        cpprob_amd.forecast.predictive_log_likelihood scores the observes with them."""
        h_from, n_rows = self._batch_predictive_shapes(from_steps)
        rows = np.zeros((self.batch_B, n_rows, self.batch_K))
        if rows.size == 0:
            return rows
        self._chk(self.L.cpprob_hip_batch_predictive(self.h, None if h_from is None else h_from.ctypes.data_as(C.POINTER(C.c_uint32)), n_rows, rows.ctypes.data, rows.size))
        return rows

    def batch_predictive_device(self, rows, from_steps=None):
        """The same left in a device tensor, enqueued behind the run / advance without a host synchronisation: rows torch float64
        [B, n_rows, spp] (n_rows = its second dimension)."""
        if rows is None or rows.dim() != 3:
            raise ValueError("rows must be [B, n_rows, spp]")
        h_from, _ = self._batch_predictive_shapes(from_steps)
        self._chk(self.L.cpprob_hip_batch_predictive_device(self.h, None if h_from is None else h_from.ctypes.data_as(C.POINTER(C.c_uint32)), int(rows.shape[1]),
                                                            _dptr(rows), rows.numel()))

    def batch_decode(self):
        """The most probable state path of every problem given its observes (cpprob_hip_batch_decode): (a list of int32 [L_b] arrays,
        scores float64 [B]) -- dynamic programming over the states the particles occupy, under the transition law the device draws
        from; the score is the log joint density of the path and the observes.  A problem of length 0 has an empty path and score 0."""
        h_T, _ = self._batch_problem_shapes()
        first = batch_smooth_layout(h_T, 1)
        flat = np.zeros(int(first[-1]), np.int32)
        score = np.zeros(self.batch_B)
        self._chk(self.L.cpprob_hip_batch_decode(self.h, flat.ctypes.data if flat.size else None, flat.size, score.ctypes.data, score.size))
        return [flat[int(first[b]):int(first[b + 1])] for b in range(self.batch_B)], score

    def batch_decode_device(self, path_i8=None, score=None):
        """The same left in device tensors, enqueued behind the run / advance without a host synchronisation: path_i8 torch int8
        packed as batch_smooth_layout(T, 1) says or None, score torch float64 [B] or None (their numel() are the capacities)."""
        self._chk(self.L.cpprob_hip_batch_decode_device(self.h, _dptr(path_i8), 0 if path_i8 is None else path_i8.numel(), _dptr(score), 0 if score is None else score.numel()))

    def _batch_decode_lag_shapes(self, lag, from_steps):
        """(from uint32 [B] or None, n_rows) of a fixed-lag decode on the batch last begun / advanced; the ranges the library refuses
        are checked before anything is allocated."""
        if not 0 <= int(lag) <= DECODE_MAX_LAG:
            raise ValueError("lag must lie in 0 .. 2^24")
        if from_steps is not None:
            f = np.asarray(from_steps)
            if f.size and (f.min() < 0 or f.max() >= 1 << 32):
                raise ValueError("from_steps must be steps, 0 .. 2^32 - 1")
        _, h_from, _, n_rows = self._batch_lag_shapes(lag, from_steps)
        return h_from, n_rows

    def batch_decode_lag(self, lag, from_steps=None):
        """Fixed-lag decoding of every problem (cpprob_hip_batch_decode_lag): (states int32 [B, n_rows], scores float64 [B]).  Row r
        of problem b is X_t at t = from_b + r, the state at t of the most probable path of steps 0 .. min(t + lag, L_b - 1) -- final
        once lag more observes have arrived --, and -1 past its length; from_steps None: every problem from step 0;
        n_rows = max(L_b - from_b).  The rows with t + lag >= L_b - 1 are batch_decode's."""
        h_from, n_rows = self._batch_decode_lag_shapes(lag, from_steps)
        states = np.full((self.batch_B, n_rows), -1, np.int32)
        score = np.zeros(self.batch_B)
        self._chk(self.L.cpprob_hip_batch_decode_lag(self.h, int(lag), None if h_from is None else h_from.ctypes.data_as(C.POINTER(C.c_uint32)), n_rows,
                                                     states.ctypes.data if states.size else None, states.size, score.ctypes.data, score.size))
        return states, score

    def batch_decode_lag_device(self, lag, states_i8=None, score=None, from_steps=None):
        """The same left in device tensors, enqueued behind the run / advance without a host synchronisation: states_i8 torch int8
        [B, n_rows] (n_rows = its second dimension) or None, score torch float64 [B] or None."""
        h_from, n_rows = self._batch_decode_lag_shapes(lag, from_steps)
        if states_i8 is not None:
            if states_i8.dim() != 2:
                raise ValueError("states_i8 must be [B, n_rows]")
            n_rows = int(states_i8.shape[1])
        self._chk(self.L.cpprob_hip_batch_decode_lag_device(self.h, int(lag), None if h_from is None else h_from.ctypes.data_as(C.POINTER(C.c_uint32)), n_rows,
                                                            _dptr(states_i8), 0 if states_i8 is None else states_i8.numel(), _dptr(score), 0 if score is None else score.numel()))

    def batch_decode_logp(self, b):
        """(lp float64 [8, 8], lp0) of problem b (cpprob_hip_batch_decode_logp): lp[s, s'] = log P(s -> s') under the transition law the
        device realises (-inf where it is 0 or outside the k states), lp0 = log(1 / k): the doubles the decode kernels are given.
        Host only."""
        lp = np.zeros(64)
        lp0 = C.c_double(0.0)
        self._chk(self.L.cpprob_hip_batch_decode_logp(self.h, int(b), lp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(lp0)))
        return lp.reshape(8, 8), float(lp0.value)

    def batch_smooth_grid(self):
        """(gridDim.y of the counting launch, gridDim.y of the fixed-lag launch) of this context's last smoothing call
        (cpprob_hip_batch_smooth_grid); 0 where the launch did not happen.  Host only."""
        cy, ly = C.c_uint32(0), C.c_uint32(0)
        self._chk(self.L.cpprob_hip_batch_smooth_grid(self.h, C.byref(cy), C.byref(ly)))
        return int(cy.value), int(ly.value)

    def batch_pass_grid(self):
        """(gridDim.x of the decode's forward launch, gridDim.y of its traceback launch, gridDim.y of the forecast launch, gridDim.y of
        the predictive launch) of this context's last decode / forecast / predictive call (cpprob_hip_batch_pass_grid); 0 where the
        launch did not happen.  Host only."""
        g = [C.c_uint32(0) for _ in range(4)]
        self._chk(self.L.cpprob_hip_batch_pass_grid(self.h, *[C.byref(x) for x in g]))
        return tuple(int(x.value) for x in g)

    # ---- sharded SMC ---------------------------------------------------------------------
    def step_begin(self, t, local_totals, run_index=0):
        """local_totals: torch float64 tensor (>= 3) on this device, filled on the engine's stream."""
        self._chk(self.L.cpprob_hip_smc_step_begin(self.h, int(t), int(run_index), _dptr(local_totals)))

    def step_end(self, t, all_totals, world, rank):
        self._chk(self.L.cpprob_hip_smc_step_end(self.h, int(t), _dptr(all_totals), int(world), int(rank)))

    def finish(self):
        self._chk(self.L.cpprob_hip_smc_finish(self.h))

    def first_bad_generation(self):
        """After finish(): the first generation whose fixed-point weights lost their bits (-1: none) and the run's largest gap in nats."""
        g, gap = C.c_int32(-1), C.c_double(0.0)
        self._chk(self.L.cpprob_hip_smc_first_bad_generation(self.h, C.byref(g), C.byref(gap)))
        return int(g.value), float(gap.value)

    def repair_begin(self, g, local3):
        self._chk(self.L.cpprob_hip_smc_repair_begin(self.h, int(g), _dptr(local3)))

    def repair_end(self, g, all3, world, rank, local3):
        self._chk(self.L.cpprob_hip_smc_repair_end(self.h, int(g), _dptr(all3), int(world), int(rank), _dptr(local3)))

    # ---- exchange scope: exact global resampling with migration ----------------------------
    def exchange_plan(self, t, world, rank, shard_begin):
        """-> (do_resample, send_counts[world], recv_counts[world]) in lineage records of t + 1 values.  Host-synchronising."""
        sb = np.ascontiguousarray(shard_begin, dtype=np.uint64)
        send = np.zeros(world, np.uint64)
        recv = np.zeros(world, np.uint64)
        flag = C.c_int32(0)
        self._chk(self.L.cpprob_hip_exchange_plan(self.h, int(t), int(world), int(rank), sb.ctypes.data, send.ctypes.data, recv.ctypes.data, C.byref(flag)))
        return bool(flag.value), send, recv

    def exchange_traffic(self):
        """(records sent after each step [T], total records, total bytes) of this rank's last exchange-scope run on a fixed transport."""
        per = np.zeros(self.T, np.int64)
        rec, byt = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.L.cpprob_hip_exchange_traffic(self.h, per.ctypes.data, per.size, C.byref(rec), C.byref(byt)))
        return per, int(rec.value), int(byt.value)

    def exchange_pack(self, t, send):
        self._chk(self.L.cpprob_hip_exchange_pack(self.h, int(t), _dptr(send) if send is not None else None))

    def exchange_commit(self, t, recv):
        self._chk(self.L.cpprob_hip_exchange_commit(self.h, int(t), _dptr(recv) if recv is not None else None))

    # ---- building blocks (torch tensors on this device carry the memory) -------------------
    def philox_blocks(self, seed, pid0, draw, out):
        self._chk(self.L.cpprob_hip_philox_blocks(self.h, seed, pid0, draw, out.numel() // 4, _dptr(out)))

    def draw_normal(self, seed, pid0, draw, mean, sigma, out):
        self._chk(self.L.cpprob_hip_draw_normal(self.h, seed, pid0, draw, mean, sigma, out.numel(), _dptr(out)))

    def draw_uniform_smallint(self, seed, pid0, draw, a, b, out):
        self._chk(self.L.cpprob_hip_draw_uniform_smallint(self.h, seed, pid0, draw, a, b, out.numel(), _dptr(out)))

    def draw_discrete(self, seed, pid0, draw, weights, out):
        w = (C.c_double * len(weights))(*weights)
        self._chk(self.L.cpprob_hip_draw_discrete(self.h, seed, pid0, draw, w, len(weights), out.numel(), _dptr(out)))

    def draw_uniform_real(self, seed, pid0, draw, a, b, out):
        self._chk(self.L.cpprob_hip_draw_uniform_real(self.h, seed, pid0, draw, a, b, out.numel(), _dptr(out)))

    def draw_poisson(self, seed, pid0, draw, mean, out):
        self._chk(self.L.cpprob_hip_draw_poisson(self.h, seed, pid0, draw, mean, out.numel(), _dptr(out)))

    def logpdf_normal(self, x, mean, sigma, out):
        self._chk(self.L.cpprob_hip_logpdf_normal(self.h, _dptr(x), _dptr(mean), _dptr(sigma), x.numel(), _dptr(out)))

    def logpdf_uniform_real(self, x, a, b, out):
        self._chk(self.L.cpprob_hip_logpdf_uniform_real(self.h, _dptr(x), _dptr(a), _dptr(b), x.numel(), _dptr(out)))

    def logpdf_poisson(self, x, mean, out):
        self._chk(self.L.cpprob_hip_logpdf_poisson(self.h, _dptr(x), _dptr(mean), x.numel(), _dptr(out)))

    def logpdf_uniform_smallint(self, x, a, b, out):
        self._chk(self.L.cpprob_hip_logpdf_uniform_smallint(self.h, _dptr(x), a, b, x.numel(), _dptr(out)))

    def logpdf_discrete(self, x, weights, out):
        w = (C.c_double * len(weights))(*weights)
        self._chk(self.L.cpprob_hip_logpdf_discrete(self.h, _dptr(x), w, len(weights), x.numel(), _dptr(out)))

    def fastmath(self, which, x, out0, out1=None):
        """which: 0 log01, 1 sincospi02 (out0 = sin, out1 = cos), 2 exp_nonpos, 3 fix_weight against reference 0; torch float64 tensors on this device."""
        self._chk(self.L.cpprob_hip_fastmath(self.h, int(which), _dptr(x), x.numel(), _dptr(out0), _dptr(out1)))

    def variate_from_bits(self, which, params, blocks, out0, out1=None):
        """The library's variate generators on chosen Philox blocks: blocks is an [n, 4] tensor of 32-bit words, which one of VARIATE_*,
        params its parameters ((a, b), the weights, (a, b), (mean,), ()); float64 results in out0 (and out1: normal's second output)."""
        p = (C.c_double * max(1, len(params)))(*params)
        self._chk(self.L.cpprob_hip_variate_from_bits(self.h, int(which), p, len(params), _dptr(blocks), blocks.numel() // 4, _dptr(out0), _dptr(out1)))

    def logsumexp_ess(self, logw):
        out = (C.c_double * 3)()
        self._chk(self.L.cpprob_hip_logsumexp_ess(self.h, _dptr(logw), logw.numel(), out))
        return tuple(out)

    def weighted_moments(self, x, logw):
        out = (C.c_double * 4)()
        self._chk(self.L.cpprob_hip_weighted_moments(self.h, _dptr(x), _dptr(logw), logw.numel(), out))
        return tuple(out)

    def weighted_hist(self, x, logw, k):
        out = (C.c_double * 8)()
        self._chk(self.L.cpprob_hip_weighted_hist(self.h, _dptr(x), _dptr(logw), logw.numel(), k, out))
        return np.array(out[:k])

    def weighted_moments_columns(self, x, logw):
        """x: [n_cols, n] device tensor (contiguous rows) -> array [n_cols, 4] of (mean, variance, logsumexp, ess)."""
        n_cols, n = int(x.shape[0]), int(x.shape[1])
        out = (C.c_double * (4 * n_cols))()
        self._chk(self.L.cpprob_hip_weighted_moments_columns(self.h, _dptr(x), n_cols, n, _dptr(logw), n, out))
        return np.array(out[:]).reshape(n_cols, 4)

    def weighted_hist_columns(self, x, logw, k):
        """x: [n_cols, n] int32 device tensor -> array [n_cols, k] of P(x = s)."""
        n_cols, n = int(x.shape[0]), int(x.shape[1])
        out = (C.c_double * (k * n_cols))()
        self._chk(self.L.cpprob_hip_weighted_hist_columns(self.h, _dptr(x), n_cols, n, _dptr(logw), n, k, out, None))
        return np.array(out[:]).reshape(n_cols, k)

    def lineage_gather(self, anc, resampled, cols, gens, out):
        """anc [T, n] int32, resampled [T] int32, cols [H, n] (fp64 / int32) recorded in generations gens[h]; out [H, n]: the traces."""
        T, n = int(anc.shape[0]), int(anc.shape[1])
        g = (C.c_int32 * len(gens))(*gens)
        self._chk(self.L.cpprob_hip_lineage_gather(self.h, _dptr(anc), _dptr(resampled), T, n, _dptr(cols), 0 if cols.dtype.is_floating_point else 1, g, len(gens), _dptr(out)))

    def lineage_moments(self, anc, resampled, cols, gens, logw):
        """-> array [H, 4] = {mean, variance, logsumexp, ess} of every record along the final particles' lineages."""
        T, n = int(anc.shape[0]), int(anc.shape[1])
        g = (C.c_int32 * len(gens))(*gens)
        out = (C.c_double * (4 * len(gens)))()
        self._chk(self.L.cpprob_hip_lineage_moments(self.h, _dptr(anc), _dptr(resampled), T, n, _dptr(cols), g, len(gens), _dptr(logw), out))
        return np.array(out[:]).reshape(len(gens), 4)

    def lineage_hist(self, anc, resampled, cols, gens, logw, k):
        """-> array [H, k] of P(record h = s) along the final particles' lineages."""
        T, n = int(anc.shape[0]), int(anc.shape[1])
        g = (C.c_int32 * len(gens))(*gens)
        out = (C.c_double * (k * len(gens)))()
        self._chk(self.L.cpprob_hip_lineage_hist(self.h, _dptr(anc), _dptr(resampled), T, n, _dptr(cols), g, len(gens), _dptr(logw), k, out, None))
        return np.array(out[:]).reshape(len(gens), k)

    def readback_with_next_result(self, src, out):
        """Hang a read-back of device tensor `src` into the numpy array `out` on the next lineage_moments / lineage_hist call (one wait for both)."""
        self._chk(self.L.cpprob_hip_readback_with_next_result(self.h, _dptr(src), out.ctypes.data, out.nbytes))

    def resample(self, kind, logw, seed, step, anc_out, j0=0, n_total_out=None):
        n_out = anc_out.numel()
        nt = logw.numel() if n_total_out is None else n_total_out
        self._chk(self.L.cpprob_hip_resample(self.h, kind, _dptr(logw), logw.numel(), seed, step, j0, n_out, nt, _dptr(anc_out)))

    def smc_bookkeep(self, kind, logw, seed, step, last, ess_frac, ess, resampled, log_z, anc):
        """Device-side SMC bookkeeping of one step (all tensors on this device; no host sync)."""
        self._chk(self.L.cpprob_hip_smc_bookkeep(self.h, kind, _dptr(logw), logw.numel(), seed, int(step), 1 if last else 0, float(ess_frac),
                                                 _dptr(ess), _dptr(resampled), _dptr(log_z), _dptr(anc)))

    def smc_bookkeep_fixed(self, logw, seed, step, last, ess_frac, ess, resampled, log_z, anc):
        """The same for systematic resampling on fixed-point weights (integer masses; cpprob_hip_smc_bookkeep_fixed)."""
        self._chk(self.L.cpprob_hip_smc_bookkeep_fixed(self.h, _dptr(logw), logw.numel(), seed, int(step), 1 if last else 0, float(ess_frac),
                                                       _dptr(ess), _dptr(resampled), _dptr(log_z), _dptr(anc)))

    def gather(self, src, idx, dst):
        import torch
        fn = self.L.cpprob_hip_gather_f64 if src.dtype == torch.float64 else self.L.cpprob_hip_gather_i32
        self._chk(fn(self.h, _dptr(src), _dptr(idx), idx.numel(), _dptr(dst)))

    def profile_enable(self, on=True):
        self._chk(self.L.cpprob_hip_profile_enable(self.h, 1 if on else 0))

    def profile_read(self, reset=True):
        ms = (C.c_double * N_KERNEL_CLASSES)()
        calls = (C.c_int64 * N_KERNEL_CLASSES)()
        self._chk(self.L.cpprob_hip_profile_read(self.h, ms, calls, 1 if reset else 0))
        return {KERNEL_CLASS_NAMES[k]: (ms[k], calls[k]) for k in range(N_KERNEL_CLASSES)}


class Group:
    """One joint population over several GPUs, driven by the library's own host code (cpprob_amd/csrc/group.hpp): the
    exchange scope's per-step protocol with RCCL collectives on each context's stream and no host synchronisation inside a
    run.  devices: this process's GPUs.  world > len(devices): one rank of a multi-process group (unique_id from
    Group.unique_id() on rank 0, distributed by the launcher).  All devices equal: loopback (every rank on that one GPU)."""

    def __init__(self, devices, world=None, first_rank=0, unique_id=None, allgather=None):
        """allgather(bytes_in) -> bytes of every rank in rank order: the caller's own collective (cpprob_hip_group_create_external);
        then devices = [this rank's GPU], world and first_rank (= rank) as given."""
        self.L = load_library()
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        world = len(devices) if world is None else int(world)
        h = C.c_void_p()
        if allgather is not None:
            def _cb(user, h_in, h_out, nbytes):
                try:
                    out = allgather(C.string_at(h_in, nbytes))
                    if len(out) != nbytes * world:
                        return 1
                    C.memmove(h_out, out, len(out))
                    return 0
                except Exception:        # noqa: reported as a failed collective
                    return 1
            self._cb = ALLGATHER_FN(_cb)              # (kept alive with the group)
            self._coll = Collectives(None, self._cb)
            rc = self.L.cpprob_hip_group_create_external(int(devices[0]), world, int(first_rank), C.byref(self._coll), C.byref(h))
        else:
            uid = C.create_string_buffer(bytes(unique_id), 128) if unique_id is not None else None
            rc = self.L.cpprob_hip_group_create(devs, len(devices), world, int(first_rank), uid, C.byref(h))
        if rc:
            msg = self.L.cpprob_hip_group_last_error(None)
            raise CpprobHipError("cpprob_hip_group_create failed (%d): %s" % (rc, msg.decode() if msg else "?"))
        self.h = h
        self.world, self.n_local, self.first_rank = world, len(devices), int(first_rank)
        self.T = self.K = 0
        self.is_int = False

    @staticmethod
    def unique_id():
        L = load_library()
        buf = C.create_string_buffer(128)
        rc = L.cpprob_hip_group_unique_id(buf, 128)
        if rc:
            msg = L.cpprob_hip_group_last_error(None)
            raise CpprobHipError("cpprob_hip_group_unique_id failed (%d): %s" % (rc, msg.decode() if msg else "?"))
        return buf.raw

    def close(self):
        if getattr(self, "h", None):
            self.L.cpprob_hip_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            msg = self.L.cpprob_hip_group_last_error(self.h)
            raise CpprobHipError("cpprob_hip group error %d: %s" % (rc, msg.decode() if msg else "?"))

    def begin(self, algorithm, model, observes, n_particles, seed=12345, resampler=RESAMPLE_SYSTEMATIC, ess_threshold=2.0, shard_sizes=None, flags=0,
              keep_history=True):
        """n_particles = the whole population."""
        obs = np.ascontiguousarray(observes, np.float64)
        cfg = Config(algorithm, model, resampler, SCOPE_EXCHANGE, 1 if keep_history else 0, 0, int(flags), 0, float(ess_threshold), int(seed), int(n_particles), 0,
                     int(n_particles))
        ss = None
        if shard_sizes is not None:
            ss = np.ascontiguousarray(shard_sizes, np.uint64)
            assert len(ss) == self.world
        self._chk(self.L.cpprob_hip_group_begin(self.h, C.byref(cfg), obs.ctypes.data_as(C.POINTER(C.c_double)), len(obs),
                                                ss.ctypes.data if ss is not None else None))
        gauss = model in (MODEL_GAUSSIAN_UNKNOWN_MEAN, MODEL_GAUSSIAN_README)
        self.T = 1 if gauss else len(obs)
        self.is_int = model in (MODEL_HMM3, MODEL_HMM_TABLE)
        self.K = 8 if model == MODEL_HMM_TABLE else (3 if self.is_int else 2)
        self.n = int(n_particles)
        return self

    def transport(self, records_per_peer=0, all_peers=-1, flags=0):
        """Transport parameters of the next begin() (0 / -1: the defaults; flags: GROUP_SENDRECV, GROUP_WORLD1_COLLECTIVES)."""
        self._chk(self.L.cpprob_hip_group_transport(self.h, int(records_per_peer), int(all_peers), int(flags)))

    PHASES = ["step_and_totals", "allgather", "totals_handover", "pack", "barrier", "commit", "mailbox_wait"]

    def profile(self, on=True):
        """HIP events between the launches of every step of the following runs (cpprob_hip_group_profile)."""
        self._chk(self.L.cpprob_hip_group_profile(self.h, 1 if on else 0))

    def profile_read(self):
        """Microseconds per rank-step of the last (profiled) run, by phase; 'steps' = steps timed."""
        out = (C.c_double * 8)()
        self._chk(self.L.cpprob_hip_group_profile_read(self.h, out))
        d = {k: out[i] for i, k in enumerate(self.PHASES)}
        d["steps"] = int(out[7])
        return d

    def note(self):
        """Which collectives / transport the group settled on, and why."""
        return self.L.cpprob_hip_group_note(self.h).decode()

    def traffic(self):
        """Of the run results() last collected: dict of records, payload_bytes, wire_bytes, collective_bytes, transport."""
        t = Traffic()
        self._chk(self.L.cpprob_hip_group_traffic(self.h, C.byref(t)))
        return {f: getattr(t, f) for f, _ in Traffic._fields_}

    def run(self, run_index=0):
        self._chk(self.L.cpprob_hip_group_run(self.h, int(run_index)))

    def sync(self):
        self._chk(self.L.cpprob_hip_group_sync(self.h))

    def results(self):
        """(stats[T, K], summary dict, reruns): the joint population's numbers, as one GPU holding all particles would report them."""
        s = Summary()
        out = np.zeros((self.T, self.K))
        rr = C.c_int32(0)
        self._chk(self.L.cpprob_hip_group_results(self.h, C.byref(s), out.ctypes.data_as(C.POINTER(C.c_double)), out.size, C.byref(rr)))
        return out, {f: getattr(s, f) for f, _ in Summary._fields_}, int(rr.value)

    def context(self, local_index):
        """The rank's context as an Engine view (not owned): shard-level read-outs (paths, values, logw)."""
        e = Engine.__new__(Engine)
        e.L = self.L
        e.h = C.c_void_p(self.L.cpprob_hip_group_context(self.h, int(local_index)))
        e.device = None
        e.T, e.K, e.is_int = self.T, self.K, self.is_int
        e.close = lambda: None
        return e
