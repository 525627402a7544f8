"""icp_amd — Python mirror of the reference's src/GPU interface over libicp_hip.so.

The product is the C-ABI library (include/icp_capi.h) built from csrc/; this module only
binds it with ctypes so tests, bench.py and the graft entry point can drive it.  Names
follow the reference (yassram/iterative-closest-point):

  ICP(m, p, max_iter).find_corresponding_opti()   src/GPU/gpu.cc:52-83
  ICP.find_alignment(y)                            src/GPU/gpu.cc:95-151
  compute_Y_w_opti(m, p)                           src/GPU/compute.cu:154-245
  compute_err_w(Y, p, in_place, sr, t)             src/GPU/compute.cu:348-379
  compute_centroid(M)  (mean + substract_col_w)   src/GPU/compute.cu:400-416
  y_p_norm_w(y, p)                                 src/GPU/compute.cu:442-469
  load_matrix / write_matrix                       src/load.cc:3-97

Clouds are numpy float64 arrays of shape (n, 3) here (row = point).  That is the same
memory as the reference's 3 x n column-major Eigen matrix, so no copy is needed at the
C boundary.  There is NO CPU fallback: if libicp_hip.so is missing or no HIP device is
visible, every compute call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ICP_AMD_LIB") or os.path.join(_HERE, "build", "libicp_hip.so")

ICP_OK = 0
ICP_E_ARG = -1
ICP_E_HIP = -2
ICP_E_SIZE_MISMATCH = -3
ICP_E_TOO_FEW_POINTS = -4
ICP_E_NO_MODEL = -5
ICP_E_RCCL = -6
ICP_E_NO_DEVICE = -7
ICP_E_IO = -8
ICP_E_RANGE = -9
ICP_E_DEGENERATE = -10  # point-to-plane: an iteration's 6 x 6 system is singular; ransac_pose: no sample kept

NN_CERTIFIED = 0
NN_FP64 = 1
VARIANT_AUTO = 0
VARIANT_VALU = 1
VARIANT_MFMA = 2
VARIANT_MFMA16 = 3
VARIANT_GRID = 4  # exact grid NN for every query
VARIANT_BUNDLE = 5  # f16 pair filter behind the per-(query, 32-point bundle) MFMA bound
RULE_SQUARED = 0    # icp_set_nn_rule: the reference GPU path's squared distance (default)
RULE_CPU_SQRT = 1   # the reference CPU path's sqrt(pow) distance (src/cpu.cc:17-22)
RUN_AUTO = 0        # icp_set_run_mode: one launch for eligible small runs, else the launch loop
RUN_LAUNCHES = 1
RUN_PERSISTENT = 2
METRIC_POINT_TO_POINT = 0  # icp_set_metric: Horn's closed form, scale included (the default)
METRIC_POINT_TO_PLANE = 1  # the distance along the model's normals (set_model_normals), no scale
ROBUST_NONE = 0    # icp_set_robust: every kept pair with weight 1 (the default)
ROBUST_HUBER = 1   # w = 1 within k, k / |r| beyond
ROBUST_TUKEY = 2   # w = (1 - r^2/k^2)^2 within k, 0 beyond
ROBUST_CAUCHY = 3  # w = 1 / (1 + r^2/k^2)

# every function include/icp_capi.h declares (checked by tests/test_capi.py)
EXPORTED = [
    "icp_ctx_create", "icp_ctx_create_dist", "icp_rccl_unique_id", "icp_ctx_create_sharded",
    "icp_ctx_destroy",
    "icp_last_error", "icp_strerror", "icp_device_count", "icp_set_model", "icp_set_scene",
    "icp_set_model_device", "icp_set_scene_device", "icp_set_model_device_stream",
    "icp_set_scene_device_stream", "icp_set_progress",
    "icp_get_scene", "icp_set_allow_unequal", "icp_set_nn_variant", "icp_run", "icp_closest_matrix",
    "icp_compute_centroid", "icp_y_p_norm", "icp_err_compute", "icp_find_alignment",
    "icp_horn_solve", "icp_max_element_index", "icp_shard_range", "icp_synthetic_pair",
    "icp_load_matrix", "icp_write_matrix", "icp_free", "icp_get_stats", "icp_reset_stats",
    "icp_ensure_model", "icp_subtract_col", "icp_get_indices", "icp_set_index_digest",
    "icp_get_index_digest", "icp_set_cert_audit", "icp_set_run_mode", "icp_set_nn_rule",
    "icp_get_comm_info", "icp_set_bundle_counters", "icp_get_bundle_counters", "icp_get_model_order",
    "icp_bundle_audit", "icp_sort_pairs", "icp_get_grid", "icp_debug_live_buffers",
    "icp_set_max_distance", "icp_get_inliers", "icp_get_inlier_trace",
    "icp_set_metric", "icp_set_model_normals", "icp_set_model_normals_device",
    "icp_model_knn", "icp_estimate_model_normals", "icp_get_model_normals",
    "icp_set_robust", "icp_get_robust_trace",
    "icp_voxel_downsample", "icp_voxel_downsample_device", "icp_get_transform", "icp_transform_scene",
    "icp_set_trim", "icp_get_trim_trace", "icp_select_kth",
    "icp_set_plane_symmetric", "icp_set_scene_normals", "icp_set_scene_normals_device", "icp_get_scene_normals",
    "icp_estimate_scene_normals", "icp_set_plane_to_plane",
    "icp_set_one_to_one",
    "icp_fpfh", "icp_match_features", "icp_match_features_plan", "icp_ransac_pose", "icp_global_pose",
    "icp_filter_statistical", "icp_filter_statistical_device", "icp_filter_radius", "icp_filter_radius_device",
    "icp_evaluate", "icp_evaluate_device",
]


class ICPError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{msg} (code {code})")
        self.code = code


class Result(C.Structure):
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("err", C.c_double),
                ("s", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3)]


class Stats(C.Structure):
    _fields_ = [("nn_ms", C.c_double), ("nn_launches", C.c_longlong), ("nn_pairs", C.c_longlong),
                ("ambiguous", C.c_longlong), ("level1_queued", C.c_longlong), ("level1_unrecovered", C.c_longlong), ("iter_ms", C.c_double), ("iterations", C.c_longlong),
                ("grid_fallback", C.c_longlong), ("allreduce_ms", C.c_double),
                ("allreduce_calls", C.c_longlong), ("cert_max_err_ratio", C.c_double),
                ("cert_min_margin", C.c_double), ("cert_audited", C.c_longlong),
                ("persistent_runs", C.c_longlong), ("cpu_rule_ties", C.c_longlong),
                ("cpu_rule_changed", C.c_longlong), ("persistent_fallbacks", C.c_longlong),
                ("last_filter", C.c_int), ("bundle_builds", C.c_longlong),
                ("bundle_builds_in_run", C.c_longlong), ("run_bundle_searches", C.c_longlong),
                ("run_grid_searches", C.c_longlong), ("run_certified", C.c_longlong),
                ("run_walked", C.c_longlong), ("run_path_bits", C.c_ulonglong)]


class GlobalParams(C.Structure):
    """icp_global_params: zero fields take the header's defaults."""
    _fields_ = [("voxel", C.c_double), ("k_normals", C.c_int), ("k_fpfh", C.c_int), ("mutual", C.c_int),
                ("hypotheses", C.c_longlong), ("seed", C.c_uint64), ("max_dist", C.c_double),
                ("edge_ratio", C.c_double)]


class GlobalReport(C.Structure):
    _fields_ = [(k, C.c_longlong) for k in ("model_points", "scene_points", "matches", "evaluated", "inliers",
                                            "best_h")]


class Evaluation(C.Structure):
    """icp_evaluation: what icp_evaluate reports of the resident scene against the resident model."""
    _fields_ = [("scene_points", C.c_longlong), ("correspondences", C.c_longlong), ("fitness", C.c_double),
                ("inlier_rmse", C.c_double), ("max_inlier_d2", C.c_double), ("information", C.c_double * 36),
                ("model_points", C.c_longlong), ("model_correspondences", C.c_longlong),
                ("model_fitness", C.c_double), ("model_rmse", C.c_double), ("model_max_inlier_d2", C.c_double)]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "information"}
        d["information"] = np.array(self.information, dtype=np.float64).reshape(6, 6)
        return d


FPFH_DIM = 33


class BundleAudit(C.Structure):
    _fields_ = [("max_err_ratio", C.c_double), ("min_gap", C.c_double), ("pairs", C.c_longlong),
                ("excluded", C.c_longlong), ("checked", C.c_longlong), ("violations", C.c_longlong)]


# icp_stats.last_filter (ICP_FILTER_*): the search level that decided most queries
FILTER_NAMES = {-1: None, 0: "valu", 1: "mfma", 2: "mfma16", 3: "bundle", 4: "grid", 5: "fp64", 6: "one_launch"}


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_size_t, C.c_void_p)
PROGRESS_FN = C.CFUNCTYPE(None, C.c_int, C.c_double, C.c_void_p)

_lib = None


def lib() -> C.CDLL:
    """Load libicp_hip.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ICPError(ICP_E_NO_DEVICE, f"{LIB_PATH} not built: run `make -C iterative-closest-point_amd`")
    L = C.CDLL(LIB_PATH)
    dp = C.POINTER(C.c_double)
    vp = C.c_void_p
    sz = C.c_size_t
    L.icp_ctx_create.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    L.icp_ctx_create_dist.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(vp)]
    L.icp_rccl_unique_id.argtypes = [C.c_char_p]
    L.icp_ctx_create_sharded.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, ALLREDUCE_FN, vp, C.POINTER(vp)]
    L.icp_ctx_destroy.argtypes = [vp]
    L.icp_ctx_destroy.restype = None
    L.icp_last_error.argtypes = [vp]
    L.icp_last_error.restype = C.c_char_p
    L.icp_strerror.argtypes = [C.c_int]
    L.icp_strerror.restype = C.c_char_p
    L.icp_device_count.argtypes = [C.POINTER(C.c_int)]
    L.icp_set_model.argtypes = [vp, dp, sz]
    L.icp_set_model_device.argtypes = [vp, vp, sz]
    L.icp_set_progress.argtypes = [vp, PROGRESS_FN, vp]
    L.icp_set_scene_device.argtypes = [vp, vp, sz, sz]
    if hasattr(L, "icp_set_model_device_stream"):  # (an A/B library of an earlier round may lack them)
        L.icp_set_model_device_stream.argtypes = [vp, vp, sz, vp]
        L.icp_set_scene_device_stream.argtypes = [vp, vp, sz, sz, vp]
    L.icp_set_scene.argtypes = [vp, dp, sz, sz]
    L.icp_get_scene.argtypes = [vp, dp]
    L.icp_set_allow_unequal.argtypes = [vp, C.c_int]
    L.icp_set_nn_variant.argtypes = [vp, C.c_int]
    L.icp_set_run_mode.argtypes = [vp, C.c_int]
    L.icp_set_nn_rule.argtypes = [vp, C.c_int]
    L.icp_run.argtypes = [vp, C.c_int, C.c_double, dp, C.POINTER(Result)]
    L.icp_closest_matrix.argtypes = [vp, dp, sz, dp, C.POINTER(C.c_int32)]
    L.icp_compute_centroid.argtypes = [vp, dp, sz, dp, dp]
    L.icp_y_p_norm.argtypes = [vp, dp, dp, sz, dp, dp]
    L.icp_err_compute.argtypes = [vp, dp, dp, sz, C.c_int, dp, dp, dp]
    L.icp_find_alignment.argtypes = [vp, dp, dp, sz, dp, dp, dp, dp]
    L.icp_horn_solve.argtypes = [dp, dp, dp, C.c_double, C.c_double, dp, dp, dp]
    L.icp_max_element_index.argtypes = [dp]
    L.icp_shard_range.argtypes = [sz, C.c_int, C.c_int, C.POINTER(sz), C.POINTER(sz)]
    L.icp_synthetic_pair.argtypes = [C.c_uint64, sz, C.c_double, dp, dp, dp, dp]
    L.icp_load_matrix.argtypes = [C.c_char_p, C.POINTER(dp), C.POINTER(sz)]
    L.icp_write_matrix.argtypes = [C.c_char_p, dp, sz]
    L.icp_free.argtypes = [vp]
    L.icp_free.restype = None
    L.icp_ensure_model.argtypes = [vp, dp, sz, C.POINTER(C.c_int)]
    L.icp_subtract_col.argtypes = [vp, dp, sz, dp, dp]
    L.icp_get_indices.argtypes = [vp, C.POINTER(C.c_int32)]
    L.icp_get_model_order.argtypes = [vp, C.POINTER(C.c_int32)]
    L.icp_get_grid.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                               C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.icp_sort_pairs.argtypes = [C.c_int, C.POINTER(C.c_uint32), sz, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
    L.icp_debug_live_buffers.argtypes = []
    L.icp_debug_live_buffers.restype = C.c_longlong
    L.icp_set_index_digest.argtypes = [vp, sz]
    L.icp_get_index_digest.argtypes = [vp, C.POINTER(C.c_uint64), sz]
    L.icp_set_cert_audit.argtypes = [vp, C.c_int]
    L.icp_bundle_audit.argtypes = [vp, C.c_int, C.POINTER(BundleAudit)]
    L.icp_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.icp_reset_stats.argtypes = [vp]
    L.icp_set_bundle_counters.argtypes = [vp, C.c_int]
    L.icp_get_bundle_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.icp_get_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    if hasattr(L, "icp_set_max_distance"):  # (an A/B library of an earlier round lacks them)
        L.icp_set_max_distance.argtypes = [vp, C.c_double]
        L.icp_get_inliers.argtypes = [vp, C.POINTER(C.c_uint8), C.POINTER(C.c_longlong)]
        L.icp_get_inlier_trace.argtypes = [vp, C.POINTER(C.c_longlong), sz]
    if hasattr(L, "icp_set_metric"):
        L.icp_set_metric.argtypes = [vp, C.c_int]
        L.icp_set_model_normals.argtypes = [vp, dp, sz]
        L.icp_set_model_normals_device.argtypes = [vp, vp, sz]
    if hasattr(L, "icp_model_knn"):
        L.icp_model_knn.argtypes = [vp, C.c_int, C.POINTER(C.c_int32), dp]
        L.icp_estimate_model_normals.argtypes = [vp, C.c_int, dp, C.POINTER(C.c_longlong)]
        L.icp_get_model_normals.argtypes = [vp, dp]
    if hasattr(L, "icp_set_robust"):
        L.icp_set_robust.argtypes = [vp, C.c_int, C.c_double]
        L.icp_get_robust_trace.argtypes = [vp, dp, C.POINTER(C.c_longlong), sz]
    if hasattr(L, "icp_voxel_downsample"):
        L.icp_voxel_downsample.argtypes = [vp, dp, sz, C.c_double, dp, dp, C.POINTER(C.c_int32), C.POINTER(sz)]
        L.icp_voxel_downsample_device.argtypes = [vp, vp, sz, C.c_double, dp, vp, vp, C.POINTER(sz)]
        L.icp_get_transform.argtypes = [vp, dp, dp, dp]
        L.icp_transform_scene.argtypes = [vp, C.c_double, dp, dp]
    if hasattr(L, "icp_set_trim"):
        L.icp_set_trim.argtypes = [vp, C.c_double]
        L.icp_get_trim_trace.argtypes = [vp, dp, sz]
        L.icp_select_kth.argtypes = [C.c_int, dp, sz, sz, dp]
    if hasattr(L, "icp_set_plane_symmetric"):
        L.icp_set_plane_symmetric.argtypes = [vp, C.c_int]
        L.icp_set_scene_normals.argtypes = [vp, dp, sz]
        L.icp_set_scene_normals_device.argtypes = [vp, vp, sz]
        L.icp_get_scene_normals.argtypes = [vp, dp]
        L.icp_estimate_scene_normals.argtypes = [vp, C.c_int, dp, C.POINTER(C.c_longlong)]
    if hasattr(L, "icp_set_plane_to_plane"):
        L.icp_set_plane_to_plane.argtypes = [vp, C.c_double]
    if hasattr(L, "icp_set_one_to_one"):
        L.icp_set_one_to_one.argtypes = [vp, C.c_int]
    if hasattr(L, "icp_fpfh"):
        ip, llp = C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
        L.icp_fpfh.argtypes = [vp, dp, sz, dp, C.c_int, dp, C.c_int, dp, dp, dp]
        L.icp_match_features.argtypes = [vp, dp, sz, dp, sz, ip, dp]
        L.icp_match_features_plan.argtypes = [sz, sz, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.icp_ransac_pose.argtypes = [vp, dp, dp, sz, C.c_longlong, C.c_uint64, C.c_double, C.c_double, dp, dp,
                                      llp, llp, llp, ip, C.POINTER(C.c_uint8)]
        L.icp_global_pose.argtypes = [vp, dp, sz, dp, sz, C.POINTER(GlobalParams), dp, dp, C.POINTER(GlobalReport)]
    if hasattr(L, "icp_filter_statistical"):
        u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        L.icp_filter_statistical.argtypes = [vp, dp, sz, C.c_int, C.c_double, dp, u8p, C.POINTER(sz), dp, dp]
        L.icp_filter_statistical_device.argtypes = [vp, vp, sz, C.c_int, C.c_double, vp, vp, C.POINTER(sz), vp, dp]
        L.icp_filter_radius.argtypes = [vp, dp, sz, C.c_double, C.c_int, dp, u8p, C.POINTER(sz), i32p]
        L.icp_filter_radius_device.argtypes = [vp, vp, sz, C.c_double, C.c_int, vp, vp, C.POINTER(sz), vp]
    if hasattr(L, "icp_evaluate"):
        i32p = C.POINTER(C.c_int32)
        L.icp_evaluate.argtypes = [vp, C.c_double, C.c_int, C.POINTER(Evaluation), i32p, dp, i32p, dp]
        L.icp_evaluate_device.argtypes = [vp, C.c_double, C.c_int, C.POINTER(Evaluation), vp, vp, vp, vp]
    _lib = L
    return L


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _cloud(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("clouds are (n, 3) float64 arrays")
    return a


def _vec(a, n) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    if a.size != n:
        raise ValueError(f"expected {n} values")
    return a


# ---------------------------------------------------------------------------------
# host-only helpers (no device needed)
# ---------------------------------------------------------------------------------

def strerror(code: int) -> str:
    return lib().icp_strerror(code).decode()


def device_count() -> int:
    n = C.c_int(0)
    lib().icp_device_count(C.byref(n))
    return n.value


def sort_pairs(keys, bits: int, device: int = 0):
    """The engine's stable LSD radix sort (icp_sort_pairs) -> (order int32, sorted keys uint32)."""
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    order = np.empty(k.size, dtype=np.int32); out = np.empty(k.size, dtype=np.uint32)
    rc = lib().icp_sort_pairs(device, k.ctypes.data_as(C.POINTER(C.c_uint32)), k.size, bits,
                              out.ctypes.data_as(C.POINTER(C.c_uint32)), order.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != ICP_OK:
        raise ICPError(rc, strerror(rc))
    return order, out


def debug_live_buffers() -> int:
    """The blocks of device and pinned host memory the library holds now (icp_debug_live_buffers)."""
    return int(lib().icp_debug_live_buffers())


def select_kth(values, k: int, device: int = 0) -> float:
    """The engine's radix select (icp_select_kth): the k-th smallest (1-based) of the doubles in the
    order -inf < ... < -0 < +0 < ... < +inf < NaN."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    out = C.c_double(0.0)
    rc = lib().icp_select_kth(device, _dp(v) if v.size else None, v.size, int(k) if k >= 0 else 0, C.byref(out))
    if rc != ICP_OK:
        raise ICPError(rc, strerror(rc))
    return out.value


def horn_solve(S, mu_p, mu_y, d_caps: float, sp: float):
    """Host half of find_alignment (gpu.cc:104-146) -> (s, R(3x3), t(3))."""
    S = _vec(S, 9); mu_p = _vec(mu_p, 3); mu_y = _vec(mu_y, 3)
    s = C.c_double(0.0); R = np.zeros(9); t = np.zeros(3)
    rc = lib().icp_horn_solve(_dp(S), _dp(mu_p), _dp(mu_y), d_caps, sp, C.byref(s), _dp(R), _dp(t))
    if rc != ICP_OK:
        raise ICPError(rc, strerror(rc))
    return s.value, R.reshape(3, 3), t


def max_element_index(ev) -> int:
    """gpu.cc:85-93 verbatim (the quirky 'largest' eigenvalue picker)."""
    ev = _vec(ev, 4)
    return lib().icp_max_element_index(_dp(ev))


def shard_range(n_total: int, rank: int, world: int):
    b = C.c_size_t(0); c = C.c_size_t(0)
    rc = lib().icp_shard_range(n_total, rank, world, C.byref(b), C.byref(c))
    if rc != ICP_OK:
        raise ICPError(rc, strerror(rc))
    return b.value, c.value


def synthetic_pair(n: int, seed: int = 42, angle_deg: float = 5.0, axis=(1.0, 2.0, 3.0),
                   t=(0.05, -0.03, 0.02)):
    """SURVEY.md §8d generator: (model, scene) as (n, 3) float64."""
    m = np.empty((n, 3)); p = np.empty((n, 3))
    ax = np.asarray(axis, dtype=np.float64); tt = np.asarray(t, dtype=np.float64)
    rc = lib().icp_synthetic_pair(seed, n, angle_deg, _dp(ax), _dp(tt), _dp(m), _dp(p))
    if rc != ICP_OK:
        raise ICPError(rc, strerror(rc))
    return m, p


def load_matrix(path: str) -> np.ndarray:
    """src/load.cc:3-33 -> (n, 3) float64."""
    ptr = C.POINTER(C.c_double)(); n = C.c_size_t(0)
    rc = lib().icp_load_matrix(path.encode(), C.byref(ptr), C.byref(n))
    if rc != ICP_OK:
        raise ICPError(rc, f"{path}: {strerror(rc)}")
    try:
        out = np.ctypeslib.as_array(ptr, shape=(max(n.value, 1) * 3,))[: n.value * 3].copy()
    finally:
        lib().icp_free(ptr)
    return out.reshape(n.value, 3)


def write_matrix(path: str, xyz) -> None:
    xyz = _cloud(xyz)
    rc = lib().icp_write_matrix(path.encode(), _dp(xyz), xyz.shape[0])
    if rc != ICP_OK:
        raise ICPError(rc, strerror(rc))


def rccl_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    rc = lib().icp_rccl_unique_id(buf)
    if rc != ICP_OK:
        raise ICPError(rc, strerror(rc))
    return buf.raw


# ---------------------------------------------------------------------------------
# device context
# ---------------------------------------------------------------------------------

class Context:
    """One HIP device context (optionally one rank of an RCCL job)."""

    def __init__(self, device: int = 0, nn_mode: int = NN_CERTIFIED, rank: int = 0,
                 world_size: int = 1, rccl_id: bytes | None = None, host_allreduce=None):
        """host_allreduce(np.ndarray) -> None: in-place sum over ranks (instead of RCCL)."""
        L = lib()
        h = C.c_void_p()
        self._cb = None
        if host_allreduce is not None:
            def _cb(buf, count, _user):
                try:
                    host_allreduce(np.ctypeslib.as_array(buf, shape=(count,)))
                    return 0
                except Exception:  # a failed rendezvous must not unwind through C
                    return 1
            self._cb = ALLREDUCE_FN(_cb)
            rc = L.icp_ctx_create_sharded(device, nn_mode, rank, world_size, self._cb, None, C.byref(h))
        elif world_size > 1 or rccl_id is not None:
            rc = L.icp_ctx_create_dist(device, nn_mode, rank, world_size, rccl_id, C.byref(h))
        else:
            rc = L.icp_ctx_create(device, nn_mode, C.byref(h))
        if rc != ICP_OK:
            raise ICPError(rc, f"context creation failed: {strerror(rc)}")
        self._h = h
        self.rank, self.world_size = rank, world_size

    def _check(self, rc: int):
        if rc != ICP_OK:
            raise ICPError(rc, f"{strerror(rc)}: {lib().icp_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None):
            lib().icp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # resident clouds
    def set_model(self, m):
        m = _cloud(m)
        self._check(lib().icp_set_model(self._h, _dp(m), m.shape[0]))
        self._nm = m.shape[0]

    def set_model_device(self, ptr: int, nm: int, stream=None):
        """icp_set_model_device: the model's AoS fp64 array already in device memory (a device
        pointer, e.g. a torch tensor's data_ptr()).  stream None: read after all work enqueued so
        far on the device (a device synchronisation); else a HIP stream handle (e.g.
        torch.cuda.current_stream().cuda_stream): read after the work enqueued on that stream
        (icp_set_model_device_stream, no host synchronisation; stream-ordered: keep the array alive
        and unmodified until run() or another synchronising call returns)."""
        if stream is None or not hasattr(lib(), "icp_set_model_device_stream"):
            self._check(lib().icp_set_model_device(self._h, C.c_void_p(ptr), nm))
        else:
            self._check(lib().icp_set_model_device_stream(self._h, C.c_void_p(ptr), nm, C.c_void_p(stream)))
        self._nm = nm

    def set_scene_device(self, ptr: int, np_local: int, np_total: int | None = None, stream=None):
        """icp_set_scene_device: the scene's AoS fp64 array already in device memory (stream: as
        set_model_device)."""
        npt = np_local if np_total is None else np_total
        if stream is None or not hasattr(lib(), "icp_set_scene_device_stream"):
            self._check(lib().icp_set_scene_device(self._h, C.c_void_p(ptr), np_local, npt))
        else:
            self._check(lib().icp_set_scene_device_stream(self._h, C.c_void_p(ptr), np_local, npt,
                                                          C.c_void_p(stream)))
        self._np_local = np_local

    def set_progress(self, fn):
        """icp_set_progress: fn(iteration, err) for each recorded iteration of icp_run, as it ends
        (None switches it off).  The ctypes thunk is kept alive with the context."""
        self._progress = PROGRESS_FN(lambda i, e, _u: fn(i, e)) if fn is not None else None
        self._check(lib().icp_set_progress(self._h, self._progress if fn is not None else PROGRESS_FN(), None))

    def ensure_model(self, m) -> bool:
        """icp_ensure_model: upload unless the resident model has these exact contents."""
        m = _cloud(m)
        up = C.c_int(0)
        self._check(lib().icp_ensure_model(self._h, _dp(m), m.shape[0], C.byref(up)))
        self._nm = m.shape[0]
        return bool(up.value)

    def set_scene(self, p, np_total: int | None = None):
        p = _cloud(p)
        self._check(lib().icp_set_scene(self._h, _dp(p), p.shape[0], p.shape[0] if np_total is None else np_total))
        self._np_local = p.shape[0]

    def get_scene(self) -> np.ndarray:
        out = np.empty((self._np_local, 3))
        self._check(lib().icp_get_scene(self._h, _dp(out)))
        return out

    def set_nn_variant(self, variant: int):
        self._check(lib().icp_set_nn_variant(self._h, variant))

    def set_nn_rule(self, rule: int):
        """icp_set_nn_rule: RULE_SQUARED (GPU path) / RULE_CPU_SQRT (the reference CPU path)."""
        self._check(lib().icp_set_nn_rule(self._h, rule))

    def set_run_mode(self, mode: int):
        """icp_set_run_mode: RUN_AUTO / RUN_LAUNCHES / RUN_PERSISTENT (bit-identical results)."""
        self._check(lib().icp_set_run_mode(self._h, mode))

    def set_allow_unequal(self, allow: bool):
        self._check(lib().icp_set_allow_unequal(self._h, 1 if allow else 0))
        self._allow_unequal = bool(allow)

    def voxel_downsample(self, xyz, voxel: float, origin=None, counts: bool = False):
        """icp_voxel_downsample: one point per occupied cell of a lattice of side `voxel` through
        `origin` (None: the cloud's minimum corner), the mean of the cell's points, in ascending cell-key
        order -> (n_out, 3), or (points, counts int32) with counts."""
        xyz = _cloud(xyz)
        n = xyz.shape[0]
        o = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        out = np.empty((max(n, 1), 3))
        cnt = np.empty(max(n, 1), dtype=np.int32) if counts else None
        n_out = C.c_size_t(0)
        self._check(lib().icp_voxel_downsample(self._h, _dp(xyz), n, float(voxel), None if o is None else _dp(o),
                                               _dp(out), cnt.ctypes.data_as(C.POINTER(C.c_int32)) if counts else None,
                                               C.byref(n_out)))
        k = int(n_out.value)
        return (out[:k].copy(), cnt[:k].copy()) if counts else out[:k].copy()

    def voxel_downsample_device(self, ptr: int, n: int, voxel: float, out_ptr: int, origin=None,
                                count_ptr: int | None = None) -> int:
        """icp_voxel_downsample_device: the cloud (AoS fp64), the output cloud (room for n points) and
        the counts (int32, room for n; None: not wanted) are device pointers -> the number of cells."""
        o = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        n_out = C.c_size_t(0)
        self._check(lib().icp_voxel_downsample_device(self._h, C.c_void_p(ptr), n, float(voxel),
                                                      None if o is None else _dp(o), C.c_void_p(out_ptr),
                                                      C.c_void_p(count_ptr) if count_ptr else None, C.byref(n_out)))
        return int(n_out.value)

    def filter_statistical(self, xyz, k: int = 16, std_ratio: float = 2.0, mask: bool = False, mean_dist: bool = False,
                           stats: bool = False):
        """icp_filter_statistical: the points whose mean distance to their k nearest neighbours is at most
        mu + std_ratio * sigma of those means, in input order -> (n_out, 3), or a tuple of the points and, as
        asked for, the mask (n, uint8), the mean distances (n) and (mu, sigma, T)."""
        xyz = _cloud(xyz)
        n = xyz.shape[0]
        out = np.empty((max(n, 1), 3))
        mk = np.empty(max(n, 1), dtype=np.uint8) if mask else None
        md = np.empty(max(n, 1)) if mean_dist else None
        st = np.empty(3) if stats else None
        n_out = C.c_size_t(0)
        self._check(lib().icp_filter_statistical(self._h, _dp(xyz), n, int(k), float(std_ratio), _dp(out),
                                                 mk.ctypes.data_as(C.POINTER(C.c_uint8)) if mask else None,
                                                 C.byref(n_out), _dp(md) if mean_dist else None,
                                                 _dp(st) if stats else None))
        res = (out[:int(n_out.value)].copy(),) + tuple(a[:n] for a in (mk, md) if a is not None)
        if stats:
            res += (st,)
        return res if len(res) > 1 else res[0]

    def filter_radius(self, xyz, radius: float, min_neighbors: int, mask: bool = False, counts: bool = False):
        """icp_filter_radius: the points with at least min_neighbors other points within `radius`, in input
        order -> (n_out, 3), or a tuple of the points and, as asked for, the mask (n, uint8) and the counts
        (n, int32: the points within the radius, the point itself included)."""
        xyz = _cloud(xyz)
        n = xyz.shape[0]
        out = np.empty((max(n, 1), 3))
        mk = np.empty(max(n, 1), dtype=np.uint8) if mask else None
        cn = np.empty(max(n, 1), dtype=np.int32) if counts else None
        n_out = C.c_size_t(0)
        self._check(lib().icp_filter_radius(self._h, _dp(xyz), n, float(radius), int(min_neighbors), _dp(out),
                                            mk.ctypes.data_as(C.POINTER(C.c_uint8)) if mask else None, C.byref(n_out),
                                            cn.ctypes.data_as(C.POINTER(C.c_int32)) if counts else None))
        res = (out[:int(n_out.value)].copy(),) + tuple(a[:n] for a in (mk, cn) if a is not None)
        return res if len(res) > 1 else res[0]

    def filter_statistical_device(self, ptr: int, n: int, k: int, std_ratio: float, out_ptr: int | None,
                                  mask_ptr: int | None = None, mean_dist_ptr: int | None = None):
        """icp_filter_statistical_device: the cloud (AoS fp64), the output cloud (room for n points), the mask
        (uint8, n) and the mean distances (fp64, n) are device pointers (None: not wanted)
        -> (n_out, (mu, sigma, T))."""
        n_out = C.c_size_t(0)
        st = np.empty(3)
        opt = lambda q: C.c_void_p(q) if q else None
        self._check(lib().icp_filter_statistical_device(self._h, C.c_void_p(ptr), n, int(k), float(std_ratio),
                                                        opt(out_ptr), opt(mask_ptr), C.byref(n_out),
                                                        opt(mean_dist_ptr), _dp(st)))
        return int(n_out.value), st

    def filter_radius_device(self, ptr: int, n: int, radius: float, min_neighbors: int, out_ptr: int | None,
                             mask_ptr: int | None = None, count_ptr: int | None = None) -> int:
        """icp_filter_radius_device: as filter_statistical_device; the counts are int32 -> n_out."""
        n_out = C.c_size_t(0)
        opt = lambda q: C.c_void_p(q) if q else None
        self._check(lib().icp_filter_radius_device(self._h, C.c_void_p(ptr), n, float(radius), int(min_neighbors),
                                                   opt(out_ptr), opt(mask_ptr), C.byref(n_out), opt(count_ptr)))
        return int(n_out.value)

    def evaluate(self, max_dist: float, both: bool = False, per_point: bool = False) -> dict:
        """icp_evaluate: the resident scene as it lies now against the resident model -> a dict of
        icp_evaluation's fields, `information` a (6, 6) array.  A pair is kept iff its squared distance is
        at most max_dist * max_dist (float('inf'): every pair).  both: the model's side too (model_*).
        per_point: `idx` (int32, -1: no pair) and `d2` (+inf: no pair) of the np scene points in the
        caller's order, and with both `model_idx` / `model_d2` of the nm model points."""
        ev = Evaluation()
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        idx = d2 = midx = md2 = None
        if per_point:
            idx, d2 = np.empty(self._np_local, dtype=np.int32), np.empty(self._np_local)
            if both:
                midx, md2 = np.empty(self._nm, dtype=np.int32), np.empty(self._nm)
        self._check(lib().icp_evaluate(self._h, float(max_dist), 1 if both else 0, C.byref(ev),
                                       ip(idx) if per_point else None, _dp(d2) if per_point else None,
                                       ip(midx) if midx is not None else None, _dp(md2) if md2 is not None else None))
        out = ev.as_dict()
        if per_point:
            out["idx"], out["d2"] = idx, d2
            if both:
                out["model_idx"], out["model_d2"] = midx, md2
        return out

    def evaluate_device(self, max_dist: float, both: bool = False, idx_ptr: int | None = None,
                        d2_ptr: int | None = None, model_idx_ptr: int | None = None,
                        model_d2_ptr: int | None = None) -> dict:
        """icp_evaluate_device: as evaluate; the per-point arrays (int32 / fp64, np and nm entries) are device
        pointers (None: not wanted)."""
        ev = Evaluation()
        opt = lambda q: C.c_void_p(q) if q else None  # noqa: E731
        self._check(lib().icp_evaluate_device(self._h, float(max_dist), 1 if both else 0, C.byref(ev), opt(idx_ptr),
                                              opt(d2_ptr), opt(model_idx_ptr), opt(model_d2_ptr)))
        return ev.as_dict()

    def transform(self):
        """icp_get_transform: (s, R (3, 3), t (3,)) with q = s R p + t mapping the scene as set_scene
        received it onto the resident scene now (every applied iteration, every transform_scene)."""
        s = C.c_double(0.0)
        R = np.empty(9)
        t = np.empty(3)
        self._check(lib().icp_get_transform(self._h, C.cast(C.byref(s), C.POINTER(C.c_double)), _dp(R), _dp(t)))
        return float(s.value), R.reshape(3, 3), t

    def transform_scene(self, s: float, R, t):
        """icp_transform_scene: moves the resident scene by q = s R p + t, composes it into the total
        and prepares the scene as set_scene of the moved points would."""
        R = _vec(R, 9)
        t = _vec(t, 3)
        self._check(lib().icp_transform_scene(self._h, float(s), _dp(R), _dp(t)))

    def set_max_distance(self, d: float):
        """icp_set_max_distance: run() keeps only the pairs no farther apart than d (0 or inf: off)."""
        self._check(lib().icp_set_max_distance(self._h, float(d)))

    def set_metric(self, metric: int):
        """icp_set_metric: METRIC_POINT_TO_POINT (the default) / METRIC_POINT_TO_PLANE (needs
        set_model_normals; run() then returns s = 1 and may raise ICP_E_DEGENERATE)."""
        self._check(lib().icp_set_metric(self._h, int(metric)))

    def set_model_normals(self, n):
        """icp_set_model_normals: one normal per point of the resident model, used as given."""
        n = _cloud(n)
        self._check(lib().icp_set_model_normals(self._h, _dp(n), n.shape[0]))

    def set_model_normals_device(self, ptr: int, nm: int):
        """icp_set_model_normals_device: the normals' AoS fp64 array already in device memory."""
        self._check(lib().icp_set_model_normals_device(self._h, C.c_void_p(ptr), nm))

    def model_knn(self, k: int, distances: bool = False):
        """icp_model_knn: the k nearest model points of every model point, ascending (d2, index)
        -> idx (nm, k) int32, or (idx, d2) with distances."""
        k = int(k)
        cnt = getattr(self, "_nm", 0) * k if 0 < k <= 64 else 0  # (a refused k writes nothing)
        idx = np.empty(max(cnt, 1), dtype=np.int32)
        d2 = np.empty(max(cnt, 1)) if distances else None
        self._check(lib().icp_model_knn(self._h, k, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                        _dp(d2) if distances else None))
        idx = idx[:cnt].reshape(-1, k)
        return (idx, d2[:cnt].reshape(-1, k)) if distances else idx

    def estimate_model_normals(self, k: int, viewpoint=None) -> int:
        """icp_estimate_model_normals: the resident model's normals from its own k-neighbourhoods
        (PCA; towards `viewpoint`, or the largest component positive); they become the context's
        normals.  Returns how many points got a zero normal (direction undetermined)."""
        v = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(3)
        deg = C.c_longlong(0)
        self._check(lib().icp_estimate_model_normals(self._h, int(k), None if v is None else _dp(v), C.byref(deg)))
        return int(deg.value)

    def model_normals(self) -> np.ndarray:
        """icp_get_model_normals: the context's normals (nm, 3), however they were set."""
        nm = getattr(self, "_nm", 0)
        out = np.empty((max(nm, 1), 3))
        self._check(lib().icp_get_model_normals(self._h, _dp(out)))
        return out[:nm]

    def set_plane_symmetric(self, on):
        """icp_set_plane_symmetric: with METRIC_POINT_TO_PLANE, run() minimises the symmetric objective
        (needs set_model_normals and set_scene_normals; its err is up to four times the one-sided one)."""
        self._check(lib().icp_set_plane_symmetric(self._h, int(on)))

    def set_plane_to_plane(self, eps):
        """icp_set_plane_to_plane: with METRIC_POINT_TO_PLANE, run() minimises generalised ICP's plane-to-plane
        objective, each cloud's covariance (eps, 1, 1) about its normal (0 < eps <= 1; PCL's and Open3D's
        default is 1e-3; 0: off).  Needs set_model_normals and set_scene_normals, excludes
        set_plane_symmetric; its err is the mean squared Mahalanobis residual."""
        self._check(lib().icp_set_plane_to_plane(self._h, float(eps)))

    def set_scene_normals(self, n):
        """icp_set_scene_normals: one normal per point of the resident scene as set_scene received it,
        kept as given; the current normals follow the scene (scene_normals)."""
        n = _cloud(n)
        self._check(lib().icp_set_scene_normals(self._h, _dp(n), n.shape[0]))

    def set_scene_normals_device(self, ptr: int, np_local: int):
        """icp_set_scene_normals_device: the normals' AoS fp64 array already in device memory."""
        self._check(lib().icp_set_scene_normals_device(self._h, C.c_void_p(ptr), np_local))

    def scene_normals(self) -> np.ndarray:
        """icp_get_scene_normals: the CURRENT normals (np_local, 3), the given ones turned by the
        rotation of transform(), in the caller's point order."""
        n = getattr(self, "_np_local", 0)
        out = np.empty((max(n, 1), 3))
        self._check(lib().icp_get_scene_normals(self._h, _dp(out)))
        return out[:n]

    def estimate_scene_normals(self, k: int, viewpoint=None) -> int:
        """icp_estimate_scene_normals: the resident scene's normals from its own k-neighbourhoods, as
        estimate_model_normals makes the model's; only on an unsharded scene no run() or
        transform_scene() has touched.  Returns how many points got a zero normal."""
        v = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(3)
        deg = C.c_longlong(0)
        self._check(lib().icp_estimate_scene_normals(self._h, int(k), None if v is None else _dp(v), C.byref(deg)))
        return int(deg.value)

    def fpfh(self, xyz, k: int = 32, normals=None, k_normals: int = 16, viewpoint=None, spfh: bool = False,
             return_normals: bool = False):
        """icp_fpfh: the 33-bin FPFH descriptors of a cloud from its k-neighbourhoods; the normals are
        the given ones or estimated from k_normals neighbours -> fpfh (n, 33), or a tuple with the SPFH
        rows (spfh) and the normals used (return_normals) behind it."""
        xyz = _cloud(xyz)
        n = xyz.shape[0]
        nr = None if normals is None else _cloud(normals)
        if nr is not None and nr.shape[0] != n:
            raise ValueError("one normal per point")
        v = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(3)
        out = np.empty((max(n, 1), FPFH_DIM))
        sp = np.empty((max(n, 1), FPFH_DIM)) if spfh else None
        no = np.empty((max(n, 1), 3)) if return_normals else None
        self._check(lib().icp_fpfh(self._h, _dp(xyz), n, None if nr is None else _dp(nr), int(k_normals),
                                   None if v is None else _dp(v), int(k), _dp(out), None if sp is None else _dp(sp),
                                   None if no is None else _dp(no)))
        res = (out[:n],) + ((sp[:n],) if spfh else ()) + ((no[:n],) if return_normals else ())
        return res[0] if len(res) == 1 else res

    def match_features(self, fa, fb, distances: bool = False):
        """icp_match_features: for every row of fa the nearest row of fb (the lowest index among the
        minimisers; -1 when every distance is a NaN) -> idx (na,) int32, or (idx, D) with distances."""
        fa = np.ascontiguousarray(fa, dtype=np.float64)
        fb = np.ascontiguousarray(fb, dtype=np.float64)
        if fa.ndim != 2 or fb.ndim != 2 or fa.shape[1] != FPFH_DIM or fb.shape[1] != FPFH_DIM:
            raise ValueError("descriptors are (n, 33) float64 arrays")
        idx = np.empty(max(fa.shape[0], 1), dtype=np.int32)
        d = np.empty(max(fa.shape[0], 1)) if distances else None
        self._check(lib().icp_match_features(self._h, _dp(fa), fa.shape[0], _dp(fb), fb.shape[0],
                                             idx.ctypes.data_as(C.POINTER(C.c_int32)), _dp(d) if distances else None))
        idx = idx[:fa.shape[0]]
        return (idx, d[:fa.shape[0]]) if distances else idx

    def ransac_pose(self, p, q, hypotheses: int = 100000, seed: int = 0, max_dist: float = 1.0,
                    edge_ratio: float = 0.9, counts: bool = False, mask: bool = False) -> dict:
        """icp_ransac_pose: the rigid pose q = R p + t with the most pairs p_c -> q_c within max_dist among
        `hypotheses` 3-pair samples of `seed` -> dict(R (3, 3), t, inliers, best_h, evaluated, and with
        counts / mask: counts (hypotheses,) int32 with -1 for a rejected sample, mask (C,) bool)."""
        p = _cloud(p)
        q = _cloud(q)
        if p.shape[0] != q.shape[0]:
            raise ValueError("one q per p")
        H = int(hypotheses)
        R = np.empty(9)
        t = np.empty(3)
        inl, bh, ev = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        cn = np.empty(max(H, 1), dtype=np.int32) if counts and 0 < H < 2 ** 32 else None
        mk = np.empty(max(p.shape[0], 1), dtype=np.uint8) if mask else None
        self._check(lib().icp_ransac_pose(self._h, _dp(p), _dp(q), p.shape[0], H, int(seed), float(max_dist),
                                          float(edge_ratio), _dp(R), _dp(t), C.byref(inl), C.byref(bh), C.byref(ev),
                                          None if cn is None else cn.ctypes.data_as(C.POINTER(C.c_int32)),
                                          None if mk is None else mk.ctypes.data_as(C.POINTER(C.c_uint8))))
        out = {"R": R.reshape(3, 3), "t": t, "inliers": int(inl.value), "best_h": int(bh.value),
               "evaluated": int(ev.value)}
        if cn is not None:
            out["counts"] = cn[:H]
        if mk is not None:
            out["mask"] = mk[:p.shape[0]].astype(bool)
        return out

    def global_pose(self, m, p, voxel: float, k_normals: int = 0, k_fpfh: int = 0, mutual: bool = True,
                    hypotheses: int = 0, seed: int = 0, max_dist: float = 0.0, edge_ratio: float = 0.0):
        """icp_global_pose: downsample both clouds, FPFH, (mutual) feature matches, RANSAC; zeros take the
        header's defaults -> (R (3, 3), t, report dict) with q = R p + t mapping the scene onto the model."""
        m = _cloud(m)
        p = _cloud(p)
        prm = GlobalParams(float(voxel), int(k_normals), int(k_fpfh), 1 if mutual else 0, int(hypotheses), int(seed),
                           float(max_dist), float(edge_ratio))
        rep = GlobalReport()
        R = np.empty(9)
        t = np.empty(3)
        self._check(lib().icp_global_pose(self._h, _dp(m), m.shape[0], _dp(p), p.shape[0], C.byref(prm), _dp(R), _dp(t),
                                          C.byref(rep)))
        return R.reshape(3, 3), t, {k: int(getattr(rep, k)) for k, _ in GlobalReport._fields_}

    def inliers(self):
        """The last gate of the last gated run() -> (mask: bool (np_local,), caller's order; K over all ranks)."""
        mask = np.zeros(self._np_local, dtype=np.uint8)
        k = C.c_longlong(0)
        self._check(lib().icp_get_inliers(self._h, mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(k)))
        return mask.astype(bool), int(k.value)

    def inlier_trace(self) -> np.ndarray:
        """K of each recorded iteration of the last gated run() (int64)."""
        n = lib().icp_get_inlier_trace(self._h, None, 0)
        if n < 0:
            self._check(n)
        out = np.zeros(max(n, 1), dtype=np.int64)
        rc = lib().icp_get_inlier_trace(self._h, out.ctypes.data_as(C.POINTER(C.c_longlong)), n)
        if rc < 0:
            self._check(rc)
        return out[:n]

    def set_trim(self, fraction: float):
        """icp_set_trim: run() keeps, in every iteration, the fraction of the pairs with the smallest
        distances (ties at the cut included); 1: off."""
        self._check(lib().icp_set_trim(self._h, float(fraction)))

    def set_one_to_one(self, on):
        """icp_set_one_to_one: run() keeps, of all the pairs that chose one model point, only the closest
        (ties whole); False: off.  Combines with the gate, the trim, robust weights and every metric."""
        self._check(lib().icp_set_one_to_one(self._h, int(on)))

    def trim_trace(self) -> np.ndarray:
        """C, the selected squared distance, of each recorded iteration of the last trimmed run() (float64)."""
        n = lib().icp_get_trim_trace(self._h, None, 0)
        if n < 0:
            self._check(n)
        out = np.zeros(max(n, 1))
        rc = lib().icp_get_trim_trace(self._h, _dp(out), n)
        if rc < 0:
            self._check(rc)
        return out[:n]

    def set_robust(self, kind: int, k: float = 0.0):
        """icp_set_robust: run() weighs every kept pair by ROBUST_HUBER / ROBUST_TUKEY / ROBUST_CAUCHY of
        its residual with the scale k (the clouds' units); ROBUST_NONE (k ignored): off."""
        self._check(lib().icp_set_robust(self._h, int(kind), float(k)))

    def robust_trace(self):
        """Of each recorded iteration of the last robust run() -> (W: the kept pairs' weights summed
        (float64), K+: the kept pairs with a weight > 0 (int64)), over all ranks."""
        n = lib().icp_get_robust_trace(self._h, None, None, 0)
        if n < 0:
            self._check(n)
        w = np.zeros(max(n, 1))
        kpos = np.zeros(max(n, 1), dtype=np.int64)
        rc = lib().icp_get_robust_trace(self._h, _dp(w), kpos.ctypes.data_as(C.POINTER(C.c_longlong)), n)
        if rc < 0:
            self._check(rc)
        return w[:n], kpos[:n]

    def run(self, max_iter: int, threshold: float = 1e-5):
        errs = np.zeros(max(max_iter, 1))
        res = Result()
        self._check(lib().icp_run(self._h, max_iter, threshold, _dp(errs), C.byref(res)))
        return res, errs[: res.iterations].copy()

    # per-operation surface
    def closest_matrix(self, p):
        p = _cloud(p)
        y = np.empty_like(p); idx = np.empty(p.shape[0], dtype=np.int32)
        self._check(lib().icp_closest_matrix(self._h, _dp(p), p.shape[0], _dp(y),
                                             idx.ctypes.data_as(C.POINTER(C.c_int32))))
        return y, idx

    def subtract_col(self, xyz, m):
        """substract_col_w (compute.cu:381-416): xyz - m for a caller-given 3-vector m."""
        xyz = _cloud(xyz)
        out = np.empty_like(xyz)
        self._check(lib().icp_subtract_col(self._h, _dp(xyz), xyz.shape[0], _dp(_vec(m, 3)), _dp(out)))
        return out

    def get_indices(self) -> np.ndarray:
        """Correspondences of the last search over the resident scene (np_local int32)."""
        idx = np.empty(self._np_local, dtype=np.int32)
        self._check(lib().icp_get_indices(self._h, idx.ctypes.data_as(C.POINTER(C.c_int32))))
        return idx

    def model_order(self, nm: int) -> np.ndarray:
        """The bundle filter's kd order of the resident model (icp_get_model_order)."""
        kd = np.empty(nm, dtype=np.int32)
        self._check(lib().icp_get_model_order(self._h, kd.ctypes.data_as(C.POINTER(C.c_int32))))
        return kd

    def get_grid(self, nm: int) -> dict:
        """The resident model's grid (icp_get_grid): g (3 ints), lo (3 doubles), inv_h, start
        (ncell + 1 int32), order (nm int32: each sorted position's model index)."""
        g = (C.c_int * 3)()
        lo = (C.c_double * 3)()
        inv_h = C.c_double()
        self._check(lib().icp_get_grid(self._h, g, lo, C.byref(inv_h), None, None))
        ncell = g[0] * g[1] * g[2]
        start = np.empty(ncell + 1, dtype=np.int32)
        order = np.empty(nm, dtype=np.int32)
        self._check(lib().icp_get_grid(self._h, g, lo, C.byref(inv_h), start.ctypes.data_as(C.POINTER(C.c_int32)),
                                       order.ctypes.data_as(C.POINTER(C.c_int32))))
        return dict(g=np.array(g[:]), lo=np.array(lo[:]), inv_h=inv_h.value, start=start, order=order)

    def set_index_digest(self, cap: int):
        self._check(lib().icp_set_index_digest(self._h, cap))
        self._digest_cap = cap

    def set_cert_audit(self, on: bool):
        self._check(lib().icp_set_cert_audit(self._h, 1 if on else 0))

    def bundle_audit(self, groups: int = 64) -> dict:
        """The bundle bound's exclusions checked on `groups` 32-query groups of the resident
        scene (icp_bundle_audit): max MFMA error over its margin, and the excluded bundles'
        geometry (violations must be 0)."""
        out = BundleAudit()
        self._check(lib().icp_bundle_audit(self._h, int(groups), C.byref(out)))
        return {f: getattr(out, f) for f, _ in BundleAudit._fields_}

    def index_digest(self, k: int | None = None) -> np.ndarray:
        """(k, 3) uint64: per icp_run iteration (sum idx, sum (j+1) idx[j], #{idx[j] == j})."""
        k = self._digest_cap if k is None else k
        out = np.zeros((max(k, 1), 3), dtype=np.uint64)
        self._check(lib().icp_get_index_digest(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), k))
        return out[:k]

    def compute_centroid(self, xyz, centred: bool = True):
        xyz = _cloud(xyz)
        mu = np.zeros(3); out = np.empty_like(xyz) if centred else None
        self._check(lib().icp_compute_centroid(self._h, _dp(xyz), xyz.shape[0], _dp(mu),
                                               _dp(out) if centred else None))
        return mu, out

    def y_p_norm(self, y, p):
        y = _cloud(y); p = _cloud(p)
        d = C.c_double(0.0); s = C.c_double(0.0)
        self._check(lib().icp_y_p_norm(self._h, _dp(y), _dp(p), y.shape[0], C.byref(d), C.byref(s)))
        return d.value, s.value

    def err_compute(self, y, p, in_place: bool, sR, t):
        y = _cloud(y); p = _cloud(p).copy()
        sR = _vec(sR, 9); t = _vec(t, 3); e = C.c_double(0.0)
        self._check(lib().icp_err_compute(self._h, _dp(y), _dp(p), y.shape[0], 1 if in_place else 0,
                                          _dp(sR), _dp(t), C.byref(e)))
        return e.value, p

    def find_alignment(self, p, y):
        p = _cloud(p); y = _cloud(y)
        s = C.c_double(0.0); R = np.zeros(9); t = np.zeros(3); e = C.c_double(0.0)
        self._check(lib().icp_find_alignment(self._h, _dp(p), _dp(y), p.shape[0], C.byref(s), _dp(R),
                                             _dp(t), C.byref(e)))
        return s.value, R.reshape(3, 3), t, e.value

    def stats(self) -> dict:
        st = Stats()
        self._check(lib().icp_get_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in Stats._fields_}

    def reset_stats(self):
        self._check(lib().icp_reset_stats(self._h))

    def set_bundle_counters(self, on: bool):
        self._check(lib().icp_set_bundle_counters(self._h, 1 if on else 0))

    def bundle_counters(self) -> dict:
        """The bundle filter's executed work since set_bundle_counters(True)."""
        out = (C.c_uint64 * 16)()
        self._check(lib().icp_get_bundle_counters(self._h, out))
        tasks = max(int(out[7]), 1)
        return {"stream_mfma": int(out[8]), "block_triggers": int(out[0]), "group_tests": int(out[1]),
                "pair_tests": int(out[2]), "wave_tasks": int(out[7]),
                "us_per_wave_task": {"prologue": out[3] * 0.01 / tasks, "stream": out[4] * 0.01 / tasks,
                                     "deferred": out[5] * 0.01 / tasks, "epilogue": out[6] * 0.01 / tasks},
                "deferred_us_per_wave_task": {"bound_tests": out[10] * 0.01 / tasks,
                                              "pair_block_waits": out[11] * 0.01 / tasks,
                                              "pair_tests": out[12] * 0.01 / tasks},
                "slowest_task_us_total": out[9] * 0.01}

    def comm_info(self) -> dict:
        """RCCL communicator size / rank (None / this rank without one) and the PCI bus id of
        this context's device: what a multi-GPU run really ran on."""
        cnt, rk = C.c_int(0), C.c_int(0)
        bus = C.create_string_buffer(64)
        self._check(lib().icp_get_comm_info(self._h, C.byref(cnt), C.byref(rk), bus, 64))
        return {"comm_count": cnt.value if cnt.value >= 0 else None, "comm_rank": rk.value,
                "pci_bus_id": bus.value.decode()}


# ---------------------------------------------------------------------------------
# reference-shaped API (src/GPU/gpu.hh)
# ---------------------------------------------------------------------------------

def register_pyramid(ctx: Context, m, p, voxels, max_iter: int, level_iter: int | None = None,
                     threshold: float = 1e-5, estimate_normals: int | None = None,
                     estimate_scene_normals: int | None = None):
    """Coarse-to-fine registration of the scene p onto the model m from the engine's own calls (the
    icp-gpu CLI's --pyramid makes the same calls in the same order).  For each voxel size, in the
    order given (coarse to fine): downsample both clouds, set them with the unequal-size check
    lifted, move the scene by the pose so far (transform_scene), run level_iter (default max_iter)
    iterations with the context's own settings (gate, robust weights, metric), take the total
    (transform).  Then the full clouds: set them, apply the pose, run max_iter iterations.
    estimate_normals = K: the model's normals are estimated at every level (and for the full
    clouds) from K neighbours; a level whose model has fewer than K points raises before any run.
    estimate_scene_normals = K: likewise the scene's normals (the symmetric iteration,
    set_plane_symmetric), estimated after each level's set_scene and before its transform_scene; a
    level whose scene has fewer than K points raises before any run.
    -> (the fine run's Result, the total (s, R, t), the records: one dict per level -- voxel,
    model_points, scene_points, iterations, err, converged, errs -- and a last one, voxel None, for
    the fine run)."""
    m = _cloud(m)
    p = _cloud(p)
    voxels = [float(h) for h in voxels]
    if any(not (h > 0.0) or not np.isfinite(h) for h in voxels):
        raise ValueError("voxel sizes must be finite and > 0")
    k_iter = max_iter if level_iter is None else int(level_iter)
    allow = getattr(ctx, "_allow_unequal", False)
    clouds = [(h, ctx.voxel_downsample(m, h), ctx.voxel_downsample(p, h)) for h in voxels]
    if estimate_normals is not None:
        for h, mc, _ in clouds:
            if mc.shape[0] < estimate_normals:
                raise ValueError(f"--estimate-normals {estimate_normals}: the level h={h:g} has a model of "
                                 f"{mc.shape[0]} points")
    if estimate_scene_normals is not None:
        for h, _, pc in clouds:
            if pc.shape[0] < estimate_scene_normals:
                raise ValueError(f"--estimate-scene-normals {estimate_scene_normals}: the level h={h:g} has a scene of "
                                 f"{pc.shape[0]} points")
    clouds.append((None, m, p))
    pose = (1.0, np.eye(3), np.zeros(3))
    records = []
    res = None
    try:
        for h, mc, pc in clouds:
            ctx.set_allow_unequal(True if h is not None else allow)
            ctx.set_model(mc)
            if estimate_normals is not None:
                ctx.estimate_model_normals(estimate_normals)
            ctx.set_scene(pc)
            if estimate_scene_normals is not None:
                ctx.estimate_scene_normals(estimate_scene_normals)
            ctx.transform_scene(*pose)
            res, errs = ctx.run(max_iter if h is None else k_iter, threshold)
            pose = ctx.transform()
            records.append({"voxel": h, "model_points": mc.shape[0], "scene_points": pc.shape[0],
                            "iterations": res.iterations, "err": float(res.err), "converged": bool(res.converged),
                            "errs": errs})
    finally:
        ctx.set_allow_unequal(allow)
    return res, pose, records


def match_plan(na: int, nb: int):
    """icp_match_features_plan -> (tile, chunk, splits): the rows of fb staged at a time, the rows of a
    workgroup's range and the number of ranges for these sizes."""
    tile, chunk, splits = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = lib().icp_match_features_plan(int(na), int(nb), C.byref(tile), C.byref(chunk), C.byref(splits))
    if rc != ICP_OK:
        raise ICPError(rc, strerror(rc))
    return tile.value, chunk.value, splits.value


def register_global(ctx: Context, m, p, voxel: float, max_iter: int, threshold: float = 1e-5,
                    estimate_normals: int | None = None, estimate_scene_normals: int | None = None, **global_opts):
    """Registration of a scene p that need not start near the model m (the icp-gpu CLI's --global makes
    the same calls in the same order): global_pose(m, p, voxel, **global_opts), set_model / set_scene of
    the full clouds, the requested normal estimates (before the scene moves: estimate_scene_normals needs
    the scene as given), transform_scene by the global pose, run(max_iter, threshold) with the context's
    own settings, transform().
    -> (the run's Result, its error trace, the total (s, R, t), the global pose (R, t), its report)."""
    m = _cloud(m)
    p = _cloud(p)
    R0, t0, report = ctx.global_pose(m, p, voxel, **global_opts)
    ctx.set_model(m)
    if estimate_normals is not None:
        ctx.estimate_model_normals(estimate_normals)
    ctx.set_scene(p)
    if estimate_scene_normals is not None:
        ctx.estimate_scene_normals(estimate_scene_normals)
    ctx.transform_scene(1.0, R0, t0)
    res, errs = ctx.run(max_iter, threshold)
    return res, errs, ctx.transform(), (R0, t0), report


def evaluate_registration(ctx: Context, m, p, max_dist: float, pose=None, both: bool = False) -> dict:
    """Open3D's evaluate_registration on this engine: set_model(m), set_scene(p), the scene moved by
    pose = (s, R, t) (None: as given) with transform_scene, then ctx.evaluate(max_dist, both)."""
    ctx.set_model(_cloud(m))
    ctx.set_scene(_cloud(p))
    if pose is not None:
        s, R, t = pose
        ctx.transform_scene(float(s), R, t)
    return ctx.evaluate(max_dist, both=both)


@dataclass
class ICP:
    """GPU::ICP (src/GPU/gpu.hh:41-104): ICP(m, p, max_iter); find_corresponding_opti()."""
    m: np.ndarray
    p: np.ndarray
    max_iter: int
    nn_mode: int = NN_CERTIFIED
    device: int = 0
    threshold: float = 1e-5  # src/GPU/gpu.hh:103
    allow_unequal: bool = False
    max_distance: float | None = None  # icp_set_max_distance (None: no gate)
    normals: np.ndarray | None = None  # the model's normals: the point-to-plane metric (None: point-to-point)
    estimate_normals: int | None = None  # k: the normals estimated from the model (estimate_model_normals), same metric
    robust: tuple | None = None  # (kind, k): icp_set_robust (None: every kept pair with weight 1)
    trim: float | None = None  # icp_set_trim: the fraction of the pairs each iteration keeps (None: all)
    scene_normals: np.ndarray | None = None  # the scene's normals too: the symmetric iteration (needs model normals)
    plane_to_plane: float | None = None  # epsilon: the plane-to-plane iteration (generalised ICP) instead of the
    # symmetric one, from the same two sets of normals (the two forms exclude each other; needs scene_normals)
    one_to_one: bool = False  # icp_set_one_to_one: a model point keeps its closest pair alone
    new_p: np.ndarray = field(init=False)
    s: float = field(init=False, default=1.0)
    r: np.ndarray = field(init=False)
    t: np.ndarray = field(init=False)
    errors: np.ndarray = field(init=False)

    def __post_init__(self):
        if self.normals is not None and self.estimate_normals is not None:
            raise ValueError("ICP: give either normals or estimate_normals, not both")
        if self.plane_to_plane is not None and self.scene_normals is None:
            raise ValueError("ICP: plane_to_plane needs scene_normals (and normals or estimate_normals)")
        self.m = _cloud(self.m); self.p = _cloud(self.p)
        self.new_p = self.p.copy()
        self.r = np.eye(3); self.t = np.zeros(3)
        self.errors = np.zeros(0)
        self._ctx = Context(self.device, self.nn_mode)
        self._ctx.set_allow_unequal(self.allow_unequal)
        if self.max_distance is not None:
            self._ctx.set_max_distance(self.max_distance)
        if self.trim is not None:
            self._ctx.set_trim(self.trim)
        if self.one_to_one:
            self._ctx.set_one_to_one(True)
        if self.robust is not None:
            self._ctx.set_robust(*self.robust)
        self._ctx.set_model(self.m)
        if self.normals is not None:
            self._ctx.set_model_normals(self.normals)
            self._ctx.set_metric(METRIC_POINT_TO_PLANE)
        if self.estimate_normals is not None:
            self._ctx.estimate_model_normals(self.estimate_normals)
            self._ctx.set_metric(METRIC_POINT_TO_PLANE)
        self._ctx.set_scene(self.p)
        if self.scene_normals is not None:
            if self.normals is None and self.estimate_normals is None:
                raise ValueError("ICP: scene_normals need the model's normals (normals or estimate_normals)")
            self._ctx.set_scene_normals(self.scene_normals)
            if self.plane_to_plane is not None:  # (one form at a time: icp_run refuses both switches)
                self._ctx.set_plane_to_plane(self.plane_to_plane)
            else:
                self._ctx.set_plane_symmetric(True)

    def find_corresponding_opti(self):
        res, errs = self._ctx.run(self.max_iter, self.threshold)
        self.errors = errs
        self.s, self.r, self.t = res.s, np.array(res.R).reshape(3, 3), np.array(res.t)
        self.new_p = self._ctx.get_scene()
        return res

    def find_alignment(self, y):
        s, R, t, e = self._ctx.find_alignment(self.new_p, y)
        self.s, self.r, self.t = s, R, t
        return e

    def compute_y_naive(self):
        """gpu.cc:6-15: one NN search per scene point (compute_distance_w_naive)."""
        Y = np.empty_like(self.new_p)
        for j in range(self.new_p.shape[0]):
            Y[j] = self.m[compute_distance_w_naive(self.m, self.new_p[j], self._ctx)]
        return Y

    def find_corresponding_naive(self):
        """gpu.cc:17-49: the per-point loop; err = (find_alignment + transform residual)/np,
        stop after the iteration whose err < threshold.  Same results as the opti loop."""
        if self.p.shape[0] != self.m.shape[0] and not self.allow_unequal:
            raise ICPError(ICP_E_SIZE_MISMATCH, "Point sets need to have the same number of points.")
        if self.p.shape[0] < 4:
            raise ICPError(ICP_E_TOO_FEW_POINTS, "Need at least 4 point pairs")
        errs = []
        for _ in range(self.max_iter):
            Y = self.compute_y_naive()
            err = self.find_alignment(Y)
            e2, self.new_p = self._ctx.err_compute(Y, self.new_p, True, self.s * self.r, self.t)
            err = (err + e2) / self.p.shape[0]
            errs.append(err)
            if err < self.threshold:
                break
        self.errors = np.array(errs)
        return len(errs)


_default_ctx: Context | None = None


def _ctx_for_model(m) -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    _default_ctx.set_model(m)
    return _default_ctx


def compute_distance_w_naive(m, pi, ctx: Context | None = None) -> int:
    """compute.cu:279-308: index of the first nearest model point of one query point."""
    c = ctx if ctx is not None else _ctx_for_model(m)
    _, idx = c.closest_matrix(np.asarray(pi, dtype=np.float64).reshape(1, 3))
    return int(idx[0])


def compute_Y_w_opti(m, p):
    """compute.cu:154-245: Y[j] = m[NN(p_j)] (returns Y, idx)."""
    return _ctx_for_model(m).closest_matrix(p)


def compute_err_w(Y, p, in_place: bool, sr, t):
    """compute.cu:348-379 -> (err, p_after)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx.err_compute(Y, p, in_place, sr, t)


def compute_centroid(M):
    """rowwise().mean() + substract_col_w (gpu.cc:98-102) on the device -> (mu, M - mu)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx.compute_centroid(M, centred=True)
