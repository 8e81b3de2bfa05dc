"""ctypes binding of ``libgs_hip.so`` -- the same C ABI (``include/gs_hip.h``) that the
reference-side Rust shim binds (``rust/compute_hip/src/ffi.rs``).

There is deliberately NO fallback: if the HIP library is missing or a call fails, this
module raises (``GsError``).  Nothing here imports ``oracle``.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GS_HIP_LIBRARY names another build of the same ABI (A/B timing of kernel variants, tools/ab_build.py);
# it is loaded instead of, never as a fallback for, the in-tree library.
LIB_PATH = os.environ.get("GS_HIP_LIBRARY") or os.path.join(_HERE, "libgs_hip.so")

GS_OK = 0
GS_ERR_INVALID = -1
GS_ERR_HIP = -2
GS_ERR_RCCL = -3
GS_ERR_NO_DEVICE = -4
GS_ERR_UNSUPPORTED = -5
GS_ERR_NOMEM = -6

GS_MATH_STRICT, GS_MATH_FUSED = 0, 1
GS_KERNEL_AUTO, GS_KERNEL_SIMPLE, GS_KERNEL_STREAM, GS_KERNEL_TB, GS_KERNEL_LDS, GS_KERNEL_TILE, GS_KERNEL_WINDOW = 0, 1, 2, 3, 4, 5, 6
GS_BOUNDARY_CLIPPED, GS_BOUNDARY_ZERO_HALO, GS_BOUNDARY_PERIODIC, GS_BOUNDARY_NEUMANN = 0, 1, 2, 3
GS_UNIQUE_ID_BYTES = 128
GS_REGION_PAIRS_MAX = 1 << 25  # counters per field of one gs_fields_region_correlation call (include/gs_hip.h)
GS_REGION_HIST_MAX = 1 << 25  # counters per field of one gs_fields_region_histogram call (include/gs_hip.h)
GS_REGION_SPECTRUM_MAX = 1 << 25  # result words per field of one gs_fields_region_spectrum call (include/gs_hip.h)
GS_REGION_SPECTRUM_RECORDS_MAX = 1 << 27  # segment-record words over the fields of one such call (include/gs_hip.h)
GS_REGION_COMPONENTS_MAX = 1 << 20  # results per field of one gs_fields_region_components call (include/gs_hip.h)
GS_REGION_CHANGE_RECORDS_MAX = 1 << 28  # bytes of row records per slab of one gs_fields_region_compare call (include/gs_hip.h)
# time statistics (include/gs_hip.h): the groups of accumulators, the result planes and the raw accumulators
GS_TSTAT_SUM, GS_TSTAT_SQUARES, GS_TSTAT_EXTREMES, GS_TSTAT_CROSSINGS = 1, 2, 4, 8
GS_TSTAT_MEAN, GS_TSTAT_VARIANCE, GS_TSTAT_MIN, GS_TSTAT_MAX, GS_TSTAT_OCCUPANCY, GS_TSTAT_ARRIVAL = 0, 1, 2, 3, 4, 5
(GS_TSTAT_RAW_SUM, GS_TSTAT_RAW_SQUARES, GS_TSTAT_RAW_MIN, GS_TSTAT_RAW_MAX, GS_TSTAT_RAW_SET_COUNT,
 GS_TSTAT_RAW_FIRST_STAMP) = 0, 1, 2, 3, 4, 5

# Every symbol include/gs_hip.h declares; tests check that the library exports them all.
EXPORTS = (
    "gs_default_params", "gs_default_options", "gs_abi_version", "gs_last_error",
    "gs_device_count", "gs_get_unique_id", "gs_ctx_create", "gs_ctx_destroy",
    "gs_ctx_set_params", "gs_field_create", "gs_field_destroy", "gs_field_shape",
    "gs_field_local_rows", "gs_field_raw_shape", "gs_field_fill", "gs_field_fill_slice",
    "gs_field_finalize", "gs_field_upload", "gs_field_download", "gs_field_device_ptr",
    "gs_step", "gs_run", "gs_sync", "gs_timer_start", "gs_timer_stop", "gs_ctx_info",
    "gs_host_alloc", "gs_host_free", "gs_field_download_async", "gs_download_wait",
    "gs_ctx_get_tuned", "gs_ctx_set_tuned", "gs_ctx_comm_info", "gs_field_colormap",
    "gs_ctx_stats", "gs_ctx_set_pass_timing", "gs_field_mark_written", "gs_rccl_selftest",
    "gs_runtime_info", "gs_fields_place", "gs_debug_dyn_lds_key", "gs_debug_window_plan",
    "gs_debug_place_stats", "gs_debug_exchange_probe_create", "gs_debug_exchange_probe_run",
    "gs_debug_exchange_probe_destroy", "gs_download_wait_but",
    "gs_ensemble_create", "gs_ensemble_destroy", "gs_ensemble_shape", "gs_ensemble_set_params", "gs_ensemble_seed",
    "gs_ensemble_upload", "gs_ensemble_download", "gs_ensemble_run",
    "gs_ctx_set_param_map",
    "gs_ctx_set_mask",
    "gs_ctx_set_noise", "gs_ctx_get_noise",
    "gs_fields_summarize", "gs_members_summarize",
    "gs_fields_histogram", "gs_members_histogram",
    "gs_field_reduced_shape", "gs_field_download_reduced", "gs_field_download_reduced_async", "gs_field_colormap_reduced",
    "gs_fields_compare", "gs_members_compare", "gs_fields_copy", "gs_members_copy",
    "gs_members_set_active", "gs_members_get_active",
    "gs_members_set_noise", "gs_members_get_noise", "gs_members_clear_noise",
    "gs_fields_morphology", "gs_members_morphology",
    "gs_region_grid", "gs_fields_region_summaries", "gs_fields_region_morphology", "gs_fields_region_correlation",
    "gs_fields_region_histogram", "gs_fields_region_components", "gs_fields_region_compare", "gs_fields_region_spectrum",
    "gs_fields_correlation", "gs_members_correlation",
    "gs_spectrum_tables", "gs_fields_spectrum", "gs_members_spectrum",
    "gs_fields_components", "gs_members_components",
    "gs_field_component_list", "gs_members_component_list", "gs_component_list_view", "gs_component_list_destroy",
    "gs_fields_match", "gs_members_match", "gs_component_match_view", "gs_component_match_destroy",
    "gs_time_stats_create", "gs_time_stats_destroy", "gs_time_stats_reset", "gs_time_stats_accumulate", "gs_time_stats_samples",
    "gs_time_stats_result", "gs_time_stats_download",
    "gs_members_time_stats_create", "gs_members_time_stats_accumulate", "gs_members_time_stats_result",
    "gs_members_bundle_stats",
    "gs_ctx_quiet_stats", "gs_ctx_quiet_edge_stats",
)


class GsError(RuntimeError):
    """A non-zero ``gs_status`` (the Rust shim maps the same codes to ``HipError``)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"gs_hip error {code}: {message}")
        self.code = code
        self.message = message


class GsParams(ctypes.Structure):
    """``gs_params`` = ``Parameters`` (data/src/parameters.rs:13-33)."""

    _fields_ = [
        ("w", (ctypes.c_float * 3) * 3),
        ("du", ctypes.c_float),
        ("dv", ctypes.c_float),
        ("feed", ctypes.c_float),
        ("kill", ctypes.c_float),
        ("dt", ctypes.c_float),
    ]


class GsOptions(ctypes.Structure):
    _fields_ = [
        ("math", ctypes.c_int32),
        ("kernel", ctypes.c_int32),
        ("rows_per_block", ctypes.c_int32),
        ("fuse_steps", ctypes.c_int32),
        ("use_graph", ctypes.c_int32),
        ("pitch_pad", ctypes.c_int32),
        ("split", ctypes.c_int32),
        ("general_kernels", ctypes.c_int32),
        ("cols_per_lane", ctypes.c_int32),
        ("boundary", ctypes.c_int32),
        ("no_tune", ctypes.c_int32),
        ("tile_shape", ctypes.c_int32),
        ("share_taps", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 3),
    ]


class GsStats(ctypes.Structure):
    """``gs_stats`` (include/gs_hip.h)."""

    _fields_ = [
        ("passes", ctypes.c_uint64),
        ("steps", ctypes.c_uint64),
        ("launches", ctypes.c_uint64),
        ("ghost_refreshes", ctypes.c_uint64),
        ("timed_passes", ctypes.c_uint64),
        ("halo_ms", ctypes.c_float),
        ("interior_ms", ctypes.c_float),
        ("halo_exposed_ms", ctypes.c_float),
        ("reserved", ctypes.c_float),
        ("window_fallbacks", ctypes.c_uint64),
    ]


class GsNoise(ctypes.Structure):
    """``gs_noise`` (include/gs_hip.h): the two sigmas, the seed and the index of the next step -- 24 bytes."""

    _fields_ = [
        ("sigma_u", ctypes.c_float),
        ("sigma_v", ctypes.c_float),
        ("seed", ctypes.c_uint64),
        ("step", ctypes.c_uint64),
    ]


class GsSummary(ctypes.Structure):
    """``gs_summary`` (include/gs_hip.h): one plane's sum, sum of squares, min and max of its finite cells, and its
    count of non-finite cells -- 32 bytes."""

    _fields_ = [
        ("sum", ctypes.c_double),
        ("sum_sq", ctypes.c_double),
        ("min", ctypes.c_float),
        ("max", ctypes.c_float),
        ("nonfinite", ctypes.c_uint64),
    ]


class GsChange(ctypes.Structure):
    """``gs_change`` (include/gs_hip.h): how far one plane is from another -- the sums of |d| and d * d and the largest |d|
    over the cells where both are finite (d = a - b in f64), the count of cells whose bits differ and the count of cells
    where either is not finite -- 40 bytes."""

    _fields_ = [
        ("sum_abs", ctypes.c_double),
        ("sum_sq", ctypes.c_double),
        ("max_abs", ctypes.c_double),
        ("differing", ctypes.c_uint64),
        ("nonfinite", ctypes.c_uint64),
    ]


class GsMorphology(ctypes.Structure):
    """``gs_morphology`` (include/gs_hip.h): the bit-quad counts of one thresholded plane -- Q0, Q1, Q2, Q3, Q4, QD -- 48
    bytes."""

    _fields_ = [("quads", ctypes.c_uint64 * 6)]


class GsComponents(ctypes.Structure):
    """``gs_components`` (include/gs_hip.h): the connected components of one thresholded plane -- their number, the sum of
    their sizes, the largest, and how many fall into each power-of-two size bin -- 280 bytes."""

    _fields_ = [
        ("components", ctypes.c_uint64),
        ("set_cells", ctypes.c_uint64),
        ("largest", ctypes.c_uint64),
        ("by_size", ctypes.c_uint64 * 32),
    ]


class GsComponentRecord(ctypes.Structure):
    """``gs_component_record`` (include/gs_hip.h): one connected component of a thresholded plane -- its cells, the sums of
    their row and column indices, its first cell in row-major order and its bounding box (inclusive) -- 48 bytes."""

    _fields_ = [
        ("size", ctypes.c_uint64),
        ("sum_row", ctypes.c_uint64),
        ("sum_col", ctypes.c_uint64),
        ("first_row", ctypes.c_uint32),
        ("first_col", ctypes.c_uint32),
        ("row_min", ctypes.c_uint32),
        ("row_max", ctypes.c_uint32),
        ("col_min", ctypes.c_uint32),
        ("col_max", ctypes.c_uint32),
    ]


class GsComponentOverlap(ctypes.Structure):
    """``gs_component_overlap`` (include/gs_hip.h): a before-record and an after-record of a ``gs_component_match`` that
    share ``cells`` grid cells -- 16 bytes."""

    _fields_ = [
        ("before", ctypes.c_uint32),
        ("after", ctypes.c_uint32),
        ("cells", ctypes.c_uint64),
    ]


_lib = None


def load() -> ctypes.CDLL:
    """Load ``libgs_hip.so`` (building is ``__graft_entry__.build()``'s job); raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GsError(GS_ERR_NO_DEVICE,
                      f"{LIB_PATH} is missing: build it with `python -m grayscott_amd._build` "
                      "(there is no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32, u64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_float
    u32 = ctypes.c_uint32
    P = ctypes.POINTER
    sig = {
        "gs_default_params": (None, [P(GsParams)]),
        "gs_default_options": (None, [P(GsOptions)]),
        "gs_abi_version": (i32, []),
        "gs_last_error": (ctypes.c_char_p, []),
        "gs_device_count": (i32, [P(i32)]),
        "gs_get_unique_id": (i32, [vp]),
        "gs_ctx_create": (i32, [P(vp), P(GsParams), P(GsOptions), P(i32), i32, i32, i32, vp]),
        "gs_ctx_destroy": (i32, [vp]),
        "gs_ctx_set_params": (i32, [vp, P(GsParams)]),
        "gs_ctx_set_param_map": (i32, [vp, vp, vp]),
        "gs_ctx_set_mask": (i32, [vp, vp]),
        "gs_ctx_set_noise": (i32, [vp, P(GsNoise)]),
        "gs_ctx_get_noise": (i32, [vp, P(GsNoise), P(i32)]),
        "gs_field_create": (i32, [vp, P(vp), u64, u64]),
        "gs_field_destroy": (i32, [vp, vp]),
        "gs_field_shape": (i32, [vp, P(u64), P(u64)]),
        "gs_field_local_rows": (i32, [vp, P(u64), P(u64)]),
        "gs_field_raw_shape": (i32, [vp, P(u64), P(u64)]),
        "gs_field_fill": (i32, [vp, vp, f32]),
        "gs_field_fill_slice": (i32, [vp, vp, u64, u64, u64, u64, f32]),
        "gs_field_finalize": (i32, [vp, vp]),
        "gs_field_upload": (i32, [vp, vp, vp]),
        "gs_field_download": (i32, [vp, vp, vp]),
        "gs_field_device_ptr": (i32, [vp, i32, P(vp), P(u64), P(u64), P(u64), P(i32)]),
        "gs_step": (i32, [vp, vp, vp, vp, vp]),
        "gs_run": (i32, [vp, vp, vp, vp, vp, u64, P(i32)]),
        "gs_sync": (i32, [vp]),
        "gs_timer_start": (i32, [vp]),
        "gs_timer_stop": (i32, [vp, P(f32)]),
        "gs_ctx_info": (i32, [vp, ctypes.c_char_p, ctypes.c_size_t, P(u64)]),
        "gs_host_alloc": (i32, [P(vp), u64]),
        "gs_host_free": (i32, [vp]),
        "gs_field_download_async": (i32, [vp, vp, vp]),
        "gs_download_wait": (i32, [vp]),
        "gs_ctx_get_tuned": (i32, [vp, u64, u64, P(i32), P(i32), P(i32), P(i32)]),
        "gs_ctx_set_tuned": (i32, [vp, u64, u64, i32, i32, i32, i32]),
        "gs_ctx_comm_info": (i32, [vp, P(i32), P(i32), P(i32)]),
        "gs_field_colormap": (i32, [vp, vp, f32, vp, i32, vp]),
        "gs_ctx_stats": (i32, [vp, P(GsStats)]),
        "gs_ctx_set_pass_timing": (i32, [vp, i32]),
        "gs_ctx_quiet_stats": (i32, [vp, P(u64)]),
        "gs_ctx_quiet_edge_stats": (i32, [vp, P(u64)]),
        "gs_field_mark_written": (i32, [vp, vp]),
        "gs_rccl_selftest": (i32, [i32, u64]),
        "gs_runtime_info": (i32, [i32, ctypes.c_char_p, ctypes.c_size_t]),
        "gs_fields_place": (i32, [vp, P(vp), i32, P(f32), P(f32)]),
        "gs_debug_place_stats": (i32, [vp, P(u64), P(u64)]),
        "gs_download_wait_but": (i32, [vp, i32]),
        "gs_debug_exchange_probe_create": (i32, [i32, i32, i32, u64, P(vp)]),
        "gs_debug_exchange_probe_run": (i32, [vp, P(f32), P(f32)]),
        "gs_debug_exchange_probe_destroy": (i32, [vp]),
        "gs_ensemble_create": (i32, [vp, P(vp), u64, u64, u64]),
        "gs_ensemble_destroy": (i32, [vp, vp]),
        "gs_ensemble_shape": (i32, [vp, P(u64), P(u64), P(u64)]),
        "gs_ensemble_set_params": (i32, [vp, vp, P(GsParams), u64]),
        "gs_ensemble_seed": (i32, [vp, vp]),
        "gs_ensemble_upload": (i32, [vp, vp, u64, u64, vp, vp]),
        "gs_ensemble_download": (i32, [vp, vp, u64, u64, i32, vp]),
        "gs_ensemble_run": (i32, [vp, vp, u64]),
        "gs_fields_summarize": (i32, [vp, P(vp), i32, P(GsSummary)]),
        "gs_members_summarize": (i32, [vp, vp, u64, u64, P(GsSummary)]),
        "gs_fields_histogram": (i32, [vp, P(vp), i32, P(f32), P(f32), i32, P(u64)]),
        "gs_members_histogram": (i32, [vp, vp, u64, u64, P(f32), P(f32), i32, P(u64)]),
        "gs_field_reduced_shape": (i32, [vp, i32, P(u64), P(u64), P(u64), P(u64)]),
        "gs_field_download_reduced": (i32, [vp, vp, i32, vp]),
        "gs_field_download_reduced_async": (i32, [vp, vp, i32, vp]),
        "gs_field_colormap_reduced": (i32, [vp, vp, i32, f32, vp, i32, vp]),
        "gs_fields_compare": (i32, [vp, P(vp), P(vp), i32, P(GsChange)]),
        "gs_fields_region_compare": (i32, [vp, P(vp), P(vp), i32, i32, i32, P(GsChange)]),
        "gs_members_compare": (i32, [vp, vp, vp, u64, u64, P(GsChange)]),
        "gs_fields_copy": (i32, [vp, P(vp), P(vp), i32]),
        "gs_members_copy": (i32, [vp, vp, vp, u64, u64]),
        "gs_members_set_active": (i32, [vp, vp, u64, u64, vp]),
        "gs_members_get_active": (i32, [vp, vp, u64, u64, vp, vp, P(u64)]),
        "gs_members_set_noise": (i32, [vp, vp, u64, u64, vp, u64]),
        "gs_members_get_noise": (i32, [vp, vp, u64, u64, vp, P(i32)]),
        "gs_members_clear_noise": (i32, [vp, vp]),
        "gs_fields_morphology": (i32, [vp, P(vp), i32, P(f32), P(i32), i32, P(GsMorphology)]),
        "gs_members_morphology": (i32, [vp, vp, u64, u64, P(f32), P(i32), i32, P(GsMorphology)]),
        "gs_region_grid": (i32, [u64, u64, i32, i32, P(u64), P(u64)]),
        "gs_fields_region_summaries": (i32, [vp, P(vp), i32, i32, i32, P(GsSummary)]),
        "gs_fields_region_morphology": (i32, [vp, P(vp), i32, i32, i32, P(f32), P(i32), i32, P(GsMorphology)]),
        "gs_fields_region_correlation": (i32, [vp, P(vp), i32, i32, i32, P(f32), P(i32), i32, i32, P(u64)]),
        "gs_fields_region_histogram": (i32, [vp, P(vp), i32, i32, i32, P(f32), P(f32), i32, P(u64)]),
        "gs_fields_components": (i32, [vp, P(vp), i32, P(f32), P(i32), i32, i32, P(GsComponents)]),
        "gs_fields_region_components": (i32, [vp, P(vp), i32, i32, i32, P(f32), P(i32), i32, i32, P(GsComponents)]),
        "gs_members_components": (i32, [vp, vp, u64, u64, P(f32), P(i32), i32, i32, P(GsComponents)]),
        "gs_field_component_list": (i32, [vp, vp, f32, i32, i32, u64, P(vp)]),
        "gs_members_component_list": (i32, [vp, vp, u64, u64, i32, f32, i32, i32, u64, P(vp)]),
        "gs_component_list_view": (i32, [vp, P(u64), P(P(u64)), P(P(GsComponentRecord))]),
        "gs_component_list_destroy": (i32, [vp]),
        "gs_fields_match": (i32, [vp, vp, vp, f32, i32, i32, u64, P(vp)]),
        "gs_members_match": (i32, [vp, vp, vp, u64, u64, i32, f32, i32, i32, u64, P(vp)]),
        "gs_component_match_view": (i32, [vp, P(vp), P(vp), P(u64), P(P(u64)), P(P(GsComponentOverlap))]),
        "gs_component_match_destroy": (i32, [vp]),
        "gs_fields_correlation": (i32, [vp, P(vp), i32, P(f32), P(i32), i32, i32, P(u64)]),
        "gs_members_correlation": (i32, [vp, vp, u64, u64, P(f32), P(i32), i32, i32, P(u64)]),
        "gs_spectrum_tables": (i32, [i32, P(f32), P(f32)]),
        "gs_fields_spectrum": (i32, [vp, P(vp), i32, i32, i32, P(ctypes.c_double), P(u64)]),
        "gs_members_spectrum": (i32, [vp, vp, u64, u64, i32, i32, P(ctypes.c_double), P(u64)]),
        "gs_fields_region_spectrum": (i32, [vp, P(vp), i32, i32, i32, i32, i32, P(ctypes.c_double), P(u64)]),
        "gs_time_stats_create": (i32, [vp, P(vp), u64, u64, i32, u32, P(f32), P(i32)]),
        "gs_time_stats_destroy": (i32, [vp, vp]),
        "gs_time_stats_reset": (i32, [vp, vp]),
        "gs_time_stats_accumulate": (i32, [vp, vp, P(vp), i32, u32]),
        "gs_time_stats_samples": (i32, [vp, P(u64)]),
        "gs_time_stats_result": (i32, [vp, vp, i32, i32, vp]),
        "gs_time_stats_download": (i32, [vp, vp, i32, i32, vp]),
        "gs_members_time_stats_create": (i32, [vp, P(vp), vp, u64, u64, u32, P(f32), P(i32)]),
        "gs_members_time_stats_accumulate": (i32, [vp, vp, vp, u32]),
        "gs_members_time_stats_result": (i32, [vp, vp, i32, i32, vp]),
        "gs_members_bundle_stats": (i32, [vp, vp, u64, u64, u64, P(i32), i32, P(f32), P(i32), P(vp), u64]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int) -> None:
    if status != GS_OK:
        msg = load().gs_last_error()
        raise GsError(status, msg.decode(errors="replace") if msg else "unknown error")


def default_params() -> GsParams:
    p = GsParams()
    load().gs_default_params(ctypes.byref(p))
    return p


def default_options() -> GsOptions:
    o = GsOptions()
    load().gs_default_options(ctypes.byref(o))
    return o


def device_count() -> int:
    n = ctypes.c_int32(0)
    status = load().gs_device_count(ctypes.byref(n))
    return int(n.value) if status == GS_OK else 0


def rccl_selftest(device: int = 0, floats: int = 1 << 16) -> None:
    """``gs_rccl_selftest``: raises ``GsError`` when RCCL cannot be loaded or a one-rank send / receive fails."""
    check(load().gs_rccl_selftest(device, floats))


def runtime_info(load_rccl: bool = False) -> dict:
    """``gs_runtime_info``: the HIP runtime and the RCCL this process's libgs_hip.so is bound to (paths, versions)."""
    import json

    buf = ctypes.create_string_buffer(2048)
    check(load().gs_runtime_info(1 if load_rccl else 0, buf, len(buf)))
    return json.loads(buf.value.decode())


def get_unique_id() -> bytes:
    buf = ctypes.create_string_buffer(GS_UNIQUE_ID_BYTES)
    check(load().gs_get_unique_id(buf))
    return buf.raw
