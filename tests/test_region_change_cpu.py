"""Regional state comparison (gs_fields_region_compare) without a GPU: the exports, the refusals that are decided before any
handle is looked at through the built library, the arithmetic of ``RegionChange``, the driver's flags, the kernels' resources
and the C++ mirror."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import change_ref, region_change_ref, regions_ref
from tests.children import ROOT, build_program, run_program

HEADER = os.path.join(ROOT, "include", "gs_hip.h")


def _prototype(text, name):
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_symbol_is_exported_declared_and_bound(built):
    import grayscott_amd
    from grayscott_amd import capi

    full = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    name = "gs_fields_region_compare"
    assert _prototype(text, name) == ["gs_ctx *ctx", "gs_field *const *a", "gs_field *const *b", "int32_t n", "int32_t rh",
                                      "int32_t rw", "gs_change *out"]
    assert "GS_HIP_REGION_CHANGE_ROUTE" in full and "#define GS_REGION_CHANGE_RECORDS_MAX (1ull << 28)" in full
    assert capi.GS_REGION_CHANGE_RECORDS_MAX == 1 << 28
    ffi = open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    assert f"pub fn {name}(" in ffi
    lib = capi.load()
    i32, vp, P = ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER
    assert name in capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).restype is i32
    assert getattr(lib, name).argtypes == [vp, P(vp), P(vp), i32, i32, i32, P(capi.GsChange)]
    assert ctypes.sizeof(capi.GsChange) == 40                              # no struct is added: the result is gs_change
    assert lib.gs_abi_version() == 4 and re.search(r"#define\s+GS_ABI_VERSION\s+4\b", full)
    hpp = open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    assert "region_changes_since(const Snapshot &snap" in hpp and "gs_fields_region_compare(context_->get()" in hpp
    assert "RegionChange" in grayscott_amd.__all__ and hasattr(grayscott_amd.simulation, "region_compare_fields")
    assert hasattr(grayscott_amd.HipConcentration, "region_change_from") and hasattr(grayscott_amd.Species, "region_changes_since")


def test_refusals_decided_before_any_handle_is_looked_at(built):
    from grayscott_amd import capi

    lib = capi.load()
    INV = capi.GS_ERR_INVALID
    F = lib.gs_fields_region_compare
    bogus = ctypes.c_void_p(0x10)                                         # never dereferenced: every call is refused first
    fields = (ctypes.c_void_p * 4)(None, None, None, None)
    out = (capi.GsChange * 16)()
    err = lambda: lib.gs_last_error().decode()  # noqa: E731

    assert F(None, fields, fields, 1, 4, 16, out) == INV and "null" in err()
    assert F(bogus, None, fields, 1, 4, 16, out) == INV and "null" in err()
    assert F(bogus, fields, None, 1, 4, 16, out) == INV and "null" in err()
    assert F(bogus, fields, fields, 1, 4, 16, None) == INV and "null" in err()
    assert F(bogus, fields, fields, 1, 0, 18, None) == INV and "null" in err()                  # null before everything
    for rh, rw in ((4, 12), (4, 18), (0, 16), (4, 0), (4, 8), (-1, 16), (4, -16)):
        for n in (1, 0, 5):                                                                     # the region shape before n
            assert F(bogus, fields, fields, n, rh, rw, out) == INV and "region" in err(), (rh, rw, n)
    for n in (0, 5, -1):                                                                        # then the handles
        assert F(bogus, fields, fields, n, 4, 16, out) == INV and "fields (1..4)" in err(), n
    assert F(bogus, fields, fields, 1, 4, 16, out) == INV and "field 0" in err()


def test_the_route_switch_refuses_what_it_does_not_know(built, monkeypatch):
    from grayscott_amd import capi

    lib = capi.load()
    fields = (ctypes.c_void_p * 4)(None, None, None, None)
    out = (capi.GsChange * 4)()
    monkeypatch.setenv("GS_HIP_REGION_CHANGE_ROUTE", "fastest")
    assert lib.gs_fields_region_compare(ctypes.c_void_p(0x10), fields, fields, 1, 4, 16, out) == capi.GS_ERR_INVALID
    assert "GS_HIP_REGION_CHANGE_ROUTE" in lib.gs_last_error().decode()
    for known in ("records", "wave", ""):
        monkeypatch.setenv("GS_HIP_REGION_CHANGE_ROUTE", known)
        assert lib.gs_fields_region_compare(ctypes.c_void_p(0x10), fields, fields, 1, 4, 16, out) == capi.GS_ERR_INVALID
        assert "field 0" in lib.gs_last_error().decode(), known


def test_the_reference_is_the_whole_grid_rule_on_the_crops():
    shape, region = (9, 300), (4, 64)
    a, b = change_ref.order_sensitive(shape, 5)
    a[0, 0], b[8, 299] = np.nan, np.inf
    got = region_change_ref.changes(a, b, region)
    assert got.shape == regions_ref.grid(shape, region) == (3, 5)
    for (at, ca), (_, cb) in zip(regions_ref.crops(a, region), regions_ref.crops(b, region)):
        assert change_ref.same(got[at], change_ref.literal(ca, cb)), at
    whole = change_ref.change(a, b)
    assert int(got["differing"].sum()) == whole["differing"] and int(got["nonfinite"].sum()) == whole["nonfinite"] == 2
    assert float(got["max_abs"].max()) == whole["max_abs"]
    assert region_change_ref.UNROLL == 4 and region_change_ref.BAND == 16
    kernels_h = open(os.path.join(ROOT, "grayscott_amd", "csrc", "gs_kernels.h")).read()
    assert "kRegionChangeUnroll = 4;" in kernels_h and "kRegionChangeBand = 16;" in kernels_h


def test_region_change_arithmetic():
    from grayscott_amd import Change, RegionChange

    shape, region = (5, 40), (4, 16)                                       # regions of 64, 64, 32 cells; 16, 16, 8 in the last row
    rec = np.zeros((2, 3), region_change_ref.CHANGE_DTYPE)
    rec["sum_abs"] = [[64.0, 3.0, 0.0], [8.0, 0.0, 0.0]]
    rec["sum_sq"] = [[256.0, 9.0, 0.0], [16.0, 0.0, 0.0]]
    rec["max_abs"] = [[2.5, 3.0, 0.0], [1e-4, 0.0, 0.0]]
    rec["differing"] = [[64, 1, 0], [16, 0, 8]]
    rec["nonfinite"] = [[0, 1, 0], [0, 0, 8]]
    c = RegionChange.from_records(rec, region, shape)
    assert c.shape == shape and c.region == region and c.sum_abs.shape == (2, 3)
    assert np.array_equal(c.size, [[64, 64, 32], [16, 16, 8]]) and c.size.dtype == np.int64
    assert np.array_equal(c.comparable, [[64, 63, 32], [16, 16, 0]])
    assert np.array_equal(c.mean_abs(), [[1.0, 3.0 / 63.0, 0.0], [0.5, 0.0, np.nan]], equal_nan=True)
    assert np.array_equal(c.rms(), [[2.0, math.sqrt(9.0 / 63.0), 0.0], [1.0, 0.0, np.nan]], equal_nan=True)
    assert np.array_equal(c.steady(1e-3), [[False, False, True], [True, True, False]]) and c.steady(1e-3).dtype == np.bool_
    assert np.array_equal(c.steady(0.0), [[False, False, True], [False, True, False]])
    assert np.array_equal(c.steady(3.0), [[True, False, True], [True, True, False]])     # a non-finite cell is never steady
    one = c.at(0, 1)
    assert isinstance(one, Change) and one == Change(3.0, 9.0, 3.0, 1, 1, 64) and one.comparable == 63
    assert c.at(1, 2).cells == 8 and math.isnan(c.at(1, 2).mean_abs)
    rec["sum_abs"][0, 0] = -1.0                                            # the object holds copies
    assert c.sum_abs[0, 0] == 64.0


def test_simulate_flags():
    from grayscott_amd import simulate

    a = simulate.parse(["--hip-regions", "16x32", "--hip-region-change"])
    assert a.hip_regions == (16, 32) and a.hip_region_change is True and a.hip_region_steady_tol is None
    a = simulate.parse(["--hip-regions", "16", "--hip-region-change", "--hip-region-steady-tol", "1e-3"])
    assert a.hip_region_change is True and a.hip_region_steady_tol == 1e-3
    assert simulate.parse(["--hip-regions", "16", "--hip-region-change", "--hip-region-steady-tol", "0"]).hip_region_steady_tol == 0.0
    plain = simulate.parse(["--hip-regions", "16"])
    assert plain.hip_region_change is False and plain.hip_region_steady_tol is None and simulate.parse([]).hip_region_change is False
    base = ["--hip-regions", "16", "--hip-region-change", "--hip-region-steady-tol"]
    for wrong in (["--hip-region-change"], ["--hip-regions", "16", "--hip-region-steady-tol", "1e-3"], ["--hip-region-steady-tol", "1e-3"],
                  base + ["-1"], base + ["-1e-9"], base + ["nan"], base + ["inf"], base + ["x"], base):
        with pytest.raises(SystemExit):
            simulate.parse(wrong)
    log = simulate.RegionLog((16, 32), [0.25], None, None, None)           # the five-argument constructor: no change
    assert log.change is False and log.steady_tol is None and log.snapshot is None
    log = simulate.RegionLog((16, 32), [0.25], None, change=True, steady_tol=1e-3)
    assert log.change is True and log.steady_tol == 1e-3
    with pytest.raises(ValueError):
        simulate.RegionLog((16, 32), [0.25], None, steady_tol=1e-3)


def test_region_change_kernels_resources(built):
    """Both routes of the comparison kernel, narrow and wide, and the fold: no scratch, no spills, no dynamic stack, no LDS;
    hipcc's default float mode (f32 sub-normals kept); the whole-grid kernels and the regions' summary are still there."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import codeobj
    finally:
        sys.path.pop(0)
    all_kernels = codeobj.kernels(disassemble=False)
    ks = {k.name.split("(")[0]: k for k in all_kernels if k.name.startswith("gs_region_change_")}
    assert sorted(ks) == ["gs_region_change_fold_k", "gs_region_change_k<false, false>", "gs_region_change_k<false, true>",
                          "gs_region_change_k<true, false>", "gs_region_change_k<true, true>"], sorted(ks)
    for name, k in ks.items():
        assert (k.scratch, k.vgpr_spill, k.sgpr_spill, k.dynamic_stack, k.lds) == (0, 0, 0, False, 0), name
        assert k.vgpr <= 128 and k.agpr == 0, (name, k.vgpr)               # four waves a SIMD at the least
        assert k.denorm_mode_32 == 3, (name, k.denorm_mode_32)
    for old in ("gs_row_change_k<", "gs_change_fold_k", "gs_region_summary_k<"):
        assert [k for k in all_kernels if k.name.startswith(old)], old


def test_cpp_region_change_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("region_change_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_region_change_mirror.py)
        r = run_program([str(exe), "64", "128", "16", "32", "5", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
