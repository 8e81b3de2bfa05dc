"""Regional two-point correlations (gs_fields_region_correlation) without a GPU: the definition (tests/region_corr_ref.py)
against the literal whole-grid rule on small crops, the refusals that need no handle in the header's order through the built
library, the exports, the derived arrays of ``RegionCorrelation``, the stripe plane whose whole-grid wavelength belongs to
no region, the driver's flag, and the C++ mirror."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import corr_ref, region_corr_ref, regions_ref
from tests.children import ROOT, build_program, run_program

HEADER = os.path.join(ROOT, "include", "gs_hip.h")


def odd_plane(shape, seed):
    rng = np.random.default_rng(seed)
    a = (rng.random(shape, dtype=np.float32) - np.float32(0.3)).astype(np.float32)
    odd = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-40, 3.4028235e38], np.float32)
    a.flat[rng.choice(a.size, size=len(odd), replace=False)] = odd
    return a


# ---- the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,region", [((5, 40), (2, 16)), ((3, 21), (3, 16)), ((4, 33), (1, 32)), ((6, 20), (4, 16))])
def test_the_reference_is_the_literal_rule_on_every_crop(shape, region):
    a = odd_plane(shape, shape[1])
    L = 6
    for above in (True, False):
        got = region_corr_ref.pairs(a, region, 0.1, above, L)
        assert got.shape == regions_ref.grid(shape, region) + (4, L + 1) and got.dtype == np.uint64
        assert np.array_equal(got, region_corr_ref.pairs_by_label(a, region, 0.1, above, L))
        for (i, j), crop in regions_ref.crops(a, region):
            assert np.array_equal(got[i, j], corr_ref.literal(crop, 0.1, above, L)), (i, j, above)
            assert (got[i, j] <= corr_ref.totals(crop.shape[0], crop.shape[1], L).astype(np.uint64)).all()
    # an all-set plane: every pair that exists inside a region and none across a border; the areas partition the cells
    full = region_corr_ref.pairs(np.ones(shape, np.float32), region, 0.5, True, L)
    assert np.array_equal(full.astype(np.int64), region_corr_ref.totals(shape, region, L))
    assert int(full[:, :, 0, 0].sum()) == shape[0] * shape[1]
    assert (full[:, :, :, 0] == full[:, :, :1, 0]).all()                   # d = 0 is the area for all four directions


# ---- refusals that need no handle, in the header's order -----------------------------------------------------------------------
def _f32(*values):
    return (ctypes.c_float * len(values))(*values)


def test_refusals_decided_before_any_handle_is_looked_at_in_order(built):
    from grayscott_amd import capi

    lib = capi.load()
    INV = capi.GS_ERR_INVALID
    F = lib.gs_fields_region_correlation
    bogus = ctypes.c_void_p(0x10)                                         # never dereferenced: every call is refused first
    fields = (ctypes.c_void_p * 4)(None, None, None, None)
    out = (ctypes.c_uint64 * (4 * 4 * 65))()
    thr, sense = _f32(*([0.5] * 16)), (ctypes.c_int32 * 4)(1, 0, 1, 0)
    nan = _f32(0.1, math.nan, 0.3, 0.4)
    err = lambda: lib.gs_last_error().decode()  # noqa: E731

    assert F(None, fields, 1, 4, 16, thr, sense, 1, 8, out) == INV and "null" in err()
    assert F(bogus, None, 1, 4, 16, thr, sense, 1, 8, out) == INV and "null" in err()
    assert F(bogus, fields, 1, 4, 16, None, sense, 1, 8, out) == INV and "null" in err()
    assert F(bogus, fields, 1, 4, 16, thr, None, 1, 8, out) == INV and "null" in err()
    assert F(bogus, fields, 1, 4, 16, thr, sense, 1, 8, None) == INV and "null" in err()
    assert F(None, fields, 1, 0, 18, nan, sense, 0, 0, out) == INV and "null" in err()          # null before everything
    for rh, rw in ((0, 16), (4, 0), (4, 8), (4, 18), (-1, 16), (4, -16)):
        assert F(bogus, fields, 1, rh, rw, thr, sense, 1, 8, out) == INV and "region" in err(), (rh, rw)
        assert F(bogus, fields, 1, rh, rw, nan, sense, 0, 0, out) == INV and "region" in err(), (rh, rw)   # the region shape first
    for nt in (0, 5, -1, 1 << 20):
        assert F(bogus, fields, 1, 4, 16, thr, sense, nt, 8, out) == INV and "thresholds (1..4)" in err(), nt
        assert F(bogus, fields, 1, 4, 16, nan, sense, nt, 0, out) == INV and "thresholds (1..4)" in err(), nt  # nt before NaN, lag
    assert F(bogus, fields, 1, 4, 16, nan, sense, 2, 0, out) == INV and "NaN" in err()                     # NaN before the lag
    assert F(bogus, fields, 2, 4, 16, _f32(0.1, 0.2, 0.3, math.nan), sense, 2, 8, out) == INV and "threshold 1 of plane 1" in err()
    for lag in (0, -1, 65, 1 << 20):
        assert F(bogus, fields, 1, 4, 16, thr, sense, 1, lag, out) == INV and "(1..64)" in err(), lag
        assert F(bogus, fields, 0, 4, 16, thr, sense, 1, lag, out) == INV and "(1..64)" in err(), lag      # the lag before n
    for n in (0, 5, -1):                                                                                   # then the handles
        assert F(bogus, fields, n, 4, 16, thr, sense, 1, 8, out) == INV and "fields (1..4)" in err(), n
    for lag in (1, 64):
        assert F(bogus, fields, 4, 4, 16, thr, sense, 4, lag, out) == INV and "field 0" in err(), lag
    assert F(bogus, fields, 2, 1, 16, _f32(math.inf, -math.inf), sense, 1, 8, out) == INV and "field 0" in err()


def _prototype(text, name):
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_symbol_is_exported_declared_and_bound(built):
    import grayscott_amd
    from grayscott_amd import capi

    full = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    name = "gs_fields_region_correlation"
    assert _prototype(text, name) == ["gs_ctx *ctx", "gs_field *const *fields", "int32_t n", "int32_t rh", "int32_t rw",
                                      "const float *thresholds", "const int32_t *above", "int32_t nt", "int32_t max_lag",
                                      "uint64_t *out"]
    # the morphology twin's conventions, with the lag and plain counters in place of gs_morphology
    assert _prototype(text, name)[:8] == _prototype(text, "gs_fields_region_morphology")[:8]
    assert "#define GS_REGION_PAIRS_MAX (1u << 25)" in full and capi.GS_REGION_PAIRS_MAX == 1 << 25
    assert "out[((((p * RR + i) * RC + j) * nt + t) * 4 + k) * (L + 1) + d]" in full
    lib = capi.load()
    i32, u64, vp, P = ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER
    assert name in capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).restype is i32
    assert getattr(lib, name).argtypes == [vp, P(vp), i32, i32, i32, P(ctypes.c_float), P(i32), i32, i32, P(u64)]
    assert lib.gs_abi_version() == 4
    ffi = open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    assert f"pub fn {name}(" in ffi
    hpp = open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    assert "gs_fields_region_correlation(context_->get(), planes, 2, rh, rw, t.data(), sense, (int32_t)nt, max_lag, out.data())" in hpp
    assert "RegionCorrelation" in grayscott_amd.__all__
    assert hasattr(grayscott_amd.HipConcentration, "region_correlation") and hasattr(grayscott_amd.Species, "region_correlation")


def test_region_pair_kernels_resources(built):
    """Every gs_region_pairs_k instance: no scratch, no spills, no LDS -- a unit flushes straight to the region's counters."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import codeobj
    finally:
        sys.path.pop(0)
    ks = [k for k in codeobj.kernels(disassemble=False) if k.name.startswith("gs_region_pairs_k<")]
    assert len(ks) == 12, [k.name for k in ks]                             # nt 1..4 x (four words and halo, four words, one word)
    for k in ks:
        assert (k.scratch, k.vgpr_spill, k.sgpr_spill, k.lds, k.dynamic_stack) == (0, 0, 0, 0, False), k.name


# ---- the Python result ---------------------------------------------------------------------------------------------------------
def test_region_correlation_object_is_correlation_on_the_crops():
    from grayscott_amd import Correlation, RegionCorrelation

    shape, region, L = (23, 50), (9, 16), 12
    a = odd_plane(shape, 3)
    a[0:9, 0:16] = np.float32(-1.0)                                        # a region with nothing set
    pairs = region_corr_ref.pairs(a, region, 0.1, True, L)
    c = RegionCorrelation.from_pairs(pairs, 0.1, True, region, shape)
    assert c.pairs.shape == (3, 4, 4, L + 1) and c.pairs.dtype == np.uint64 and c.region == region and c.shape == shape
    assert c.threshold == 0.1 and c.above is True and c.max_lag == L
    assert np.array_equal(c.cells, regions_ref.sizes(shape, region))
    assert np.array_equal(c.totals(), region_corr_ref.totals(shape, region, L)) and c.totals().dtype == np.int64
    for k in range(4):
        s2, cov, fmin, fmax = c.s2(k), c.autocovariance(k), c.first_minimum(k), c.first_maximum_after_minimum(k)
        assert s2.shape == cov.shape == (3, 4, L + 1) and fmin.shape == fmax.shape == (3, 4) and fmin.dtype == fmax.dtype == np.int64
        for (i, j), crop in regions_ref.crops(a, region):
            one = Correlation.from_pairs(corr_ref.pairs(crop, 0.1, True, L), 0.1, True, crop.shape[0], crop.shape[1])
            got = c.at(i, j)
            assert np.array_equal(got.pairs, one.pairs) and (got.rows, got.cols) == (one.rows, one.cols) == crop.shape
            assert (got.threshold, got.above) == (one.threshold, one.above)
            assert np.array_equal(s2[i, j], one.s2(k), equal_nan=True) and np.array_equal(cov[i, j], one.autocovariance(k), equal_nan=True)
            assert fmin[i, j] == (-1 if one.first_minimum(k) is None else one.first_minimum(k)), (i, j, k)
            assert fmax[i, j] == (-1 if one.first_maximum_after_minimum(k) is None else one.first_maximum_after_minimum(k)), (i, j, k)
    assert c.first_minimum(0)[0, 0] == -1 and c.pairs[0, 0].sum() == 0


def test_stripe_plane_has_a_wavelength_per_region_and_a_blend_for_the_whole_grid():
    from grayscott_amd import Correlation, RegionCorrelation

    a = region_corr_ref.stripe_thirds((96, 192), (8, 12, 16))
    L, region = 24, (32, 64)
    whole = Correlation.from_pairs(corr_ref.pairs(a, 0.5, True, L), 0.5, True, 96, 192)
    assert whole.first_maximum_after_minimum(0) == 10                       # a blend that belongs to no region
    c = RegionCorrelation.from_pairs(region_corr_ref.pairs(a, region, 0.5, True, L), 0.5, True, region, a.shape)
    assert c.first_maximum_after_minimum(0).tolist() == [[8, 12, 16]] * 3
    assert c.first_minimum(0).tolist() == [[4, 6, 8]] * 3


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_simulate_flag():
    from grayscott_amd import simulate

    a = simulate.parse(["--hip-regions", "16x32", "--hip-region-corr-lags", "8"])
    assert a.hip_regions == (16, 32) and a.hip_region_corr_lags == 8
    assert simulate.parse(["--hip-regions", "16", "--hip-region-corr-lags", "64"]).hip_region_corr_lags == 64
    assert simulate.parse(["--hip-regions", "16"]).hip_region_corr_lags is None and simulate.parse([]).hip_region_corr_lags is None
    for wrong in (["--hip-region-corr-lags", "8"], ["--hip-regions", "16", "--hip-region-corr-lags", "0"],
                  ["--hip-regions", "16", "--hip-region-corr-lags", "65"], ["--hip-regions", "16", "--hip-region-corr-lags", "-3"],
                  ["--hip-regions", "16", "--hip-region-corr-lags", "a"], ["--hip-regions", "16", "--hip-region-corr-lags", "8.5"]):
        with pytest.raises(SystemExit):
            simulate.parse(wrong)
    log = simulate.RegionLog((16, 32), [0.25], None)                       # the three-argument constructor: no correlations
    assert log.corr_lags is None
    assert simulate.RegionLog((16, 32), [0.25], None, 8).corr_lags == 8


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def test_cpp_region_correlation_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("region_correlation_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_region_correlation_mirror.py)
        r = run_program([str(exe), "64", "128", "16", "32", "5", "8", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
