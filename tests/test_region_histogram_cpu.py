"""Regional histograms (gs_fields_region_histogram) without a GPU: the definition (tests/region_hist_ref.py) against the
literal whole-grid rule on small crops, the refusals that need no handle in the header's order through the built library, the
exports, the derived arrays of ``RegionHistogram``, the driver's flags, the kernels' resources and the C++ mirror."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import hist_ref, region_hist_ref, regions_ref
from tests.children import ROOT, build_program, run_program

HEADER = os.path.join(ROOT, "include", "gs_hip.h")


# ---- the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,region", [((5, 40), (2, 16)), ((3, 21), (3, 16)), ((2, 260), (2, 256))])
def test_the_reference_is_the_literal_rule_on_every_crop(shape, region):
    for lo, hi, bins in ((0.0, 1.0, 7), (-0.25, 0.5, 1), (1e-3, 2e-3, 64)):
        a = hist_ref.planted(shape, lo, hi, bins, shape[1] + bins)
        got = region_hist_ref.histograms(a, region, lo, hi, bins)
        assert got.shape == regions_ref.grid(shape, region) + (bins + 3,) and got.dtype == np.uint64
        assert np.array_equal(got, region_hist_ref.by_label(a, region, lo, hi, bins))
        for (i, j), crop in regions_ref.crops(a, region):
            assert np.array_equal(got[i, j], hist_ref.literal(crop, lo, hi, bins)), (i, j, bins)
        # a region's counters sum to its cells; over the regions every slot sums to the whole grid's
        assert np.array_equal(got.sum(axis=2).astype(np.int64), regions_ref.sizes(shape, region))
        assert np.array_equal(got.sum(axis=(0, 1)), hist_ref.histogram(a, lo, hi, bins))


def test_by_label_is_the_definition_on_larger_planes():
    a = hist_ref.planted((96, 301), 0.0, 1.0, 256, 5)
    for region in ((32, 64), (7, 20), (100, 320), (1, 16)):
        assert np.array_equal(region_hist_ref.by_label(a, region, 0.0, 1.0, 256), region_hist_ref.histograms(a, region, 0.0, 1.0, 256))
    assert region_hist_ref.by_label(np.zeros((0, 40), np.float32), (2, 16), 0.0, 1.0, 8).shape == (0, 3, 11)


# ---- refusals that need no handle, in the header's order -----------------------------------------------------------------------
def _f32(*values):
    return (ctypes.c_float * len(values))(*values)


def test_refusals_decided_before_any_handle_is_looked_at_in_order(built):
    from grayscott_amd import capi

    lib = capi.load()
    INV = capi.GS_ERR_INVALID
    F = lib.gs_fields_region_histogram
    bogus = ctypes.c_void_p(0x10)                                         # never dereferenced: every call is refused first
    fields = (ctypes.c_void_p * 4)(None, None, None, None)
    out = (ctypes.c_uint64 * (4 * 4099))()
    lo, hi = _f32(0.0, 0.0, 0.0, 0.0), _f32(1.0, 1.0, 1.0, 1.0)
    nan = _f32(0.0, math.nan, 0.0, 0.0)
    err = lambda: lib.gs_last_error().decode()  # noqa: E731

    assert F(None, fields, 1, 4, 16, lo, hi, 8, out) == INV and "null" in err()
    assert F(bogus, None, 1, 4, 16, lo, hi, 8, out) == INV and "null" in err()
    assert F(bogus, fields, 1, 4, 16, None, hi, 8, out) == INV and "null" in err()
    assert F(bogus, fields, 1, 4, 16, lo, None, 8, out) == INV and "null" in err()
    assert F(bogus, fields, 1, 4, 16, lo, hi, 8, None) == INV and "null" in err()
    assert F(None, fields, 1, 0, 18, nan, nan, 0, out) == INV and "null" in err()              # null before everything
    for rh, rw in ((0, 16), (4, 0), (4, 8), (4, 18), (-1, 16), (4, -16)):
        assert F(bogus, fields, 1, rh, rw, lo, hi, 8, out) == INV and "region" in err(), (rh, rw)
        assert F(bogus, fields, 2, rh, rw, nan, hi, 0, out) == INV and "region" in err(), (rh, rw)   # the region shape first
    for bins in (0, -1, 4097, 1 << 20):
        assert F(bogus, fields, 1, 4, 16, lo, hi, bins, out) == INV and "bins (1..4096)" in err(), bins
        assert F(bogus, fields, 2, 4, 16, nan, hi, bins, out) == INV and "bins (1..4096)" in err(), bins  # bins before the ranges
        assert F(bogus, fields, 0, 4, 16, lo, hi, bins, out) == INV and "bins (1..4096)" in err(), bins   # and before n
    # the ranges of fields 0 .. n - 1: NaN, infinite, lo >= hi, a width or scale that is no normal positive f32
    assert F(bogus, fields, 2, 4, 16, nan, hi, 8, out) == INV and "range 1" in err()
    assert F(bogus, fields, 2, 4, 16, lo, _f32(1.0, math.nan), 8, out) == INV and "range 1" in err()
    assert F(bogus, fields, 1, 4, 16, nan, hi, 8, out) == INV and "field 0" in err()            # field 1's range is not read: n = 1
    assert F(bogus, fields, 1, 4, 16, _f32(-math.inf), hi, 8, out) == INV and "range 0" in err()
    assert F(bogus, fields, 1, 4, 16, lo, _f32(math.inf), 8, out) == INV and "range 0" in err()
    assert F(bogus, fields, 1, 4, 16, _f32(1.0), _f32(1.0), 8, out) == INV and "range 0" in err()
    assert F(bogus, fields, 1, 4, 16, _f32(2.0), _f32(1.0), 8, out) == INV and "range 0" in err()
    assert F(bogus, fields, 3, 4, 16, _f32(0.0, 0.0, 0.5), _f32(1.0, 1.0, 0.25), 8, out) == INV and "range 2" in err()
    assert F(bogus, fields, 1, 4, 16, _f32(-3e38), _f32(3e38), 8, out) == INV and "normal positive" in err()      # the width is inf
    assert F(bogus, fields, 1, 4, 16, _f32(0.0), _f32(1e-45), 4096, out) == INV and "normal positive" in err()    # sub-normal width
    assert F(bogus, fields, 1, 4, 16, _f32(0.0), _f32(2e-38), 4096, out) == INV and "normal positive" in err()    # the scale is inf
    for n in (0, 5, -1):                                                                        # then the handles
        assert F(bogus, fields, n, 4, 16, nan, nan, 8, out) == INV and "fields (1..4)" in err(), n   # (no range is read)
    for bins in (1, 4096):
        assert F(bogus, fields, 4, 4, 16, lo, hi, bins, out) == INV and "field 0" in err(), bins


def _prototype(text, name):
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_symbol_is_exported_declared_and_bound(built):
    import grayscott_amd
    from grayscott_amd import capi

    full = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    name = "gs_fields_region_histogram"
    assert _prototype(text, name) == ["gs_ctx *ctx", "gs_field *const *fields", "int32_t n", "int32_t rh", "int32_t rw",
                                      "const float *lo", "const float *hi", "int32_t bins", "uint64_t *out"]
    # the twins' conventions up to the region shape, the whole-grid histogram's behind it
    assert _prototype(text, name)[:5] == _prototype(text, "gs_fields_region_correlation")[:5]
    assert _prototype(text, name)[5:] == _prototype(text, "gs_fields_histogram")[3:]
    assert "#define GS_REGION_HIST_MAX (1u << 25)" in full and capi.GS_REGION_HIST_MAX == 1 << 25
    assert "out[((p * RR + i) * RC + j) * (bins + 3) + s]" in full
    assert "Not done: regions of ensemble members; regions that straddle slabs. */\n#define GS_REGION_HIST_MAX" in full
    lib = capi.load()
    i32, u64, vp, P = ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER
    assert name in capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).restype is i32
    assert getattr(lib, name).argtypes == [vp, P(vp), i32, i32, i32, P(ctypes.c_float), P(ctypes.c_float), i32, P(u64)]
    assert lib.gs_abi_version() == 4 and re.search(r"#define\s+GS_ABI_VERSION\s+4\b", full)
    ffi = open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    assert f"pub fn {name}(" in ffi and "pub const GS_REGION_HIST_MAX: u64 = 1 << 25;" in ffi
    hpp = open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    assert "gs_fields_region_histogram(context_->get(), planes, 2, rh, rw, lo, hi, bins, out.data())" in hpp
    assert "RegionHistogram" in grayscott_amd.__all__
    assert hasattr(grayscott_amd.HipConcentration, "region_histogram") and hasattr(grayscott_amd.Species, "region_histogram")


def test_region_hist_kernels_resources(built):
    """Both gs_region_hist_k forms: no scratch, no spills, dynamic LDS alone; the whole-grid kernel is still there in both forms."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import codeobj
    finally:
        sys.path.pop(0)
    all_kernels = codeobj.kernels(disassemble=False)
    ks = [k for k in all_kernels if k.name.startswith("gs_region_hist_k<")]
    assert len(ks) == 2, [k.name for k in ks]
    for k in ks:
        assert (k.scratch, k.vgpr_spill, k.sgpr_spill, k.lds, k.dynamic_stack) == (0, 0, 0, 0, False), k.name
        assert k.vgpr <= 128, (k.name, k.vgpr)                             # two workgroups of 4 waves a CU and more
    assert len([k for k in all_kernels if k.name.startswith("gs_plane_hist_k<")]) == 2


# ---- the Python result ---------------------------------------------------------------------------------------------------------
def test_region_histogram_object_is_histogram_on_the_crops():
    from grayscott_amd import Histogram, RegionHistogram

    shape, region, lo, hi, bins = (23, 50), (9, 16), -0.25, 0.75, 12
    a = hist_ref.planted(shape, lo, hi, bins, 3)
    a[0:9, 0:16] = np.float32(2.0)                                         # a region with no cell in range
    a[9:18, 16:32] = np.float32(np.nan)                                    # and one of NaN alone
    counters = region_hist_ref.histograms(a, region, lo, hi, bins)
    h = RegionHistogram.from_counters(counters, lo, hi, region, shape)
    assert h.counts.shape == (3, 4, bins) and h.counts.dtype == np.uint64 and h.bins == bins
    assert h.below.shape == h.above.shape == h.nan.shape == h.cells.shape == h.in_range.shape == (3, 4)
    assert (h.lo, h.hi, h.region, h.shape) == (lo, hi, region, shape)
    assert np.array_equal(h.cells, regions_ref.sizes(shape, region))
    assert np.array_equal(h.cells, (h.in_range + h.below + h.above + h.nan).astype(np.int64))
    assert np.array_equal(region_hist_ref.counters_of(h), counters)
    assert h.edges().shape == (bins + 1,) and h.edges()[0] == lo and h.edges()[-1] == hi
    xs, qs = (-1.0, lo, 0.0, 0.1, 0.25, float(h.edges()[5]), hi, 2.0), (0.0, 0.01, 0.25, 0.5, 0.9, 1.0)
    above, quant = {x: h.fraction_above(x) for x in xs}, {q: h.quantile(q) for q in qs}
    for (i, j), crop in regions_ref.crops(a, region):
        one = Histogram.from_counters(hist_ref.histogram(crop, lo, hi, bins), lo, hi, crop.size)
        got = h.at(i, j)
        assert np.array_equal(got.counts, one.counts) and (got.below, got.above, got.nan) == (one.below, one.above, one.nan)
        assert (got.lo, got.hi, got.size, got.in_range) == (one.lo, one.hi, one.size, one.in_range) and got.size == crop.size
        assert np.array_equal(got.edges(), h.edges())
        for x in xs:
            assert above[x].shape == (3, 4) and above[x].dtype == np.float64
            assert np.array_equal(above[x][i, j], one.fraction_above(x), equal_nan=True), (i, j, x)
        for q in qs:
            assert quant[q].shape == (3, 4) and quant[q].dtype == np.float64
            assert np.array_equal(quant[q][i, j], one.quantile(q), equal_nan=True), (i, j, q)
    assert h.in_range[0, 0] == 0 and h.above[0, 0] == 9 * 16 and math.isnan(h.fraction_above(0.1)[0, 0]) and math.isnan(h.quantile(0.5)[0, 0])
    assert h.nan[1, 1] == 9 * 16 and math.isnan(h.quantile(0.5)[1, 1]) and math.isnan(h.fraction_above(0.0)[1, 1])
    assert not np.isnan(h.quantile(0.5)[2, 3])
    with pytest.raises(ValueError):
        h.quantile(1.5)


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_simulate_flags():
    from grayscott_amd import simulate

    a = simulate.parse(["--hip-regions", "16x32", "--hip-region-hist-bins", "64"])
    assert a.hip_regions == (16, 32) and a.hip_region_hist_bins == 64
    assert a.hip_region_hist_range_u is None and a.hip_region_hist_range_v is None
    assert simulate.region_hist_args(a) == (64, None, None)
    a = simulate.parse(["--hip-regions", "16", "--hip-region-hist-bins", "4096", "--hip-region-hist-range-u", "0.25:1",
                        "--hip-region-hist-range-v=-0.5:0.5"])                     # (a range that begins with a minus sign: with =)
    assert a.hip_region_hist_bins == 4096 and a.hip_region_hist_range_u == (0.25, 1.0) and a.hip_region_hist_range_v == (-0.5, 0.5)
    assert simulate.parse(["--hip-regions", "16"]).hip_region_hist_bins is None and simulate.parse([]).hip_region_hist_bins is None
    assert simulate.region_hist_args(simulate.parse(["--hip-regions", "16"])) is None
    base = ["--hip-regions", "16", "--hip-region-hist-bins"]
    for wrong in (["--hip-region-hist-bins", "8"], base + ["0"], base + ["4097"], base + ["-3"], base + ["a"], base + ["8.5"],
                  ["--hip-regions", "16", "--hip-region-hist-range-u", "0:1"], ["--hip-regions", "16", "--hip-region-hist-range-v", "0:1"],
                  base + ["8", "--hip-region-hist-range-u", "1:0"], base + ["8", "--hip-region-hist-range-u", "1:1"],
                  base + ["8", "--hip-region-hist-range-v", "0:inf"], base + ["8", "--hip-region-hist-range-v", "nan:1"],
                  base + ["8", "--hip-region-hist-range-v", "0"], base + ["8", "--hip-region-hist-range-v", "0:1:2"],
                  base + ["8", "--hip-region-hist-range-u", "a:b"]):
        with pytest.raises(SystemExit):
            simulate.parse(wrong)
    log = simulate.RegionLog((16, 32), [0.25], None)                       # the three-argument constructor: neither
    assert log.corr_lags is None and log.hist is None
    log = simulate.RegionLog((16, 32), [0.25], None, 8)                    # the four-argument one: no histograms
    assert log.corr_lags == 8 and log.hist is None
    assert simulate.RegionLog((16, 32), [0.25], None, None, (64, None, (0.0, 0.5))).hist == (64, (0.0, 1.0), (0.0, 0.5))


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def test_cpp_region_histogram_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("region_histogram_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_region_histogram_mirror.py)
        r = run_program([str(exe), "64", "128", "16", "32", "5", "64", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
