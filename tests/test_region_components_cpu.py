"""Regional connected components (gs_fields_region_components) without a GPU: the definition (tests/region_components_ref.py)
and its three invariants against the whole-grid restatement, the refusals that need no handle in the header's order through
the built library, the exports, the derived arrays of ``RegionComponents``, the driver's flag, the kernels' resources and the
C++ mirror."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import components_ref, morph_ref, observe_cases, region_components_ref, regions_ref
from tests.children import ROOT, build_program, run_program

HEADER = os.path.join(ROOT, "include", "gs_hip.h")


# ---- the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape,region", [((37, 90), (5, 20)), ((16, 64), (16, 16)), ((23, 50), (7, 16)), ((9, 40), (64, 1024))])
def test_the_reference_keeps_the_invariants_on_random_planes(shape, region, connectivity):
    for seed, density, above in ((1, 0.3, True), (2, 0.593, False), (3, 0.95, True)):
        a = morph_ref.planted(shape, 0.25, seed, density, above)
        got = region_components_ref.invariants(a, region, 0.25, above, connectivity)
        assert got.shape == regions_ref.grid(shape, region) + (35,) and got.dtype == np.uint64
        for (i, j), crop in regions_ref.crops(a, region):
            assert np.array_equal(got[i, j], components_ref.counters(crop, 0.25, above, connectivity)), (i, j)
        # set cells are morphology's, region by region
        set_cells = morph_ref.set_cells(a, 0.25, above)
        for (i, j), crop in regions_ref.crops(set_cells.astype(np.float32), region):
            assert int(got[i, j, 1]) == int(crop.sum()), (i, j)


def test_a_full_plane_is_one_component_per_region():
    shape, region = (37, 90), (5, 20)
    a = observe_cases.plane("full", shape, 0.25, True, 1)
    for connectivity in (4, 8):
        got = region_components_ref.invariants(a, region, 0.25, True, connectivity)
        sizes = regions_ref.sizes(shape, region).astype(np.uint64)
        assert np.array_equal(got[..., 0], np.ones_like(sizes))
        assert np.array_equal(got[..., 1], sizes) and np.array_equal(got[..., 2], sizes)
        assert int(components_ref.counters(a, 0.25, True, connectivity)[0]) == 1   # the whole grid: one, not 8 x 5


def test_a_checkerboard_leaks_through_no_corner():
    """Under 8-connectivity a checkerboard is one component; every region holds one of its own."""
    shape, region = (12, 48), (4, 16)
    a = observe_cases.plane("checkerboard", shape, 0.25, True, 1, special=False)
    got = region_components_ref.invariants(a, region, 0.25, True, 8)
    assert np.array_equal(got[..., 0], np.ones((3, 3), np.uint64)) and np.array_equal(got[..., 1], np.full((3, 3), 32, np.uint64))
    assert np.array_equal(region_components_ref.counters(a, region, 0.25, True, 4)[..., 0], np.full((3, 3), 32, np.uint64))


# ---- refusals that need no handle, in the header's order -----------------------------------------------------------------------
def _f32(*values):
    return (ctypes.c_float * len(values))(*values)


def test_refusals_decided_before_any_handle_is_looked_at_in_order(built):
    from grayscott_amd import capi

    lib = capi.load()
    INV = capi.GS_ERR_INVALID
    F = lib.gs_fields_region_components
    bogus = ctypes.c_void_p(0x10)                                         # never dereferenced: every call is refused first
    fields = (ctypes.c_void_p * 4)(None, None, None, None)
    out = (capi.GsComponents * 16)()
    t, nan = _f32(*([0.25] * 16)), _f32(0.25, math.nan, *([0.25] * 14))
    above = (ctypes.c_int32 * 4)(1, 1, 1, 1)
    err = lambda: lib.gs_last_error().decode()  # noqa: E731

    assert F(None, fields, 1, 4, 16, t, above, 1, 8, out) == INV and "null" in err()
    assert F(bogus, None, 1, 4, 16, t, above, 1, 8, out) == INV and "null" in err()
    assert F(bogus, fields, 1, 4, 16, None, above, 1, 8, out) == INV and "null" in err()
    assert F(bogus, fields, 1, 4, 16, t, None, 1, 8, out) == INV and "null" in err()
    assert F(bogus, fields, 1, 4, 16, t, above, 1, 8, None) == INV and "null" in err()
    assert F(None, fields, 1, 0, 18, nan, above, 0, 5, out) == INV and "null" in err()           # null before everything
    for rh, rw in ((0, 16), (4, 0), (4, 8), (4, 18), (-1, 16), (4, -16)):
        assert F(bogus, fields, 1, rh, rw, t, above, 1, 8, out) == INV and "region" in err(), (rh, rw)
        assert F(bogus, fields, 2, rh, rw, nan, above, 0, 5, out) == INV and "region" in err(), (rh, rw)   # the region shape first
    for nt in (0, 5, -1):
        assert F(bogus, fields, 1, 4, 16, t, above, nt, 8, out) == INV and "thresholds (1..4)" in err(), nt
        assert F(bogus, fields, 2, 4, 16, nan, above, nt, 5, out) == INV and "thresholds (1..4)" in err(), nt  # nt before NaN
        assert F(bogus, fields, 0, 4, 16, t, above, nt, 8, out) == INV and "thresholds (1..4)" in err(), nt    # and before n
    assert F(bogus, fields, 1, 4, 16, nan, above, 2, 5, out) == INV and "NaN" in err()           # NaN before the connectivity
    assert F(bogus, fields, 2, 4, 16, nan, above, 1, 8, out) == INV and "NaN" in err()
    assert F(bogus, fields, 1, 4, 16, nan, above, 1, 8, out) == INV and "field 0" in err()       # field 1's is not read: n = 1
    for connectivity in (0, 5, 6, -8, 16):
        assert F(bogus, fields, 1, 4, 16, t, above, 1, connectivity, out) == INV and "connectivity" in err(), connectivity
        assert F(bogus, fields, 0, 4, 16, t, above, 1, connectivity, out) == INV and "connectivity" in err(), connectivity
    for n in (0, 5, -1):                                                                         # then the handles
        assert F(bogus, fields, n, 4, 16, nan, above, 1, 8, out) == INV and "fields (1..4)" in err(), n   # (no threshold is read)
    for connectivity in (4, 8):
        assert F(bogus, fields, 4, 4, 16, t, above, 4, connectivity, out) == INV and "field 0" in err(), connectivity


def _prototype(text, name):
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_symbol_is_exported_declared_and_bound(built):
    import grayscott_amd
    from grayscott_amd import capi

    full = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    name = "gs_fields_region_components"
    assert _prototype(text, name) == ["gs_ctx *ctx", "gs_field *const *fields", "int32_t n", "int32_t rh", "int32_t rw",
                                      "const float *thresholds", "const int32_t *above", "int32_t nt", "int32_t connectivity",
                                      "gs_components *out"]
    # the twins' conventions up to the region shape, the whole-grid call's behind it
    assert _prototype(text, name)[:5] == _prototype(text, "gs_fields_region_correlation")[:5]
    assert _prototype(text, name)[5:] == _prototype(text, "gs_fields_components")[3:]
    assert "#define GS_REGION_COMPONENTS_MAX (1u << 20)" in full and capi.GS_REGION_COMPONENTS_MAX == 1 << 20
    assert "out[((p * RR + i) * RC + j) * nt + k]" in full
    assert ("Not done: regions of ensemble members; regions that straddle slabs; regional component lists. */\n"
            "#define GS_REGION_COMPONENTS_MAX") in full
    lib = capi.load()
    i32, vp, P = ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER
    assert name in capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).restype is i32
    assert getattr(lib, name).argtypes == [vp, P(vp), i32, i32, i32, P(ctypes.c_float), P(i32), i32, i32, P(capi.GsComponents)]
    assert ctypes.sizeof(capi.GsComponents) == 280
    assert lib.gs_abi_version() == 4 and re.search(r"#define\s+GS_ABI_VERSION\s+4\b", full)
    hpp = open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    assert "using RegionComponents = Regions<Components>;" in hpp and "gs_fields_region_components(context_->get()" in hpp
    assert "RegionComponents" in grayscott_amd.__all__ and hasattr(grayscott_amd.simulation, "region_components_fields")
    assert hasattr(grayscott_amd.HipConcentration, "region_components") and hasattr(grayscott_amd.Species, "region_components")


def test_region_components_kernels_resources(built):
    """The region forms of the tile kernel, the border kernel and the tally: no scratch, no spills, no dynamic stack, the
    tile kernel's 16 KiB of LDS; the whole-grid kernels are still there."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import codeobj
    finally:
        sys.path.pop(0)
    all_kernels = codeobj.kernels(disassemble=False)
    ks = {k.name: k for k in all_kernels if k.name.startswith("gs_region_comp_")}
    assert sorted(n.split("(")[0] for n in ks) == ["gs_region_comp_border_k", "gs_region_comp_tally_k", "gs_region_comp_tile_k"], sorted(ks)
    for name, k in ks.items():
        assert (k.scratch, k.vgpr_spill, k.sgpr_spill, k.dynamic_stack) == (0, 0, 0, False), name
        assert k.vgpr <= 64, (name, k.vgpr)                                # eight waves a SIMD
        assert k.lds == (16384 if "tile" in name else 144 if "tally" in name else 0), (name, k.lds)
    for old in ("gs_comp_tile_k<", "gs_comp_border_k", "gs_comp_flatten_k", "gs_comp_tally_k", "gs_comp_seam_k"):
        assert [k for k in all_kernels if k.name.startswith(old)], old


# ---- the Python result ---------------------------------------------------------------------------------------------------------
def test_region_components_object_is_components_on_the_crops():
    from grayscott_amd import Components, Morphology, RegionComponents, RegionMorphology

    shape, region, t = (23, 50), (9, 16), 0.25
    a = morph_ref.planted(shape, t, 3, 0.5, True)
    a[0:9, 0:16] = np.float32(0.0)                                         # a region with no set cell
    a[9:18, 16:32] = np.float32(1.0)                                       # a full one
    a[11:13, 20:22] = np.float32(0.0)                                      # with one hole
    for connectivity in (4, 8):
        counters = region_components_ref.counters(a, region, t, True, connectivity)
        c = RegionComponents.from_counters(counters, t, True, connectivity, region, shape)
        assert c.count.shape == c.set_cells.shape == c.largest.shape == (3, 4) and c.by_size.shape == (3, 4, 32)
        assert c.count.dtype == c.set_cells.dtype == c.largest.dtype == c.by_size.dtype == np.uint64
        assert (c.threshold, c.above, c.connectivity, c.region, c.shape) == (t, True, connectivity, region, shape)
        assert np.array_equal(c.counters(), counters)
        m = RegionMorphology.from_quads(regions_ref.quads(a, region, t, True), t, True, region, shape)
        mean, share, holes = c.mean_size(), c.largest_fraction(), c.holes(m)
        assert mean.shape == share.shape == holes.shape == (3, 4) and mean.dtype == share.dtype == np.float64
        for (i, j), crop in regions_ref.crops(a, region):
            one = Components.from_counters(components_ref.counters(crop, t, True, connectivity), t, True, connectivity)
            got = c.at(i, j)
            assert (got.count, got.set_cells, got.largest) == (one.count, one.set_cells, one.largest), (i, j)
            assert np.array_equal(got.by_size, one.by_size) and (got.threshold, got.above, got.connectivity) == (t, True, connectivity)
            assert np.array_equal(mean[i, j], one.mean_size, equal_nan=True) and np.array_equal(share[i, j], one.largest_fraction, equal_nan=True)
            assert int(holes[i, j]) == one.holes(Morphology.from_quads(morph_ref.quads(crop, t, True), t, True, crop.size)), (i, j)
        assert c.count[0, 0] == 0 and math.isnan(mean[0, 0]) and math.isnan(share[0, 0]) and holes[0, 0] == 0
        assert c.count[1, 1] == 1 and share[1, 1] == 1.0 and holes[1, 1] == 1 and mean[1, 1] == 9 * 16 - 4
        for wrong in (RegionMorphology.from_quads(regions_ref.quads(a, region, 0.5, True), 0.5, True, region, shape),
                      RegionMorphology.from_quads(regions_ref.quads(a, region, t, False), t, False, region, shape),
                      RegionMorphology.from_quads(regions_ref.quads(a, (9, 32), t, True), t, True, (9, 32), shape)):
            with pytest.raises(ValueError):
                c.holes(wrong)


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_simulate_flags():
    from grayscott_amd import simulate

    a = simulate.parse(["--hip-regions", "16x32", "--hip-region-components"])
    assert a.hip_regions == (16, 32) and a.hip_region_components == 8
    assert simulate.parse(["--hip-regions", "16", "--hip-region-components", "4"]).hip_region_components == 4
    assert simulate.parse(["--hip-regions", "16", "--hip-region-components", "8", "-o", "x.h5"]).hip_region_components == 8
    assert simulate.parse(["--hip-regions", "16", "--hip-region-components", "-o", "x.h5"]).hip_region_components == 8
    assert simulate.parse(["--hip-regions", "16"]).hip_region_components is None and simulate.parse([]).hip_region_components is None
    base = ["--hip-regions", "16", "--hip-region-components"]
    for wrong in (["--hip-region-components"], ["--hip-region-components", "4"], base + ["6"], base + ["0"], base + ["a"], base + ["8.0"]):
        with pytest.raises(SystemExit):
            simulate.parse(wrong)
    log = simulate.RegionLog((16, 32), [0.25], None, None, None)           # the five-argument constructor: no components
    assert log.components is None
    assert simulate.RegionLog((16, 32), [0.25], None, None, None, 4).components == 4
    assert simulate.RegionLog((16, 32), [0.25], None, components=8).components == 8


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def test_cpp_region_components_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("region_components_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_region_components_mirror.py)
        r = run_program([str(exe), "64", "128", "16", "32", "5", "8", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
