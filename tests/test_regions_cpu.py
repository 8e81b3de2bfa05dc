"""Regional observables without a GPU: the definition (tests/regions_ref.py) against the literal whole-grid rules on small
crops, gs_region_grid and the refusals that need no handle through the built library, the derived arrays of the Python
results, and the driver's flags and region means."""
import ctypes
import os

import numpy as np
import pytest

from grayscott_amd import Morphology, RegionMorphology, RegionSummaries, Summary, capi, simulate
from grayscott_amd.simulation import quad_measures, region_grid, region_shape, region_sizes
from tests import morph_ref, regions_ref, summary_ref
from tests.children import ROOT, build_program, run_program


def odd_plane(shape, seed):
    rng = np.random.default_rng(seed)
    a = (rng.random(shape, dtype=np.float32) - np.float32(0.3)).astype(np.float32)
    odd = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-40, 3.4028235e38], np.float32)
    a.flat[rng.choice(a.size, size=len(odd), replace=False)] = odd
    return a


# ---- the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,region", [((5, 40), (2, 16)), ((3, 21), (3, 16)), ((4, 33), (1, 32)), ((2, 260), (2, 256))])
def test_the_reference_is_the_literal_rule_on_every_crop(shape, region):
    a = odd_plane(shape, shape[1])
    sums, quads = regions_ref.summaries(a, region), regions_ref.quads(a, region, 0.1, True)
    below = regions_ref.quads(a, region, 0.1, False)
    assert sums.shape == regions_ref.grid(shape, region) and quads.shape == sums.shape + (6,)
    for (i, j), crop in regions_ref.crops(a, region):
        assert crop.shape == (min(region[0], shape[0] - i * region[0]), min(region[1], shape[1] - j * region[1]))
        assert summary_ref.same(sums[i, j], summary_ref.literal(crop)), (i, j)
        assert np.array_equal(quads[i, j], morph_ref.literal(crop, 0.1, True)), (i, j)
        assert np.array_equal(below[i, j], morph_ref.literal(crop, 0.1, False)), (i, j)
        assert int(quads[i, j].sum()) == (crop.shape[0] + 1) * (crop.shape[1] + 1)
    assert np.array_equal(regions_ref.sizes(shape, region), region_sizes(shape[0], shape[1], region, sums.shape))
    # the regions do not partition the global quads, but they do partition the cells
    assert int(sums["nonfinite"].sum()) == int(np.count_nonzero(~np.isfinite(a)))
    assert sum(int(morph_ref.measures(q)["area"]) for q in quads.reshape(-1, 6)) == int(np.count_nonzero(morph_ref.set_cells(a, 0.1, True)))


# ---- gs_region_grid and the refusals that need no handle --------------------------------------------------------------------
def test_region_grid_and_its_limits(built):
    lib = capi.load()
    assert region_grid(5, 40, (2, 16)) == (3, 3) and region_grid(64, 128, 16) == (4, 8) and region_grid(7, 16, (100, 16)) == (1, 1)
    assert region_grid(0, 40, (2, 16)) == (0, 3) and region_grid(5, 0, (2, 16)) == (3, 0)
    assert region_grid(4096, 16384, (1, 16)) == (4096, 1024)             # exactly GS_REGIONS_MAX = 2^22 regions
    assert region_grid(2 ** 40, 2 ** 40, (2 ** 31 - 1, 2 ** 31 - 4)) == (513, 513)
    for rows, cols, region in ((4097, 16384, (1, 16)), (4096, 16385, (1, 16)), (2 ** 63, 2 ** 63, (1, 16)),
                               (5, 40, (0, 16)), (5, 40, (-3, 16)), (5, 40, (2, 0)), (5, 40, (2, 8)), (5, 40, (2, 12)), (5, 40, (2, 18)),
                               (5, 40, (2, -16))):
        with pytest.raises(capi.GsError) as e:
            region_grid(rows, cols, region)
        assert e.value.code == capi.GS_ERR_INVALID, (rows, cols, region)
    rr = ctypes.c_uint64(7)
    assert lib.gs_region_grid(5, 40, 2, 16, None, ctypes.byref(rr)) == capi.GS_ERR_INVALID
    assert lib.gs_region_grid(5, 40, 2, 16, ctypes.byref(rr), None) == capi.GS_ERR_INVALID and rr.value == 7
    assert region_shape(48) == (48, 48) and region_shape((3, 16)) == (3, 16)


def test_refusals_decided_before_any_handle_is_looked_at(built):
    lib = capi.load()
    bogus = ctypes.c_void_p(0x10)                                         # never dereferenced: every call is refused first
    fields = (ctypes.c_void_p * 1)(bogus)
    sums, quads = (capi.GsSummary * 4)(), (capi.GsMorphology * 4)()
    thr, nan, sense = (ctypes.c_float * 4)(0.1, 0.2, 0.3, 0.4), (ctypes.c_float * 4)(0.1, float("nan"), 0.3, 0.4), (ctypes.c_int32 * 1)(1)
    inv = capi.GS_ERR_INVALID
    assert lib.gs_fields_region_summaries(None, fields, 1, 4, 16, sums) == inv
    assert lib.gs_fields_region_summaries(bogus, None, 1, 4, 16, sums) == inv
    assert lib.gs_fields_region_summaries(bogus, fields, 1, 4, 16, None) == inv
    for rh, rw in ((0, 16), (4, 0), (4, 8), (4, 18), (-1, 16)):
        assert lib.gs_fields_region_summaries(bogus, fields, 0, rh, rw, sums) == inv, (rh, rw)
        assert lib.gs_fields_region_morphology(bogus, fields, 0, rh, rw, thr, sense, 1, quads) == inv, (rh, rw)
    assert lib.gs_fields_region_morphology(bogus, fields, 1, 4, 16, None, sense, 1, quads) == inv
    assert lib.gs_fields_region_morphology(bogus, fields, 1, 4, 16, thr, None, 1, quads) == inv
    assert lib.gs_fields_region_morphology(bogus, fields, 1, 4, 16, thr, sense, 1, None) == inv
    for nt in (0, 5, -1):
        assert lib.gs_fields_region_morphology(bogus, fields, 1, 4, 16, thr, sense, nt, quads) == inv, nt
    assert lib.gs_fields_region_morphology(bogus, fields, 1, 4, 16, nan, sense, 2, quads) == inv
    assert b"NaN" in lib.gs_last_error()
    for n in (0, 5):                                                      # (n outside 1..4 is the handles' first refusal)
        assert lib.gs_fields_region_summaries(bogus, fields, n, 4, 16, sums) == inv
        assert lib.gs_fields_region_morphology(bogus, fields, n, 4, 16, thr, sense, 1, quads) == inv


def test_the_library_exports_and_the_header_declares_the_calls(built):
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    assert "#define GS_REGIONS_MAX (1u << 22)" in header and capi.load().gs_abi_version() == 4
    for name in ("gs_region_grid", "gs_fields_region_summaries", "gs_fields_region_morphology"):
        assert name in capi.EXPORTS and name + "(" in header and hasattr(capi.load(), name)


# ---- the Python results ------------------------------------------------------------------------------------------------------
def test_derived_arrays_are_those_of_summary_and_morphology_on_the_crops():
    shape, region = (7, 50), (3, 16)
    a = odd_plane(shape, 9)
    a[0:3, 0:16] = np.float32(np.nan)                                     # a region with no finite cell
    rec = regions_ref.summaries(a, region)
    s = RegionSummaries.from_records(rec, region, shape)
    assert s.region == region and s.shape == shape and s.sum.shape == (3, 4)
    mean, var = s.mean(), s.variance()
    for (i, j), crop in regions_ref.crops(a, region):
        one = Summary(**summary_ref.summary(crop), size=crop.size)
        assert s.at(i, j) == one and s.size[i, j] == crop.size and s.cells[i, j] == one.cells
        if one.cells:
            assert mean[i, j] == one.mean and np.sqrt(var[i, j]) == one.std, (i, j)
        else:
            assert np.isnan(mean[i, j]) and np.isnan(var[i, j]) and np.isnan(one.mean)
    assert np.isnan(mean[0, 0]) and s.nonfinite[0, 0] == 48
    quads = regions_ref.quads(a, region, 0.1, True)
    m = RegionMorphology.from_quads(quads, 0.1, True, region, shape)
    assert m.quads.shape == (3, 4, 6) and m.quads.dtype == np.uint64 and m.threshold == 0.1
    area, perimeter, euler4, euler8 = quad_measures(quads)
    assert np.array_equal(m.area, area) and np.array_equal(m.perimeter, perimeter)
    assert np.array_equal(m.euler4, euler4) and np.array_equal(m.euler8, euler8)
    for (i, j), crop in regions_ref.crops(a, region):
        one = Morphology.from_quads(morph_ref.quads(crop, 0.1, True), 0.1, True, crop.size)
        got = m.at(i, j)
        assert np.array_equal(got.quads, one.quads) and got.cells == one.cells == m.cells[i, j]
        assert (m.area[i, j], m.perimeter[i, j], m.euler4[i, j], m.euler8[i, j]) == (one.area, one.perimeter, one.euler4, one.euler8)
        assert m.area_fraction[i, j] == one.area_fraction


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_simulate_flags():
    a = simulate.parse(["--hip-regions", "16x32", "--hip-regions-every", "3", "--hip-region-threshold-v", "0.25,0.1",
                        "--hip-region-threshold-u", "0.5,0.8"])
    assert a.hip_regions == (16, 32) and a.hip_regions_every == 3
    assert a.hip_region_threshold_v == [0.25, 0.1] and a.hip_region_threshold_u == [0.5, 0.8]
    b = simulate.parse(["--hip-regions", "64"])
    assert b.hip_regions == (64, 64) and b.hip_regions_every is None and b.hip_region_threshold_v is None
    assert simulate.parse([]).hip_regions is None
    for wrong in (["--hip-regions", "16x18"], ["--hip-regions", "0x16"], ["--hip-regions", "8"], ["--hip-regions", "4x16x2"],
                  ["--hip-regions", "ax16"], ["--hip-regions", "16", "--hip-regions-every", "0"],
                  ["--hip-region-threshold-v", "0.25,0.1", "--hip-region-threshold-u", "0.5"], ["--hip-region-threshold-u", "0.5,0.8"],
                  ["--hip-region-threshold-v", "nan"], ["--hip-region-threshold-v", "1,2,3,4,5"], ["--hip-region-threshold-u", "a"]):
        with pytest.raises(SystemExit):
            simulate.parse(wrong)
    assert [i for i in range(1, 8) if simulate.regions_observed(i, 7, None)] == [7]
    assert [i for i in range(1, 8) if simulate.regions_observed(i, 7, 3)] == [3, 6]
    assert [i for i in range(1, 4) if simulate.regions_observed(i, 3, 1)] == [1, 2, 3]
    assert simulate.regions_path("out/run.h5") == "out/run.regions.npz"
    with pytest.raises(ValueError):
        simulate.RegionLog((16, 32), [0.25, 0.1], [0.5])


def test_region_means_of_the_maps():
    shape, region = (5, 40), (2, 16)
    feed = np.repeat(simulate.linear_values(0.01, 0.06, 5)[:, None], 40, axis=1)
    kill = np.repeat(simulate.linear_values(0.04, 0.07, 40)[None, :], 5, axis=0)
    for values in (feed, kill):
        got = simulate.region_means(values, shape, region)
        assert got.shape == (3, 3) and got.dtype == np.float64
        for (i, j), crop in regions_ref.crops(values, region):
            assert got[i, j] == pytest.approx(float(crop.astype(np.float64).mean()), rel=1e-14), (i, j)
    uniform = simulate.region_means(np.float32(0.03), shape, region)
    assert uniform.shape == (3, 3) and np.all(uniform == float(np.float32(0.03)))


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def test_cpp_regions_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("regions_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_regions_mirror.py)
        r = run_program([str(exe), "64", "128", "16", "32", "5", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
