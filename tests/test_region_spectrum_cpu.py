"""Regional power spectra (gs_fields_region_spectrum) without a GPU: the exports, the refusals that need no handle in the
header's order through the built library, the record count, ``RegionSpectrum``'s arrays against ``Spectrum`` on the crops
(tests/region_spectrum_ref.py is the definition), a striped plane whose thirds differ, the regions as a partition of the
whole grid's tiles, the driver's flags, the kernels' resources and the C++ mirror."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import region_spectrum_ref as ref
from tests import regions_ref, spectrum_ref
from tests.children import ROOT, build_program, run_program

HEADER = os.path.join(ROOT, "include", "gs_hip.h")


def tables(T):
    from grayscott_amd.simulation import spectrum_tables

    return spectrum_tables(T)


def region_spectrum(plane, region, T, window):
    from grayscott_amd import RegionSpectrum

    h, w = tables(T)
    power, tiles = ref.by_crop(plane, region, T, window, h, w)
    return RegionSpectrum.from_raw(power, tiles, T, window, region, plane.shape)


def whole_spectrum(plane, T, window):
    from grayscott_amd import Spectrum

    h, w = tables(T)
    power, tiles = spectrum_ref.spectrum(plane, T, window, h, w)
    return Spectrum.from_raw(power, T, window, tiles)


# ---- the exports -----------------------------------------------------------------------------------------------------------------
def _prototype(text, name):
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_symbol_is_exported_declared_and_bound(built):
    import grayscott_amd
    from grayscott_amd import capi

    full = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    name = "gs_fields_region_spectrum"
    assert _prototype(text, name) == ["gs_ctx *ctx", "gs_field *const *fields", "int32_t n", "int32_t rh", "int32_t rw",
                                      "int32_t tile", "int32_t window", "double *power", "uint64_t *tiles"]
    # the twins' conventions up to the region shape, the whole-grid spectrum's behind it
    assert _prototype(text, name)[:5] == _prototype(text, "gs_fields_region_histogram")[:5]
    assert _prototype(text, name)[5:] == _prototype(text, "gs_fields_spectrum")[3:]
    assert "#define GS_REGION_SPECTRUM_MAX (1u << 25)" in full and capi.GS_REGION_SPECTRUM_MAX == 1 << 25
    assert "#define GS_REGION_SPECTRUM_RECORDS_MAX (1ull << 27)" in full and capi.GS_REGION_SPECTRUM_RECORDS_MAX == 1 << 27
    assert "power[(((p RR + i) RC + j) T + kr) (T/2 + 1) + kc]" in full
    assert "Not done: per-region spectra" not in full
    assert "Not done: regions of ensemble members; regions that straddle slabs; overlapping tiles. */\n#define GS_REGION_SPECTRUM_MAX" in full
    lib = capi.load()
    i32, u64, vp, P = ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER
    assert name in capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).restype is i32
    assert getattr(lib, name).argtypes == [vp, P(vp), i32, i32, i32, i32, i32, P(ctypes.c_double), P(u64)]
    assert lib.gs_abi_version() == 4 and re.search(r"#define\s+GS_ABI_VERSION\s+4\b", full)
    ffi = open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    assert f"pub fn {name}(" in ffi and "pub const GS_REGION_SPECTRUM_MAX: u64 = 1 << 25;" in ffi
    assert "pub const GS_REGION_SPECTRUM_RECORDS_MAX: u64 = 1 << 27;" in ffi
    hpp = open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    assert "gs_fields_region_spectrum(context_->get(), planes, 2, rh, rw, tile, hann ? 1 : 0, power.data(), tiles.data())" in hpp
    assert "RegionSpectrum" in grayscott_amd.__all__ and "region_spectrum_fields" in grayscott_amd.__all__
    assert hasattr(grayscott_amd.HipConcentration, "region_spectrum") and hasattr(grayscott_amd.Species, "region_spectrum")


# ---- refusals that need no handle, in the header's order -----------------------------------------------------------------------
def test_refusals_decided_before_any_handle_is_looked_at_in_order(built):
    from grayscott_amd import capi

    lib = capi.load()
    INV = capi.GS_ERR_INVALID
    F = lib.gs_fields_region_spectrum
    bogus = ctypes.c_void_p(0xdead0)                                      # never dereferenced: every call is refused first
    fields = (ctypes.c_void_p * 4)(None, None, None, None)
    power = (ctypes.c_double * (4 * 16 * 9))()
    tiles = (ctypes.c_uint64 * 8)()
    err = lambda: lib.gs_last_error().decode()  # noqa: E731

    # 1. a null output, before everything
    assert F(bogus, fields, 1, 16, 16, 16, 1, None, tiles) == INV and "null output" in err()
    assert F(bogus, fields, 1, 16, 16, 16, 1, power, None) == INV and "null output" in err()
    assert F(None, None, 9, 0, 18, 48, 2, None, tiles) == INV and "null output" in err()
    # 2. the tile, then the window, before the region shape
    for tile in (48, 0, 8, 256, -16):
        assert F(bogus, fields, 1, 0, 18, tile, 2, power, tiles) == INV and "a tile of" in err(), tile
    for window in (2, -1):
        assert F(bogus, fields, 1, 0, 18, 16, window, power, tiles) == INV and "window" in err(), window
    # 3. the region shape, before any handle
    for rh, rw in ((0, 16), (16, 0), (16, 8), (16, 18), (-1, 16), (16, -16)):
        assert F(bogus, fields, 9, rh, rw, 16, 1, power, tiles) == INV and "region" in err(), (rh, rw)
        assert F(None, None, 1, rh, rw, 16, 1, power, tiles) == INV and "region" in err(), (rh, rw)
    # 4. then the handles
    assert F(None, fields, 1, 16, 16, 16, 1, power, tiles) == INV and "null argument" in err()
    assert F(bogus, None, 1, 16, 16, 16, 1, power, tiles) == INV and "null argument" in err()
    for n in (0, 5, -1):
        assert F(bogus, fields, n, 16, 16, 16, 1, power, tiles) == INV and "fields (1..4)" in err(), n
    for tile in spectrum_ref.TILES:
        assert F(bogus, fields, 4, 16, 16, tile, 0, power, tiles) == INV and "field 0" in err(), tile


# ---- shapes and the record count -----------------------------------------------------------------------------------------------
def test_the_region_grid_agrees_with_the_result_shapes(built):
    from grayscott_amd.simulation import region_grid

    rng = np.random.default_rng(1)
    for shape, region, T in (((48, 112), (32, 48), 16), ((48, 112), (20, 36), 16), ((70, 100), (35, 52), 32), ((16, 40), (64, 128), 16)):
        plane = rng.standard_normal(shape).astype(np.float32)
        got = region_spectrum(plane, region, T, 1)
        grid = region_grid(shape[0], shape[1], region)
        assert grid == regions_ref.grid(shape, region)
        assert got.raw.shape == grid + (T, T // 2 + 1) and got.raw.dtype == np.float64
        assert got.tiles_used.shape == got.tiles_skipped.shape == grid
        assert (got.tile, got.window, got.region, got.shape) == (T, 1, region, shape)


def test_the_record_count():
    words = 16 * 9 + 2
    # (48, 112) with (32, 48): region rows of 32 and 16 rows -- 2 bands and 1 --, region columns of 48, 48 and 16 columns -- 3, 3
    # and 1 tiles, a segment each: (2 + 1) (1 + 1 + 1) records
    assert ref.records((48, 112), (32, 48), 16) == 9 * words
    # (32, 560) with (16, 272): two region rows of a band each, region columns of 17, 17 and 1 tiles -- 2, 2 and 1 segments
    assert ref.records((32, 560), (16, 272), 16) == 10 * words
    assert ref.records((32, 560), (16, 272), 16, 3) == 30 * words
    # no tile fits: no records
    assert ref.records((48, 112), (8, 16), 16) == 0 and ref.records((48, 112), (32, 48), 64) == 0
    # rh and rw no multiples of T: 20 rows hold a band, 36 columns two tiles, the ragged (8, 4) nothing
    assert ref.records((48, 112), (20, 36), 16) == 2 * 3 * words
    # one region: the whole grid's count, bands times segments of a band
    assert ref.records((48, 528), (48, 528), 16) == 3 * 3 * words
    # tall thin regions: a record per tile -- the shape that reaches the records' cap long before the results' cap
    assert ref.records((7680, 7680), (7680, 16), 16, 4) == 4 * 480 * 480 * words > 1 << 27
    assert ref.records((7680, 7680), (7680, 16), 16, 3) <= 1 << 27 and 480 * words <= 1 << 25


# ---- a striped plane ------------------------------------------------------------------------------------------------------------
def test_the_thirds_of_a_striped_plane_have_their_own_wavelengths(built):
    c = np.arange(128)
    plane = np.concatenate([np.broadcast_to((0.5 + 0.25 * np.cos(2 * np.pi * c / period)).astype(np.float32), (128, 128))
                            for period in (8, 12, 16)], axis=1)
    assert plane.shape == (128, 384)
    T = 64
    regions = region_spectrum(plane, (128, 128), T, 1)
    whole = whole_spectrum(plane, T, 1)
    lengths = regions.wavelength()
    print("regions", lengths, "whole grid", whole.wavelength())
    assert lengths.shape == (1, 3) and np.array_equal(regions.tiles_used, [[4, 4, 4]]) and whole.tiles_used == 12
    for j, period in enumerate((8, 12, 16)):
        assert abs(lengths[0, j] - period) <= 0.5, (j, lengths[0, j])
        assert abs(whole.wavelength() - lengths[0, j]) > 1.0, (j, whole.wavelength(), lengths[0, j])
    # stripes that run down the columns: the wave vector lies along a row, in every region
    assert np.all(np.minimum(regions.orientation(), 180.0 - regions.orientation()) < 1.0) and np.all(regions.anisotropy() > 0.9)


# ---- the Python result ---------------------------------------------------------------------------------------------------------
def test_region_spectrum_object_is_spectrum_on_the_crops(built):
    from grayscott_amd import Spectrum

    shape, region, T = (50, 112), (20, 48), 16
    rng = np.random.default_rng(4)
    plane = rng.standard_normal(shape).astype(np.float32)
    plane[0:20, 0:48] = np.float32(0.375)                                  # a flat region: no peak
    plane[20:36, 48:96] = np.float32(np.nan)                               # a region whose every tile is skipped
    for window in (0, 1):
        got = region_spectrum(plane, region, T, window)
        assert got.raw.shape == (3, 3, T, T // 2 + 1)
        arrays = {m: getattr(got, m)() for m in ("peak_wavenumber", "wavelength", "orientation", "anisotropy")}
        radial, power = got.radial(), got.power
        assert radial.shape == (3, 3, T // 2 + 1) and power.shape == got.raw.shape
        for (i, j), crop in regions_ref.crops(plane, region):
            one = whole_spectrum(crop, T, window)
            at = got.at(i, j)
            assert isinstance(at, Spectrum) and at.raw.tobytes() == one.raw.tobytes()
            assert (at.tile, at.window, at.tiles_used, at.tiles_skipped) == (T, window, one.tiles_used, one.tiles_skipped)
            assert np.array_equal(power[i, j], one.power, equal_nan=True) and np.array_equal(radial[i, j], one.radial(), equal_nan=True)
            for m, a in arrays.items():
                assert a.shape == (3, 3) and a.dtype == np.float64
                scalar = getattr(one, m)()
                assert np.array_equal(a[i, j], np.nan if scalar is None else scalar, equal_nan=True), (m, i, j)
        assert np.isnan(arrays["wavelength"][0, 0]) and got.tiles_used[0, 0] == 3         # flat: used, but no peak
        assert got.tiles_used[1, 1] == 0 and got.tiles_skipped[1, 1] == 3 and np.isnan(power[1, 1]).all()
        assert got.tiles_used[2, 0] == 0 and got.tiles_skipped[2, 0] == 0 and not got.raw[2].any()  # 10 rows: no tile fits
        assert np.isnan(arrays["wavelength"][2, 2]) and not np.isnan(arrays["wavelength"][0, 1])


# ---- the regions partition the tiles where rh and rw are multiples of T ----------------------------------------------------------
@pytest.mark.parametrize("shape,region,T", [((70, 330), (32, 64), 16), ((130, 200), (64, 128), 64), ((64, 600), (32, 96), 32)])
def test_regions_of_whole_tiles_partition_the_grid(built, shape, region, T):
    rng = np.random.default_rng(T)
    plane = rng.standard_normal(shape).astype(np.float32)
    plane[T - 1, 2 * T - 1] = np.nan
    h, w = tables(T)
    for window in (0, 1):
        power, tiles = ref.by_crop(plane, region, T, window, h, w)
        whole, counts = spectrum_ref.spectrum(plane, T, window, h, w)
        assert np.array_equal(tiles.sum(axis=(0, 1)), counts) and counts[1] == 1
        total, N = power.sum(axis=(0, 1)), int(counts[0])
        # sums of N non-negative terms in two orders: each rounds relative, (N - 1) roundings on either side
        assert np.all(np.abs(total - whole) <= 2 * (N - 1) * 2.0 ** -53 * whole)


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_simulate_flags():
    from grayscott_amd import simulate

    a = simulate.parse(["--hip-regions", "64", "--hip-region-spectrum-tile", "16"])
    assert a.hip_regions == (64, 64) and a.hip_region_spectrum_tile == 16 and a.hip_region_spectrum_window == "hann"
    a = simulate.parse(["--hip-regions", "64x128", "--hip-region-spectrum-tile", "64", "--hip-region-spectrum-window", "none"])
    assert a.hip_region_spectrum_tile == 64 and a.hip_region_spectrum_window == "none"
    assert simulate.parse(["--hip-regions", "16"]).hip_region_spectrum_tile is None
    for wrong in (["--hip-region-spectrum-tile", "16"], ["--hip-regions", "64", "--hip-region-spectrum-tile", "48"],
                  ["--hip-regions", "64", "--hip-region-spectrum-tile", "a"],
                  ["--hip-regions", "64", "--hip-region-spectrum-window", "none"],
                  ["--hip-regions", "64", "--hip-region-spectrum-tile", "16", "--hip-region-spectrum-window", "hamming"]):
        with pytest.raises(SystemExit):
            simulate.parse(wrong)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
def test_region_spectrum_kernels_resources(built):
    """Every form of the two regional kernels and of the whole-grid ones: no scratch, no spills, no dynamic stack, no fused
    multiply-add; the tile kernels' only static LDS is the workgroup vote's."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import codeobj
    finally:
        sys.path.pop(0)
    ks = [k for k in codeobj.kernels() if "spectrum" in k.name]
    names = sorted(k.name for k in ks)
    assert len([n for n in names if n.startswith("gs_region_spectrum_tiles_k<")]) == 8, names
    assert len([n for n in names if n.startswith("gs_spectrum_tiles_k<")]) == 8, names
    assert len([n for n in names if n.startswith("gs_region_spectrum_fold_k")]) == 1 and len([n for n in names if n.startswith("gs_spectrum_fold_k")]) == 1
    for k in ks:
        assert (k.scratch, k.vgpr_spill, k.sgpr_spill, k.dynamic_stack) == (0, 0, 0, False), k.name
        assert not [i for i in k.insts if re.match(r"v_(fma|mad|fmac|mac)_f(32|64)", i)], k.name
        assert k.denorm_mode_32 == 3, k.name                                # sub-normal values kept


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def test_cpp_region_spectrum_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("region_spectrum_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_region_spectrum_mirror.py)
        r = run_program([str(exe), "64", "128", "32", "48", "16", "1", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
