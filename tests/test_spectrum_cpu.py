"""Power spectra without a GPU: the exports and the build unit, the tables against numpy, the restatement
(tests/spectrum_ref.py) against exact arithmetic, the ``Spectrum`` object on synthetic stripes, the code objects of the
``gs_spectrum_`` kernels and the sweep's flags."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import grayscott_amd
from grayscott_amd import Spectrum, _build, capi
from grayscott_amd.simulation import spectrum_tables
from tests import spectrum_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_spectrum_tables", "gs_fields_spectrum", "gs_members_spectrum")


# ---- exports and build -----------------------------------------------------------------------------------------------------------
def test_exports_header_and_build_unit(built):
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    lib = capi.load()
    for name in NAMES:
        assert name in capi.EXPORTS
        assert re.search(r"\bint32_t %s\(" % name, header), name
        assert getattr(lib, name).restype is ctypes.c_int32, name
    assert lib.gs_abi_version() == 4 and "#define GS_ABI_VERSION 4" in header
    assert "Spectrum" in grayscott_amd.__all__
    assert [u for u in _build.UNITS if u[0] == "gs_spectrum.hip"] == [("gs_spectrum.hip", "gs_spectrum_k.o", [])]
    for missing in ("per-region spectra", "cross-spectrum of U with V", "overlapping tiles", "tiles that wrap"):
        assert missing in header, missing
    assert "autocorrelation and spectra" not in " ".join(header.split())


def test_refusals_need_no_device(built):
    lib = capi.load()
    h = (ctypes.c_float * 128)()
    for tile in (0, 8, 48, 256, -16):
        assert lib.gs_spectrum_tables(tile, h, h) == capi.GS_ERR_INVALID, tile
    power, tiles = (ctypes.c_double * 1)(), (ctypes.c_uint64 * 2)()
    # tile, window and the outputs are looked at before any handle: null handles never get that far
    for tile, window, p, t in ((48, 1, power, tiles), (64, 2, power, tiles), (64, -1, power, tiles), (64, 1, None, tiles),
                               (64, 1, power, None)):
        assert lib.gs_fields_spectrum(None, None, 1, tile, window, p, t) == capi.GS_ERR_INVALID
        assert lib.gs_members_spectrum(None, None, 0, 1, tile, window, p, t) == capi.GS_ERR_INVALID


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    key = lambda x: np.where(x.view(np.int32) < 0, np.int32(-2 ** 31) - x.view(np.int32), x.view(np.int32)).astype(np.int64)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("T", ref.TILES)
def test_tables_against_numpy(built, T):
    h, w = spectrum_tables(T)
    assert h.dtype == np.float32 and h.shape == (T,) and w.dtype == np.complex64 and w.shape == (T // 2,)
    j, k = np.arange(T, dtype=np.float64), np.arange(T // 2, dtype=np.float64)
    assert ulps(h, (0.5 - 0.5 * np.cos(2 * np.pi * j / T)).astype(np.float32)).max() <= 1
    assert ulps(w.real, np.cos(2 * np.pi * k / T).astype(np.float32)).max() <= 1
    assert ulps(w.imag, (-np.sin(2 * np.pi * k / T)).astype(np.float32)).max() <= 1
    assert h[0] == 0.0 and w[0] == 1.0 and h[T // 2] == 1.0


# ---- the restatement against exact arithmetic ------------------------------------------------------------------------------------
def sample_tiles(T, seed):
    rng = np.random.default_rng(seed)
    c = np.arange(T)
    return np.stack([rng.standard_normal((T, T)).astype(np.float32), rng.random((T, T), dtype=np.float32),
                     np.broadcast_to((0.5 + 0.25 * np.cos(2 * np.pi * 3 * c / T)).astype(np.float32), (T, T)).copy(),
                     np.where(rng.random((T, T)) < 0.05, np.float32(0.4), np.float32(0.0)).astype(np.float32)])


def test_the_bound_is_the_issues():
    assert abs(ref.bound(16) - 6.8e-6) < 0.1e-6 and abs(ref.bound(128) - 1.16e-5) < 0.02e-5


@pytest.mark.parametrize("window", (0, 1))
@pytest.mark.parametrize("T", ref.TILES)
def test_restatement_against_exact_arithmetic(built, T, window):
    h, w = spectrum_tables(T)
    tiles = sample_tiles(T, T + window)
    p = ref.tile_power(tiles, h, w, window).astype(np.float64)
    P = ref.exact_power(tiles, h, window)
    for k in range(tiles.shape[0]):
        err, total = np.abs(p[k] - P[k]).sum(), P[k].sum()
        print(f"T {T} window {window} tile {k}: sum |p - P| / sum P = {err / total:.3e}, B = {ref.bound(T):.3e}")
        assert total > 0 and err <= ref.bound(T) * total, (T, window, k, err / total)


# ---- exact cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", ref.TILES)
def test_a_constant_tile_has_no_power(built, T):
    h, w = spectrum_tables(T)
    for window in (0, 1):
        for value in (0.0, 0.3, -7.25, 1e-40, 3e38):
            power, tiles = ref.spectrum(np.full((T, 2 * T), value, np.float32), T, window, h, w)
            assert not power.any() and not np.signbit(power).any() and tuple(tiles) == (2, 0), (T, window, value)


@pytest.mark.parametrize("T,m", [(16, 3), (32, 5), (64, 8), (128, 20)])
def test_a_cosine_plane_has_one_bin(built, T, m):
    h, w = spectrum_tables(T)
    c = np.arange(2 * T)
    plane = np.broadcast_to((0.5 + 0.25 * np.cos(2 * np.pi * m * c / T)).astype(np.float32), (T, 2 * T))
    power, tiles = ref.spectrum(plane, T, 0, h, w)
    assert power[0, m] >= 0.999 * power.sum() and tuple(tiles) == (2, 0)
    s = Spectrum.from_raw(power, T, "none", tiles)
    assert abs(s.peak_wavenumber() - m / T) <= 1e-6 and abs(s.wavelength() - T / m) <= 1e-4
    assert abs(s.power[0, m] / (T * T * 0.25 ** 2 / 4) - 1.0) <= 1e-5   # |T^2 A / 2|^2 over the window's energy T^2


# ---- the Spectrum object on f64 spectra of synthetic stripes ---------------------------------------------------------------------
def f64_spectrum(plane, T=64, window="hann"):
    tiles = ref.tiles_of(plane, T).reshape(-1, T, T).astype(np.float64)
    y = tiles - tiles.mean(axis=(1, 2), keepdims=True)
    if window == "hann":
        hann = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(T) / T)
        y = y * hann[None, :, None] * hann[None, None, :]
    raw = (np.abs(np.fft.rfft2(y, axes=(1, 2))) ** 2).sum(axis=0)
    return Spectrum.from_raw(raw, T, window, (tiles.shape[0], 0))


def stripes(shape, period, degrees):
    """cos(2 pi (r sin a + c cos a) / period): the wave vector at `degrees` from the column axis towards the row axis."""
    r, c = np.mgrid[:shape[0], :shape[1]]
    a = np.radians(degrees)
    return (0.5 + 0.25 * np.cos(2 * np.pi * (r * np.sin(a) + c * np.cos(a)) / period)).astype(np.float32)


@pytest.mark.parametrize("period", (8, 12, 16))
def test_wavelength_of_stripes(period):
    T = 64
    for degrees in (0, 30, 90):
        s = f64_spectrum(stripes((128, 192), period, degrees), T)
        assert abs(1.0 / s.wavelength() - 1.0 / period) <= 1.0 / (2 * T), (period, degrees, s.wavelength())
    assert s.tiles_used == 6 and s.tiles_skipped == 0


def test_orientation_and_anisotropy_of_stripes():
    rng = np.random.default_rng(5)
    noise = f64_spectrum(rng.standard_normal((256, 256)).astype(np.float32))
    assert noise.anisotropy() < 0.5
    for degrees in (0, 45, 90):
        s = f64_spectrum(stripes((128, 192), 12, degrees))
        off = abs(s.orientation() - degrees) % 180.0
        assert min(off, 180.0 - off) <= 10.0, (degrees, s.orientation())
        assert s.anisotropy() > noise.anisotropy() and s.anisotropy() > 0.9, (degrees, s.anisotropy())


def test_radial_rings_and_the_flat_spectrum():
    T = 16
    flat = Spectrum.from_raw(np.ones((T, T // 2 + 1)), T, "none", (1, 0))
    radial = flat.radial()
    assert radial.shape == (T // 2 + 1,) and np.allclose(radial, 1.0 / (T * T))
    assert flat.peak_wavenumber() is None and flat.wavelength() is None and flat.orientation() is None and flat.anisotropy() is None
    none = Spectrum.from_raw(np.zeros((T, T // 2 + 1)), T, "hann", (0, 3))
    assert np.isnan(none.power).all() and none.peak_wavenumber() is None and none.tiles_skipped == 3
    # the weights: a bin strictly inside 0 < kc < T/2 stands for its mirror image too
    one = np.zeros((T, T // 2 + 1))
    one[0, 3] = one[3, 0] = 1.0
    ring, weight = Spectrum.from_raw(one, T, "none", (1, 0))._rings()
    assert ring[0, 3] == ring[3, 0] == ring[T - 3, 0] == 3 and weight[0, 3] == 2.0 and weight[3, 0] == 1.0 and weight[5, T // 2] == 1.0
    assert Spectrum.from_raw(one, T, "hann", (1, 0)).window_energy == pytest.approx((3 * T / 8) ** 2)


# ---- code objects ----------------------------------------------------------------------------------------------------------------
def test_code_objects(built):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import codeobj
    finally:
        sys.path.pop(0)
    found = [k for k in codeobj.kernels() if "gs_spectrum_" in k.name]
    names = " ".join(k.name for k in found)
    assert "gs_spectrum_fold_k" in names and all(f"gs_spectrum_tiles_k<{T}, {v}>" in names for T in ref.TILES for v in ("true", "false"))
    for k in found:
        assert k.vgpr_spill == 0 and k.sgpr_spill == 0 and k.scratch == 0 and not k.dynamic_stack, k.name
        # the float multiply-adds of every spelling (codeobj.FLOAT_FMA: v_fma, v_fmac, v_mad, v_pk_fma, ... on f16/f32/f64;
        # integer v_mad_u32 / v_mad_u64 address arithmetic rounds nothing and is not meant)
        assert k.matching(codeobj.FLOAT_FMA) == [], k.name
        assert k.matching(r"^v_(pk_)?(fma|fmac)") == [], k.name
        assert k.lds <= 160 * 1024, k.name
        assert k.denorm_mode_32 == 3, k.name                               # sub-normal values kept


def test_the_tile_kernels_dynamic_lds_fits():
    """What gs_spectrum.hip asks for per workgroup (its Geo<T>::LDS) stays under the 160 KiB of a CU."""
    for T in ref.TILES:
        rows_at_a_time = min(256 // (T // 2), T)
        lds = T * 8 + T * (T // 2 + 1) * 8 + rows_at_a_time * (T + 1) * 8 + (T // 2) * 8 + T * 4 + 8
        assert lds <= 160 * 1024, (T, lds)
    source = open(os.path.join(ROOT, "grayscott_amd", "csrc", "gs_spectrum.hip")).read()
    assert "(size_t)T * 8 + (size_t)BINS * 8 + (size_t)RB * SP * 8 + (size_t)HB * 8 + (size_t)T * 4 + 8" in source


# ---- the sweep's flags -----------------------------------------------------------------------------------------------------------
def test_sweep_parser():
    from grayscott_amd import sweep

    base = ["--feed", "0.02:0.04:2", "--kill", "0.05:0.06:2"]
    args = sweep.parse(base)
    assert args.spectrum_every == 0 and args.spectrum_tile == 64 and args.spectrum_window == "hann"
    args = sweep.parse(base + ["--spectrum-every", "32", "--spectrum-tile", "128", "--spectrum-window", "none"])
    assert args.spectrum_every == 32 and args.spectrum_tile == 128 and args.spectrum_window == "none"
    for bad in (["--spectrum-tile", "48"], ["--spectrum-window", "hamming"], ["--spectrum-every", "-1"]):
        with pytest.raises(SystemExit):
            sweep.parse(base + bad)
    assert sweep.spectrum_path("out/run.h5") == "out/run.spectrum.npz"
    assert "--spectrum-every" in sweep.__doc__ and ".spectrum.npz" in sweep.__doc__
