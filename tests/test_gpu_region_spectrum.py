"""Regional power spectra on the device (gs_fields_region_spectrum) against their definition (tests/region_spectrum_ref.py:
the whole-grid restatement on every region's crop, fed with the library's own tables): ``raw`` as f64 bit patterns and the
tile counts equal, at the smallest shapes that can go wrong -- one tile per region, ragged regions, region shapes that are
no multiples of the tile, no tile anywhere, one region, 17 and 33 tiles per band of a region -- for every tile size."""
import ctypes
import functools

import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, RegionSpectrum, Simulation, capi
from grayscott_amd.simulation import region_spectrum_fields, spectrum_tables
from tests import region_spectrum_ref as ref
from tests import regions_ref, spectrum_ref
from tests.helpers import species_from_arrays, stress_fields
from tests.test_gpu_spectrum import planes_for

pytestmark = pytest.mark.gpu

WINDOWS = ("none", "hann")
CASES = [(16, (48, 112), (16, 16)), (16, (48, 112), (32, 48)), (16, (48, 112), (20, 36)), (16, (48, 112), (8, 16)),
         (16, (48, 112), (1, 16)), (16, (48, 112), (48, 112)), (16, (48, 112), (64, 128)),
         (16, (32, 560), (16, 272)), (16, (16, 544), (16, 528)),
         (32, (70, 100), (35, 52)), (64, (130, 200), (65, 100)), (64, (130, 200), (64, 128)), (128, (261, 260), (130, 132))]


@functools.lru_cache(maxsize=None)
def tables(T):
    return spectrum_tables(T)


def want_of(plane, region, T, window):
    h, w = tables(T)
    return ref.by_crop(plane, region, T, WINDOWS.index(window), h, w)


def assert_same(got: RegionSpectrum, want, what):
    power, tiles = want
    assert got.raw.dtype == np.float64 and got.raw.shape == power.shape, (what, got.raw.shape, power.shape)
    assert np.array_equal(got.tiles_used, tiles[..., 0]) and np.array_equal(got.tiles_skipped, tiles[..., 1]), (what, got.tiles_used, tiles)
    if got.raw.tobytes() != power.tobytes():
        bad = np.argwhere(got.raw.view(np.uint64) != power.view(np.uint64))
        at = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {power.size} bins differ, first {at}: {got.raw[at]!r}, not {power[at]!r}")


def one_context(**kw):
    return Simulation.new(Parameters(), HipArgs(devices=[0], **kw))


def field_of(sim, plane):
    f = HipConcentration(sim.context, plane.shape)
    f.upload(sim.context, plane)
    return f


# ---- parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,shape,region", CASES)
def test_parity(built, T, shape, region):
    sim = one_context()
    f = HipConcentration(sim.context, shape)
    for kind, plane in planes_for(shape, T, 7 * T + region[1]):
        f.upload(sim.context, plane)
        for window in WINDOWS:
            got = f.region_spectrum(sim.context, region, T, window)
            assert (got.tile, got.window, got.region, got.shape) == (T, WINDOWS.index(window), region, shape)
            assert_same(got, want_of(plane, region, T, window), f"{kind} {shape} regions {region} T {T} {window}")
        assert f.make_scalar_view(sim.context).tobytes() == plane.tobytes()       # the plane is what was uploaded
    if region[0] < T or region[1] < T:
        assert not got.tiles_used.any() and not got.tiles_skipped.any() and not got.raw.any()
    if region[0] >= shape[0] and region[1] >= shape[1]:                           # one region: the whole grid's bits
        whole = f.spectrum(sim.context, T, window)
        assert got.raw.shape[:2] == (1, 1) and got.raw[0, 0].tobytes() == whole.raw.tobytes()
        assert (int(got.tiles_used[0, 0]), int(got.tiles_skipped[0, 0])) == (whole.tiles_used, whole.tiles_skipped)
    sim.context.close()


@pytest.mark.parametrize("T", (16, 32))
def test_the_unaligned_load_path(built, T):
    shape, region = (48, 112), (20, 36)
    sim = one_context(pitch_pad=3)
    for kind, plane in planes_for(shape, T, T):
        f = field_of(sim, plane)
        for window in WINDOWS:
            assert_same(f.region_spectrum(sim.context, region, T, window), want_of(plane, region, T, window), f"{kind} T {T} {window}")
    sim.context.close()


# ---- non-finite cells, overflow --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,shape,region", [(16, (48, 112), (32, 48)), (16, (48, 112), (20, 36)), (64, (130, 200), (65, 100))])
def test_a_non_finite_cell_skips_its_tile_in_its_region_alone(built, T, shape, region):
    sim = one_context()
    f = HipConcentration(sim.context, shape)
    clean = np.random.default_rng(T + region[1]).standard_normal(shape).astype(np.float32)
    f.upload(sim.context, clean)
    base = f.region_spectrum(sim.context, region, T, "hann")
    assert_same(base, want_of(clean, region, T, "hann"), "clean")
    rr, rc = regions_ref.grid(shape, region)
    for value, (i, j) in ((np.nan, (0, rc - 1)), (np.inf, (0, 0)), (-np.inf, (rr - 1, 0))):
        if base.tiles_used[i, j] == 0:
            i, j = 0, 0
        plane = clean.copy()
        plane[i * region[0] + T - 1, j * region[1] + T - 1] = value              # the last cell of the region's first tile
        f.upload(sim.context, plane)
        got = f.region_spectrum(sim.context, region, T, "hann")
        assert_same(got, want_of(plane, region, T, "hann"), f"{value} in region ({i}, {j})")
        skipped = np.zeros((rr, rc), np.uint64)
        skipped[i, j] = 1
        assert np.array_equal(got.tiles_skipped, skipped) and np.array_equal(got.tiles_used + skipped, base.tiles_used)
        others = np.ones((rr, rc), bool)
        others[i, j] = False
        assert got.raw[others].tobytes() == base.raw[others].tobytes()           # every other region's bits are unchanged
    # a NaN in the rows and columns that a region's tiles leave over is not looked at
    if region[0] % T and region[1] % T:
        plane = clean.copy()
        for i in range(rr):
            plane[i * region[0] + region[0] // T * T:(i + 1) * region[0], :] = np.nan
        for j in range(rc):
            plane[:, j * region[1] + region[1] // T * T:(j + 1) * region[1]] = np.inf
        f.upload(sim.context, plane)
        got = f.region_spectrum(sim.context, region, T, "hann")
        full = np.zeros((rr, rc), bool)
        full[:shape[0] // region[0], :shape[1] // region[1]] = True              # (a ragged region's tiles may reach those rows)
        assert got.raw[full].tobytes() == base.raw[full].tobytes() and not got.tiles_skipped[full].any()
        assert_same(got, want_of(plane, region, T, "hann"), "NaN in the leftover rows and columns")
    sim.context.close()


def test_overflow_inside_a_tile_propagates(built):
    """As in the whole-grid test: the finite bins are compared as bits, the others by kind."""
    T, shape, region = 16, (32, 96), (16, 48)
    sim = one_context()
    plane = np.random.default_rng(3).standard_normal(shape).astype(np.float32)
    plane[:16, 16:32] *= np.float32(1e37)
    f = field_of(sim, plane)
    got = f.region_spectrum(sim.context, region, T, "none")
    power, tiles = want_of(plane, region, T, "none")
    assert np.array_equal(got.tiles_used, tiles[..., 0]) and np.all(got.tiles_used == 3) and not got.tiles_skipped.any()
    assert not np.isfinite(power[0, 0]).all() and np.isfinite(power[0, 1]).all() and np.isfinite(power[1]).all()
    assert np.array_equal(np.isnan(got.raw), np.isnan(power)) and np.array_equal(np.isposinf(got.raw), np.isposinf(power))
    ok = np.isfinite(power)
    assert got.raw[ok].tobytes() == power[ok].tobytes()
    sim.context.close()


# ---- call forms ------------------------------------------------------------------------------------------------------------------
def test_field_lists(built):
    shape, region, T = (70, 100), (35, 52), 32
    sim = one_context()
    planes = [np.random.default_rng(20 + k).standard_normal(shape).astype(np.float32) for k in range(4)]
    planes[2][5, 7] = np.nan
    fields = [field_of(sim, p) for p in planes]
    alone = [f.region_spectrum(sim.context, region, T, "hann") for f in fields]
    for k in range(4):
        assert_same(alone[k], want_of(planes[k], region, T, "hann"), f"plane {k} alone")
    for n in (1, 2, 3, 4):
        got = region_spectrum_fields(sim.context, fields[:n], region, T, "hann")
        assert len(got) == n
        for k in range(n):
            assert got[k].raw.tobytes() == alone[k].raw.tobytes(), (n, k)
            assert np.array_equal(got[k].tiles_used, alone[k].tiles_used) and np.array_equal(got[k].tiles_skipped, alone[k].tiles_skipped)
    sim.context.close()


def test_a_developed_pattern(built):
    shape, region = (128, 256), (64, 64)
    sim = one_context()
    species = sim.make_species(list(shape))
    sim.perform_steps(species, 200)
    in_u, in_v, _, _ = species.in_out()
    u, v = in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)
    before = (sim.context.stats(), sim.context.info())
    for T in (16, 64):
        for window in WINDOWS:
            su, sv = species.region_spectrum(region, T, window)
            assert_same(su, want_of(u, region, T, window), f"U T {T} {window}")
            assert_same(sv, want_of(v, region, T, window), f"V T {T} {window}")
    assert (sim.context.stats(), sim.context.info()) == before
    assert np.all(sv.tiles_used == 1) and sv.raw.shape == (2, 4, 64, 33)
    in_u, in_v, _, _ = species.in_out()
    assert in_u.make_scalar_view(sim.context).tobytes() == u.tobytes() and in_v.make_scalar_view(sim.context).tobytes() == v.tobytes()
    sim.context.close()


# ---- ghost rows and pitch padding ------------------------------------------------------------------------------------------------
def test_poisoned_ghost_rows_and_padding_change_nothing(built):
    from tests.test_gpu_observe_property import poison

    shape, region = (96, 300), (32, 100)
    plane = np.random.default_rng(9).standard_normal(shape).astype(np.float32)
    for args in (HipArgs(devices=[0]), HipArgs(devices=[0], pitch_pad=3), HipArgs(devices=[0] * 3)):
        sim = Simulation.new(Parameters(), args)
        f = field_of(sim, plane)
        poison(f, np.nan)
        for T in (16, 32):
            assert_same(f.region_spectrum(sim.context, region, T, "hann"), want_of(plane, region, T, "hann"),
                        f"poisoned, {args.devices}, T {T}")
        sim.context.close()


# ---- slab chains -----------------------------------------------------------------------------------------------------------------
def chain_spectra(args, u, v, region, T):
    sim = Simulation.new(Parameters(), args)
    species = species_from_arrays(sim, u, v)
    before = sim.context.stats()
    out = [species.region_spectrum(region, T, w) for w in WINDOWS]
    assert sim.context.stats() == before
    sim.context.close()
    return out


def test_slab_chains_give_the_same_bits(built):
    shape = (128, 200)
    u = np.random.default_rng(31).standard_normal(shape).astype(np.float32)
    v = stress_fields(shape, 32)[1]
    v[40, 70] = np.inf
    # every seam (64; 32, 64, 96) is a multiple of rh; there is no condition on T at the seams
    for T, region, chains in ((16, (32, 64), ([0] * 2, [0] * 4)), (16, (16, 48), ([0] * 2, [0] * 4)), (64, (64, 100), ([0] * 2,)),
                              (16, (32, 100), ([0] * 4,)), (32, (32, 64), ([0] * 4,))):
        one = chain_spectra(HipArgs(devices=[0]), u, v, region, T)
        for k, window in enumerate(WINDOWS):
            assert_same(one[k][0], want_of(u, region, T, window), f"one slab, U, T {T} {region}")
            assert_same(one[k][1], want_of(v, region, T, window), f"one slab, V, T {T} {region}")
        for devices in chains:
            got = chain_spectra(HipArgs(devices=devices), u, v, region, T)
            for k in range(2):
                for s in range(2):
                    assert got[k][s].raw.tobytes() == one[k][s].raw.tobytes(), (T, region, devices, k, s)
                    assert np.array_equal(got[k][s].tiles_used, one[k][s].tiles_used)
                    assert np.array_equal(got[k][s].tiles_skipped, one[k][s].tiles_skipped)


def test_a_seam_off_the_regions_is_refused_and_the_context_goes_on(built):
    shape = (128, 200)
    u, v = stress_fields(shape, 5)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * 3))                  # seams at 42 and 85
    species = species_from_arrays(sim, u, v)
    for region, T in (((32, 64), 16), ((16, 48), 16), ((64, 100), 64)):
        with pytest.raises(capi.GsError) as e:
            species.region_spectrum(region, T, "hann")
        assert e.value.code == capi.GS_ERR_UNSUPPORTED, (region, T)
    su, sv = species.region_spectrum((1, 64), 16, "hann")                         # rh = 1: every seam is a multiple; no tile fits
    assert not sv.raw.any() and sv.raw.shape == (128, 4, 16, 9)
    su, sv = species.summary()
    assert sv.nonfinite == 0
    sim.context.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(built):
    sim = one_context()
    other = one_context()
    lib = sim.context._lib
    F = lib.gs_fields_region_spectrum
    INV = capi.GS_ERR_INVALID
    err = lambda: lib.gs_last_error().decode()  # noqa: E731
    dp, up = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)
    power, tiles = np.zeros(4 * 6 * 7 * 16 * 9), np.zeros(4 * 6 * 7 * 2, np.uint64)
    P, Tl = power.ctypes.data_as(dp), tiles.ctypes.data_as(up)
    garbage = (ctypes.c_void_p * 4)(0xdead0, 0xdead0, 0xdead0, 0xdead0)           # never dereferenced by the early refusals
    ctx = sim.context.handle
    for args, word in (((1, 16, 16, 48, 1, P, Tl), "a tile of"), ((1, 16, 16, 16, 2, P, Tl), "window"),
                       ((1, 16, 18, 16, 1, P, Tl), "region width"), ((1, 0, 16, 16, 1, P, Tl), "region height"),
                       ((1, 16, 16, 16, 1, None, Tl), "null output"), ((1, 16, 16, 16, 1, P, None), "null output"),
                       ((1, 0, 18, 48, 2, None, Tl), "null output"), ((1, 0, 18, 48, 2, P, Tl), "a tile of"),
                       ((1, 0, 18, 16, 2, P, Tl), "window"), ((1, 0, 18, 16, 1, P, Tl), "region height")):
        assert F(ctx, garbage, *args) == INV and word in err(), (args[:5], err())
    a, b = HipConcentration(sim.context, (48, 112)), HipConcentration(sim.context, (48, 96))
    foreign = HipConcentration(other.context, (48, 112))
    plane = np.random.default_rng(1).standard_normal((48, 112)).astype(np.float32)
    a.upload(sim.context, plane)
    for fields in ([a, b], [a, foreign], [a] * 5, []):
        with pytest.raises(capi.GsError) as e:
            region_spectrum_fields(sim.context, fields, (16, 16), 16, "hann")
        assert e.value.code == INV, len(fields)
    handles = (ctypes.c_void_p * 4)(a.handle, None, None, None)
    assert F(ctx, handles, 2, 16, 16, 16, 1, P, Tl) == INV and "field 1" in err()
    # the result cap: no tile fits anywhere, but 256 x 256 regions of 8322 words are too many
    big = HipConcentration(sim.context, (4096, 4096))
    with pytest.raises(capi.GsError) as e:
        big.region_spectrum(sim.context, (16, 16), 128, "hann")
    assert e.value.code == INV and "words each" in str(e.value)
    big.destroy()
    # the records' cap while the result cap holds: tall thin regions, a record per tile (tests/test_region_spectrum_cpu.py)
    shape, region = (7680, 7680), (7680, 16)
    assert ref.records(shape, region, 16, 4) > capi.GS_REGION_SPECTRUM_RECORDS_MAX >= ref.records(shape, region, 16, 3)
    assert 480 * (16 * 9 + 2) <= capi.GS_REGION_SPECTRUM_MAX
    tall = HipConcentration(sim.context, shape)
    with pytest.raises(capi.GsError) as e:
        region_spectrum_fields(sim.context, [tall] * 4, region, 16, "hann")
    assert e.value.code == INV and "segment records" in str(e.value)
    tall.destroy()
    # the context goes on working
    assert_same(a.region_spectrum(sim.context, (32, 48), 16, "hann"), want_of(plane, (32, 48), 16, "hann"), "after the refusals")
    sim.context.close()
    other.context.close()
