"""Power spectra on the device (gs_fields_spectrum, gs_members_spectrum) against their definition (tests/spectrum_ref.py,
fed with the library's own tables): ``power`` as f64 bit patterns and ``tiles`` equal, at the smallest shapes that can go
wrong -- one tile, ragged on both sides, 17 and 33 tiles per band (the segment seams), no tile -- for every tile size."""
import ctypes
import functools

import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, Simulation, Spectrum, capi
from grayscott_amd.simulation import spectrum_fields, spectrum_tables
from tests import spectrum_ref as ref
from tests.helpers import species_from_arrays, stress_fields

pytestmark = pytest.mark.gpu

SHAPES = [(16, (16, 16)), (16, (33, 50)), (16, (16, 272)), (16, (48, 528)), (16, (15, 40)), (32, (70, 100)), (64, (64, 128)),
          (64, (130, 200)), (128, (128, 256)), (128, (261, 133))]
WINDOWS = ("none", "hann")


@functools.lru_cache(maxsize=None)
def tables(T):
    return spectrum_tables(T)


def want_of(plane, T, window):
    h, w = tables(T)
    return ref.spectrum(plane, T, WINDOWS.index(window), h, w)


def assert_same(got: Spectrum, want, what):
    power, tiles = want
    assert got.raw.dtype == np.float64 and got.raw.shape == power.shape, what
    assert (got.tiles_used, got.tiles_skipped) == (int(tiles[0]), int(tiles[1])), (what, got.tiles_used, got.tiles_skipped, tiles)
    if got.raw.tobytes() != power.tobytes():
        bad = np.argwhere(got.raw.view(np.uint64) != power.view(np.uint64))
        at = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {power.size} bins differ, first {at}: {got.raw[at]!r}, not {power[at]!r}")


def planes_for(shape, T, seed):
    rng = np.random.default_rng(seed)
    yield "normal", rng.standard_normal(shape).astype(np.float32)
    yield "stress", stress_fields(shape, seed)[1]
    yield "constant", np.full(shape, 0.375, np.float32)
    # tiles of sub-normals, of tiny and of large values side by side: every tile is scaled by its own power of two
    scaled = rng.standard_normal(shape).astype(np.float32)
    for k, (r, c) in enumerate(np.ndindex(max(shape[0] // T, 1), max(shape[1] // T, 1))):
        scaled[r * T:(r + 1) * T, c * T:(c + 1) * T] *= np.float32((1e-42, 1e-30, 1.0, 1e12)[k % 4])
    yield "scaled", scaled


def one_context():
    return Simulation.new(Parameters(), HipArgs(devices=[0]))


# ---- parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,shape", SHAPES)
def test_parity(built, T, shape):
    sim = one_context()
    f = HipConcentration(sim.context, shape)
    for kind, plane in planes_for(shape, T, 11 * T + shape[1]):
        f.upload(sim.context, plane)
        for window in WINDOWS:
            got = f.spectrum(sim.context, T, window)
            assert got.tile == T and got.window == WINDOWS.index(window)
            assert_same(got, want_of(plane, T, window), f"{kind} {shape} T {T} {window}")
        assert f.make_scalar_view(sim.context).tobytes() == plane.tobytes()       # the plane is what was uploaded
    if shape[0] < T or shape[1] < T:
        assert got.tiles_used == 0 and not got.raw.any()
    sim.context.close()


def test_a_developed_pattern(built):
    shape = (128, 256)
    sim = one_context()
    species = sim.make_species(list(shape))
    sim.perform_steps(species, 200)
    in_u, in_v, _, _ = species.in_out()
    u, v = in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)
    before = (sim.context.stats(), sim.context.info())
    for T in ref.TILES:
        for window in WINDOWS:
            su, sv = species.spectrum(T, window)
            assert_same(su, want_of(u, T, window), f"U T {T} {window}")
            assert_same(sv, want_of(v, T, window), f"V T {T} {window}")
    assert (sim.context.stats(), sim.context.info()) == before
    assert sv.tiles_used == 2 and sv.raw.sum() > 0 and np.isfinite(sv.radial()).all()
    in_u, in_v, _, _ = species.in_out()
    assert in_u.make_scalar_view(sim.context).tobytes() == u.tobytes() and in_v.make_scalar_view(sim.context).tobytes() == v.tobytes()
    sim.context.close()


def test_a_cosine_plane(built):
    T, m = 64, 5
    sim = one_context()
    c = np.arange(192)
    plane = np.broadcast_to((0.5 + 0.25 * np.cos(2 * np.pi * m * c / T)).astype(np.float32), (128, 192)).copy()
    f = HipConcentration(sim.context, plane.shape)
    f.upload(sim.context, plane)
    got = f.spectrum(sim.context, T, "none")
    assert got.raw[0, m] >= 0.999 * got.raw.sum() and got.tiles_used == 6
    assert abs(got.peak_wavenumber() - m / T) <= 1e-6
    sim.context.close()


# ---- non-finite cells, overflow --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,shape", [(16, (33, 50)), (64, (130, 200)), (128, (128, 256))])
def test_a_non_finite_cell_skips_its_tile(built, T, shape):
    sim = one_context()
    f = HipConcentration(sim.context, shape)
    clean = np.random.default_rng(T).standard_normal(shape).astype(np.float32)
    h, w = tables(T)
    nb, nt = shape[0] // T, shape[1] // T
    for value, (b, j) in ((np.nan, (0, nt - 1)), (np.inf, (nb - 1, 0)), (-np.inf, (0, 0))):
        plane = clean.copy()
        plane[(b + 1) * T - 1, (j + 1) * T - 1] = value                            # the last cell of tile (b, j)
        f.upload(sim.context, plane)
        got = f.spectrum(sim.context, T, "hann")
        assert_same(got, want_of(plane, T, "hann"), f"{value} in tile ({b}, {j})")
        assert got.tiles_skipped == 1 and got.tiles_used == nb * nt - 1
        # all the others are unchanged: the sum over every tile but (b, j), in the fold's order
        others = ref.tiles_of(clean, T).copy()
        p = ref.tile_power(others.reshape(-1, T, T), h, w, 1).astype(np.float64).reshape(nb, nt, T, T // 2 + 1)
        total = np.zeros((T, T // 2 + 1))
        for bb in range(nb):
            band = np.zeros_like(total)
            for s0 in range(0, nt, ref.SEGMENT):
                record = np.zeros_like(total)
                for jj in range(s0, min(s0 + ref.SEGMENT, nt)):
                    if (bb, jj) != (b, j):
                        record = record + p[bb, jj]
                band = band + record
            total = total + band
        assert got.raw.tobytes() == total.tobytes()
    # outside every whole tile a NaN is not looked at
    if shape[0] % T and shape[1] % T:
        plane = clean.copy()
        plane[-1, :] = np.nan
        plane[:, -1] = np.inf
        f.upload(sim.context, plane)
        assert_same(f.spectrum(sim.context, T, "hann"), want_of(clean, T, "hann"), "NaN outside the tiles")
    sim.context.close()


def test_overflow_inside_a_tile_propagates(built):
    """A tile of finite cells whose transform overflows is used, not skipped: its infinities and NaNs reach the sums (the
    sign and payload of a NaN are the adder's own: the finite bins are compared as bits, the others by kind)."""
    T, shape = 16, (16, 48)
    sim = one_context()
    plane = np.random.default_rng(3).standard_normal(shape).astype(np.float32)
    plane[:, 16:32] *= np.float32(1e37)
    f = HipConcentration(sim.context, shape)
    f.upload(sim.context, plane)
    got = f.spectrum(sim.context, T, "none")
    power, tiles = want_of(plane, T, "none")
    assert (got.tiles_used, got.tiles_skipped) == (3, 0) == tuple(int(x) for x in tiles)
    assert not np.isfinite(power).all()
    assert np.array_equal(np.isnan(got.raw), np.isnan(power)) and np.array_equal(np.isposinf(got.raw), np.isposinf(power))
    ok = np.isfinite(power)
    assert got.raw[ok].tobytes() == power[ok].tobytes()
    sim.context.close()


# ---- ghost rows and pitch padding ------------------------------------------------------------------------------------------------
def test_poisoned_ghost_rows_and_padding_change_nothing(built):
    from tests.test_gpu_observe_property import poison

    shape, T = (96, 300), 16
    plane = np.random.default_rng(9).standard_normal(shape).astype(np.float32)
    for args in (HipArgs(devices=[0]), HipArgs(devices=[0], pitch_pad=3), HipArgs(devices=[0] * 3)):
        sim = Simulation.new(Parameters(), args)
        f = HipConcentration(sim.context, shape)
        f.upload(sim.context, plane)
        poison(f, np.nan)
        for T in (16, 32):
            assert_same(f.spectrum(sim.context, T, "hann"), want_of(plane, T, "hann"), f"poisoned, {args.devices}, T {T}")
        sim.context.close()


# ---- call forms and slab chains --------------------------------------------------------------------------------------------------
def test_field_lists(built):
    shape, T = (70, 100), 32
    sim = one_context()
    planes = [np.random.default_rng(20 + k).standard_normal(shape).astype(np.float32) for k in range(4)]
    planes[2][5, 7] = np.nan
    fields = []
    for p in planes:
        f = HipConcentration(sim.context, shape)
        f.upload(sim.context, p)
        fields.append(f)
    alone = [f.spectrum(sim.context, T, "hann") for f in fields]
    for k in range(4):
        assert_same(alone[k], want_of(planes[k], T, "hann"), f"plane {k} alone")
    for n in (1, 2, 3, 4):
        got = spectrum_fields(sim.context, fields[:n], T, "hann")
        assert len(got) == n
        for k in range(n):
            assert got[k].raw.tobytes() == alone[k].raw.tobytes() and got[k].tiles_skipped == alone[k].tiles_skipped, (n, k)
    sim.context.close()


def chain_spectra(args, u, v, T):
    sim = Simulation.new(Parameters(), args)
    species = species_from_arrays(sim, u, v)
    before = sim.context.stats()
    out = [species.spectrum(T, w) for w in WINDOWS]
    assert sim.context.stats() == before
    sim.context.close()
    return out


def test_slab_chains_give_the_same_bits(built):
    shape = (128, 200)
    u = np.random.default_rng(31).standard_normal(shape).astype(np.float32)
    v = stress_fields(shape, 32)[1]
    v[40, 70] = np.inf
    for T, chains in ((16, ([0] * 2, [0] * 4)), (32, ([0] * 2, [0] * 4)), (64, ([0] * 2,))):   # seams at multiples of T
        one = chain_spectra(HipArgs(devices=[0]), u, v, T)
        for k, window in enumerate(WINDOWS):
            assert_same(one[k][0], want_of(u, T, window), f"one slab, U, T {T}")
            assert_same(one[k][1], want_of(v, T, window), f"one slab, V, T {T}")
        for devices in chains:
            got = chain_spectra(HipArgs(devices=devices), u, v, T)
            for k in range(2):
                for s in range(2):
                    assert got[k][s].raw.tobytes() == one[k][s].raw.tobytes(), (T, devices, k, s)
                    assert (got[k][s].tiles_used, got[k][s].tiles_skipped) == (one[k][s].tiles_used, one[k][s].tiles_skipped)


def test_a_seam_off_the_tiles_is_refused_and_the_context_goes_on(built):
    shape = (128, 200)
    u, v = stress_fields(shape, 5)
    for devices, T in (([0] * 2, 128), ([0] * 4, 64), ([0] * 3, 16)):            # seams at 64; 32, 64, 96; 42, 85
        sim = Simulation.new(Parameters(), HipArgs(devices=devices))
        species = species_from_arrays(sim, u, v)
        with pytest.raises(capi.GsError) as e:
            species.spectrum(T, "hann")
        assert e.value.code == capi.GS_ERR_UNSUPPORTED, (devices, T)
        if len(devices) != 3:
            su, sv = species.spectrum(32, "hann")                                  # the context goes on working
            assert_same(sv, want_of(v, 32, "hann"), f"after the refusal, {devices}")
        su, sv = species.summary()
        assert sv.nonfinite == 0
        sim.context.close()


# ---- ensembles -------------------------------------------------------------------------------------------------------------------
def member_planes(count, shape, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((count,) + shape).astype(np.float32)
    v = (rng.random((count,) + shape, dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    return u, v


@pytest.mark.parametrize("T", (16, 64))
def test_ensemble_members_against_lone_fields(built, T):
    shape, count = (64, 128), 6
    sim = one_context()
    ens = sim.make_ensemble(shape, [Parameters()] * count)
    u, v = member_planes(count, shape, T)
    v[2, 63, 127] = np.nan
    ens.upload(u, v)
    lone = HipConcentration(sim.context, shape)
    for window in WINDOWS:
        power, tiles = ens.spectra(tile=T, window=window)
        assert power.shape == (count, 2, T, T // 2 + 1) and power.dtype == np.float64
        assert tiles.shape == (count, 2, 2) and tiles.dtype == np.uint64
        for m in range(count):
            for s, plane in enumerate((u[m], v[m])):
                lone.upload(sim.context, plane)
                alone = lone.spectrum(sim.context, T, window)
                assert_same(alone, want_of(plane, T, window), f"lone field, member {m} species {s}")
                assert power[m, s].tobytes() == alone.raw.tobytes(), (window, m, s)
                assert tuple(tiles[m, s]) == (alone.tiles_used, alone.tiles_skipped), (window, m, s)
        assert tiles[2, 1, 1] == 1
        part_power, part_tiles = ens.spectra(first=2, count=3, tile=T, window=window)
        assert part_power.tobytes() == power[2:5].tobytes() and part_tiles.tobytes() == tiles[2:5].tobytes()
    # a retired member is read like any other
    ens.retire([1])
    ens.perform_steps(4)
    uu, vv = ens.u_views(), ens.result_views()
    assert uu[1].tobytes() == u[1].tobytes()
    power, tiles = ens.spectra(tile=T, window="hann")
    for m in (0, 1, 5):
        for s, plane in enumerate((uu[m], vv[m])):
            assert_same(Spectrum.from_raw(power[m, s], T, "hann", tiles[m, s]), want_of(plane, T, "hann"), f"after steps, member {m}")
    assert ens.u_views().tobytes() == uu.tobytes() and ens.result_views().tobytes() == vv.tobytes()
    ens.destroy()
    sim.context.close()


def test_the_ragged_load_path_on_members_whose_rows_begin_anywhere(built):
    """A member of 35 x 70 cells: rows and members that begin on no 16-byte boundary (a field's rows always do)."""
    shape, count, T = (35, 70), 5, 16
    sim = one_context()
    ens = sim.make_ensemble(shape, [Parameters()] * count)
    u, v = member_planes(count, shape, 77)
    ens.upload(u, v)
    power, tiles = ens.spectra(tile=T, window="hann")
    for m in range(count):
        for s, plane in enumerate((u[m], v[m])):
            assert_same(Spectrum.from_raw(power[m, s], T, "hann", tiles[m, s]), want_of(plane, T, "hann"), f"member {m} species {s}")
    assert tuple(tiles[0, 0]) == (8, 0)
    small_power, small_tiles = ens.spectra(tile=64, window="hann")                # no tile fits
    assert not small_power.any() and not small_tiles.any()
    ens.destroy()
    sim.context.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_refusals(built):
    sim = one_context()
    other = one_context()
    a, b = HipConcentration(sim.context, (32, 32)), HipConcentration(sim.context, (32, 48))
    foreign = HipConcentration(other.context, (32, 32))
    lib = sim.context._lib
    power, tiles = (ctypes.c_double * (4 * 128 * 65))(), (ctypes.c_uint64 * 8)()
    garbage = (ctypes.c_void_p * 1)(0xdead0)                                      # never looked at
    for tile, window, p, t in ((48, 1, power, tiles), (0, 0, power, tiles), (16, 2, power, tiles), (16, 1, None, tiles),
                               (16, 1, power, None)):
        assert lib.gs_fields_spectrum(ctypes.c_void_p(0xdead0), garbage, 1, tile, window, p, t) == capi.GS_ERR_INVALID
        assert lib.gs_members_spectrum(ctypes.c_void_p(0xdead0), ctypes.c_void_p(0xdead0), 0, 1, tile, window, p, t) == capi.GS_ERR_INVALID
    for tile, window in ((48, "hann"), (16, "hamming"), (256, "none")):
        with pytest.raises(capi.GsError) as e:
            a.spectrum(sim.context, tile, window)
        assert e.value.code == capi.GS_ERR_INVALID
    for fields in ([a, b], [foreign], [a] * 5, []):
        with pytest.raises(capi.GsError) as e:
            spectrum_fields(sim.context, fields, 16, "hann")
        assert e.value.code == capi.GS_ERR_INVALID, fields
    ens = sim.make_ensemble((32, 32), [Parameters()] * 2)
    with pytest.raises(capi.GsError) as e:
        ens.spectra(first=1, count=2, tile=16)
    assert e.value.code == capi.GS_ERR_INVALID
    assert a.spectrum(sim.context, 16, "hann").tiles_used == 4                     # the context goes on working
    ens.destroy()
    for s in (sim, other):
        s.context.close()
