"""Regional histograms on the device (gs_fields_region_histogram) against their definition (tests/region_hist_ref.py): every
region's counters are those of the whole-grid rule on that region's cells alone.  Everything is bit for bit."""
import functools
import sys

import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, RegionHistogram, Simulation, capi, hdf5_min
from grayscott_amd.simulation import histogram_fields, region_histogram_fields
from tests import hist_ref, region_hist_ref, regions_ref
from tests.children import ROOT, run_program
from tests.helpers import species_from_arrays, stress_fields

pytestmark = pytest.mark.gpu

T = region_hist_ref.TILE_ROWS  # the kernel's row chunk (kTileRows), restated in tests/region_hist_ref.py
SHAPE = (96, 301)              # the column count is no multiple of 4
# a range per field: the unit interval, one around zero, a tiny one, one far from zero
RANGES = [(0.0, 1.0), (-0.25, 0.5), (1e-3, 2e-3), (-300.0, -100.0)]
BINS = [1, 7, 256, 4096]
# 16 lanes per region (32, 64), 4 lanes (16, 16) and 5 lanes (7, 20) with ragged last rows and columns, exactly one load a row
# (48, 256), one region over the whole plane (100, 320), and rh = 1
REGIONS = [(32, 64), (16, 16), (7, 20), (48, 256), (100, 320), (1, 16)]


@functools.lru_cache(maxsize=None)
def planted(k, bins):
    a = hist_ref.planted(SHAPE, RANGES[k][0], RANGES[k][1], bins, 40 + 7 * k + bins)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(k, region, bins):
    return region_hist_ref.by_label(planted(k, bins), region, RANGES[k][0], RANGES[k][1], bins)


def assert_counters(got: RegionHistogram, wanted, shape, region, what):
    c = region_hist_ref.counters_of(got)
    assert c.dtype == np.uint64 and c.shape == wanted.shape, what
    assert got.region == regions_ref.shape_of(region) and got.shape == tuple(shape), what
    assert np.array_equal(got.cells, regions_ref.sizes(shape, region)), what
    bad = np.argwhere(c != wanted)
    assert bad.size == 0, (f"{what}: [{got.lo}, {got.hi}] bins {got.bins}: {len(bad)} counters differ, first "
                           f"(i, j, slot) = {tuple(bad[0])}: {int(c[tuple(bad[0])])}, not {int(wanted[tuple(bad[0])])}")
    assert np.array_equal(c.sum(axis=2).astype(np.int64), got.cells), what


def upload_all(ctx, planes):
    fields = []
    for p in planes:
        f = HipConcentration(ctx, p.shape)
        f.upload(ctx, np.array(p))
        fields.append(f)
    return fields


# ---- planted values and ragged regions; bins, ranges and field lists ----------------------------------------------------------
@pytest.mark.parametrize("region", REGIONS)
def test_planted_values_and_ragged_regions(built, region):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    for bins in BINS:
        fields = upload_all(ctx, [planted(k, bins) for k in range(4)])
        for n in (1, 2, 3, 4):
            got = region_histogram_fields(ctx, fields[:n], region, bins, RANGES[:n])
            assert len(got) == n
            for k in range(n):
                assert (got[k].lo, got[k].hi) == (float(np.float32(RANGES[k][0])), float(np.float32(RANGES[k][1]))) and got[k].bins == bins
                assert_counters(got[k], want(k, region, bins), SHAPE, region, f"region {region} bins {bins} n {n} field {k}")
        # the plane's own method; the regions partition the cells: every slot sums to the whole grid's
        whole = histogram_fields(ctx, fields, bins, RANGES)
        for k in range(4):
            one = fields[k].region_histogram(ctx, region, bins, RANGES[k])
            assert_counters(one, want(k, region, bins), SHAPE, region, f"region {region} bins {bins} field {k} alone")
            total = region_hist_ref.counters_of(one).sum(axis=(0, 1), dtype=np.uint64)
            assert np.array_equal(total[:bins], whole[k].counts) and tuple(int(x) for x in total[bins:]) == (whole[k].below, whole[k].above, whole[k].nan)
            assert np.array_equal(total, hist_ref.histogram(planted(k, bins), RANGES[k][0], RANGES[k][1], bins))
            if region[0] >= SHAPE[0] and region[1] >= SHAPE[1]:           # one region: the whole-grid call's bits
                assert one.counts.shape == (1, 1, bins) and np.array_equal(one.counts[0, 0], whole[k].counts)
                assert (int(one.below[0, 0]), int(one.above[0, 0]), int(one.nan[0, 0])) == (whole[k].below, whole[k].above, whole[k].nan)
        for f in fields:
            f.destroy()
    sim.context.close()


# ---- one-valued data: lanes of different regions hold the same bin ---------------------------------------------------------------
@pytest.mark.parametrize("rw", [16, 20])
def test_one_valued_planes_fill_one_slot_per_region(built, rw):
    region, bins = (5, rw), 64
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    sizes = regions_ref.sizes(SHAPE, region).astype(np.uint64)
    for value, slot in ((np.float32(1.0), bins - 1), (np.float32(np.nan), bins + 2), (np.float32(-0.0), 0), (np.float32(7.0), bins + 1)):
        field = upload_all(ctx, [np.full(SHAPE, value, np.float32)])[0]
        c = region_hist_ref.counters_of(field.region_histogram(ctx, region, bins, (0.0, 1.0)))
        assert np.array_equal(c[:, :, slot], sizes), (value, slot)
        assert int(c.sum()) == SHAPE[0] * SHAPE[1], value
        field.destroy()
    # Species::new: U is 1 and V is 0 everywhere but in the seeded square
    species = sim.make_species(list(SHAPE))
    in_u, in_v, _, _ = species.in_out()
    u, v = in_u.make_scalar_view(ctx), in_v.make_scalar_view(ctx)
    hu, hv = species.region_histogram(region, bins)
    assert_counters(hu, region_hist_ref.by_label(u, region, 0.0, 1.0, bins), SHAPE, region, "Species::new U")
    assert_counters(hv, region_hist_ref.by_label(v, region, 0.0, 1.0, bins), SHAPE, region, "Species::new V")
    cu, cv = region_hist_ref.counters_of(hu), region_hist_ref.counters_of(hv)
    background = (cu[:, :, bins - 1] == sizes) & (cv[:, :, 0] == sizes)   # the regions off the square: their size in one slot each
    assert background.any() and not background.all()
    sim.context.close()


# ---- two row chunks in one region, and the region below begins in the middle of a chunk ------------------------------------------
def test_row_chunks_inside_a_region(built):
    shape, region, bins = (2 * T + 9, 80), (T + 5, 80), 256
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    plane = hist_ref.planted(shape, 0.0, 1.0, bins, 9)
    field = upload_all(sim.context, [plane])[0]
    got = field.region_histogram(sim.context, region, bins, (0.0, 1.0))
    assert got.counts.shape == (2, 1, bins)
    assert_counters(got, region_hist_ref.histograms(plane, region, 0.0, 1.0, bins), shape, region, f"{shape} {region}")
    sim.context.close()


def test_row_chunks_of_full_height(built):
    """A launch with as many tiles as workgroups it may use (8 per CU of 256) keeps tiles of T rows: 8 region rows x 2 chunks of
    T and 5 rows x 32 tiles of 3 regions side by side (4096 bins) x 4 planes = 2048 tiles."""
    shape, region, bins = (8 * (T + 5), 1536), (T + 5, 16), 4096
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    planes = [hist_ref.planted(shape, 0.0, 1.0, bins, 70 + k) for k in range(4)]
    got = region_histogram_fields(sim.context, upload_all(sim.context, planes), region, bins, [(0.0, 1.0)] * 4)
    for k in range(4):
        assert_counters(got[k], region_hist_ref.by_label(planes[k], region, 0.0, 1.0, bins), shape, region, f"{shape} {region} field {k}")
    sim.context.close()


# ---- a region wider than a tile, and wide regions whose last chunk is ragged -----------------------------------------------------
@pytest.mark.parametrize("shape,region", [((5, 2500), (3, 1500)), ((3, 2100), (3, 1028))])
def test_column_chunks_inside_a_region(built, shape, region):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    plane = hist_ref.planted(shape, -1.0, 1.0, 255, shape[1])
    field = upload_all(sim.context, [plane])[0]
    got = field.region_histogram(sim.context, region, 255, (-1.0, 1.0))
    assert_counters(got, region_hist_ref.by_label(plane, region, -1.0, 1.0, 255), shape, region, f"{shape} {region}")
    sim.context.close()


# ---- slab chains -------------------------------------------------------------------------------------------------------------
def chain_results(args, u0, v0, region, bins):
    sim = Simulation.new(Parameters(), args)
    species = species_from_arrays(sim, u0, v0)
    before = sim.context.stats()
    hu, hv = species.region_histogram(region, bins, (0.0, 1.0), (-0.125, 0.5))
    assert sim.context.stats() == before
    sim.context.close()
    return hu, hv


def test_slab_chains_give_the_same_bits(built):
    shape, bins = (96, 300), 256
    u0, v0 = stress_fields(shape, 21)
    v0[63:65, ::3] = np.float32(np.nan)
    for region, chains in (((16, 64), [HipArgs(devices=[0] * 2), HipArgs(devices=[0] * 3), HipArgs(devices=[0], split=2)]),
                           ((32, 320), [HipArgs(devices=[0] * 3), HipArgs(devices=[0], split=3)])):
        one = chain_results(HipArgs(devices=[0]), u0, v0, region, bins)
        assert_counters(one[0], region_hist_ref.by_label(u0, region, 0.0, 1.0, bins), shape, region, f"one slab {region} U")
        assert_counters(one[1], region_hist_ref.by_label(v0, region, -0.125, 0.5, bins), shape, region, f"one slab {region} V")
        for args in chains:
            for a, b in zip(one, chain_results(args, u0, v0, region, bins)):
                assert np.array_equal(region_hist_ref.counters_of(a), region_hist_ref.counters_of(b)), (region, args.devices, args.split)
    # two slabs: a seam at row 48, which is no multiple of 32 -- refused, and the context goes on working
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * 2))
    species = species_from_arrays(sim, u0, v0)
    with pytest.raises(capi.GsError) as e:
        species.region_histogram((32, 64))
    assert e.value.code == capi.GS_ERR_UNSUPPORTED
    _, hv = species.region_histogram((16, 64), 8)
    assert_counters(hv, region_hist_ref.by_label(v0, (16, 64), 0.0, 1.0, 8), shape, (16, 64), "after the refusal")
    sim.context.close()


# ---- no side effects -----------------------------------------------------------------------------------------------------------
def test_no_side_effects(built):
    shape = (64, 128)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = sim.make_species(list(shape))
    sim.perform_steps(species, 16)
    in_u, in_v, _, _ = species.in_out()
    planes = (in_u.make_scalar_view(sim.context).tobytes(), in_v.make_scalar_view(sim.context).tobytes())
    before = (sim.context.stats(), sim.context.info())
    species.region_histogram((16, 32), 64)
    assert (sim.context.stats(), sim.context.info()) == before
    in_u, in_v, _, _ = species.in_out()
    assert (in_u.make_scalar_view(sim.context).tobytes(), in_v.make_scalar_view(sim.context).tobytes()) == planes
    sim.context.close()


# ---- after real steps ----------------------------------------------------------------------------------------------------
def test_after_real_steps(built):
    shape, region, steps, bins = (64, 128), (16, 32), 200, 64
    rows, cols = shape
    feed = np.broadcast_to(np.linspace(0.01, 0.06, cols, dtype=np.float32), shape)
    kill = np.broadcast_to(np.linspace(0.04, 0.07, rows, dtype=np.float32)[:, None], shape)
    walls = np.zeros(shape, np.float32)
    walls[:, 40] = 1.0
    walls[30, :] = 1.0
    walls[30, 60:70] = 0.0
    rules = (capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_PERIODIC, capi.GS_BOUNDARY_NEUMANN)
    # every rule in the strict flavour, and the clipped rule in the fused one too
    for boundary, math in [(b, capi.GS_MATH_STRICT) for b in rules] + [(capi.GS_BOUNDARY_CLIPPED, capi.GS_MATH_FUSED)]:
        for attach in ("map", "mask"):
            sim = Simulation.new(Parameters(), HipArgs(devices=[0], boundary=boundary, math=math))
            species = sim.make_species(list(shape))
            if attach == "map":
                sim.set_param_map(feed, kill)
            else:
                sim.set_mask(walls)
            sim.perform_steps(species, steps)
            before = (sim.context.stats(), sim.context.info())
            hu, hv = species.region_histogram(region, bins, (0.0, 1.0), (0.0, 0.5))
            assert (sim.context.stats(), sim.context.info()) == before
            in_u, in_v, _, _ = species.in_out()
            u, v = in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)
            what = f"boundary {boundary}, math {math}, {attach}"             # (wall cells count)
            assert_counters(hu, region_hist_ref.by_label(u, region, 0.0, 1.0, bins), shape, region, what)
            assert_counters(hv, region_hist_ref.by_label(v, region, 0.0, 0.5, bins), shape, region, what)
            sim.context.close()


# ---- refusals that need handles, the result cap, the empty plane -------------------------------------------------------------
def test_refusals_that_need_handles_and_the_empty_plane(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    a, b = HipConcentration(sim.context, (8, 32)), HipConcentration(sim.context, (8, 33))
    foreign = HipConcentration(other.context, (8, 32))
    a.upload(sim.context, stress_fields((8, 32), 1)[0])
    for fields in ([a, b], [a, foreign], [a] * 5):
        with pytest.raises(capi.GsError) as e:
            region_histogram_fields(sim.context, fields, (4, 16), 8, [(0.0, 1.0)] * len(fields))
        assert e.value.code == capi.GS_ERR_INVALID, fields
    for region, bins, rng in (((4, 18), 8, (0.0, 1.0)), ((0, 16), 8, (0.0, 1.0)), ((4, 16), 0, (0.0, 1.0)), ((4, 16), 4097, (0.0, 1.0)),
                              ((4, 16), 8, (1.0, 1.0)), ((4, 16), 8, (float("nan"), 1.0)), ((4, 16), 8, (0.0, float("inf")))):
        with pytest.raises(capi.GsError) as e:
            a.region_histogram(sim.context, region, bins, rng)
        assert e.value.code == capi.GS_ERR_INVALID, (region, bins, rng)
    for shape in ((0, 16), (7, 0)):
        empty = HipConcentration(sim.context, shape)
        h = empty.region_histogram(sim.context, (4, 16), 8)
        assert h.counts.size == 0 and h.cells.size == 0
    for s in (sim, other):
        s.context.close()


def test_result_cap(built):
    """16 x 8066 regions stay under GS_REGIONS_MAX; with 4096 bins they are 4099 counters each, over GS_REGION_HIST_MAX = 2^25
    per field; with one bin they are 4 each and the call counts."""
    shape, region = (16, 16 * 8066), (1, 16)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    field = HipConcentration(sim.context, shape)
    plane = stress_fields(shape, 3)[0]
    field.upload(sim.context, plane)
    assert 16 * 8066 * 4099 > capi.GS_REGION_HIST_MAX >= 16 * 8066 * 4 and 16 * 8066 <= 1 << 22
    with pytest.raises(capi.GsError) as e:
        field.region_histogram(sim.context, region, 4096)
    assert e.value.code == capi.GS_ERR_INVALID and "counters" in e.value.message
    lo, hi = np.float32(0.25), np.float32(0.75)
    h = field.region_histogram(sim.context, region, 1, (0.25, 0.75))
    cells = plane.reshape(16, 8066, 16)
    assert h.counts.shape == (16, 8066, 1)
    assert np.array_equal(h.counts[:, :, 0], ((cells >= lo) & (cells <= hi)).sum(axis=2).astype(np.uint64))
    assert np.array_equal(h.below, (cells < lo).sum(axis=2).astype(np.uint64))
    assert np.array_equal(h.above, (cells > hi).sum(axis=2).astype(np.uint64))
    assert np.array_equal(h.nan, np.isnan(cells).sum(axis=2).astype(np.uint64))
    sim.context.close()


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_the_driver_records_the_histograms(built, tmp_path):
    base = [sys.executable, "-m", "grayscott_amd.simulate", "-r", "64", "-c", "128", "-n", "2", "-e", "16", "--hip-feed-map", "0.01:0.06",
            "--hip-kill-map", "0.04:0.07", "--hip-regions", "16x32", "--hip-regions-every", "1", "--hip-region-threshold-v", "0.25,0.1"]
    region = (16, 32)
    with_flag, without = tmp_path / "with.h5", tmp_path / "without.h5"
    r = run_program(base + ["--hip-region-hist-bins", "32", "--hip-region-hist-range-v=-0.125:0.5", "-o", str(with_flag)], cwd=ROOT)
    assert r.returncode == 0, r.stderr
    images = hdf5_min.read(str(with_flag))
    z = np.load(tmp_path / "with.regions.npz")
    assert int(z["hist_bins"]) == 32 and z["hist_range_u"].tolist() == [0.0, 1.0] and z["hist_range_v"].tolist() == [-0.125, 0.5]
    assert z["hist_u"].shape == z["hist_v"].shape == (2, 4, 4, 35) and z["hist_u"].dtype == z["hist_v"].dtype == np.uint64
    for k in range(2):                                                     # (the images are the V planes)
        assert np.array_equal(z["hist_v"][k], region_hist_ref.histograms(images[k], region, -0.125, 0.5, 32)), k
        assert np.array_equal(z["hist_u"][k].sum(axis=2).astype(np.int64), z["cells"]), k
    r = run_program(base + ["-o", str(without)], cwd=ROOT)
    assert r.returncode == 0, r.stderr
    old = np.load(tmp_path / "without.regions.npz")
    keys = {"region", "shape", "steps", "thresholds_v", "thresholds_u", "cells", "quads_v", "feed", "kill"}
    keys |= {f"{f}_{s}" for f in ("sum", "sum_sq", "min", "max", "nonfinite") for s in "uv"}
    assert set(old.files) == keys and set(z.files) == keys | {"hist_u", "hist_v", "hist_bins", "hist_range_u", "hist_range_v"}
    for key in keys:
        assert old[key].tobytes() == z[key].tobytes(), key
