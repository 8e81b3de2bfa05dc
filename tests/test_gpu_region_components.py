"""Regional connected components on the device (gs_fields_region_components) against their definition
(tests/region_components_ref.py): every region's counters are those of the whole-grid rule on that region's cells alone -- a
region's border is a wall.  Everything is exact integer equality."""
import functools
import sys

import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, RegionComponents, Simulation, capi, hdf5_min
from grayscott_amd.simulation import components_fields, region_components_fields
from tests import observe_cases, region_components_ref, regions_ref
from tests.children import ROOT, run_program
from tests.helpers import species_from_arrays, stress_fields

pytestmark = pytest.mark.gpu

SHAPE = (37, 532)              # three tile rows and three tile columns of 16 x 256, both ragged
# borders inside tiles with ragged last regions (5, 20), borders on the tile borders (16, 256), (7, 64), (16, 16), and one
# region over the whole plane (64, 1024): gs_fields_components' own result
REGIONS = [(5, 20), (16, 256), (7, 64), (16, 16), (64, 1024)]
T0 = 0.25
THRESHOLDS = [T0, 0.3, -1.5, 2.0 ** -130]      # distinct, one of them sub-normal; the planes are made around the first
KINDS = [("full", 0.5), ("checkerboard", 0.5), ("serpentine", 0.5), ("comb", 0.5), ("rings", 0.5), ("lane_runs", 0.5),
         ("planted", 0.3), ("planted", 0.593), ("empty", 0.5)]


@functools.lru_cache(maxsize=None)
def plane_of(kind, density, above, shape=SHAPE):
    """NaN and equal-to-threshold cells, sub-normals and infinities are sprinkled in (observe_cases.values_of,
    morph_ref.planted); full and empty planes stay what they are called."""
    a = observe_cases.plane(kind, shape, T0, above, 11 + len(kind) + int(100 * density), density)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(kind, density, above, region, t, connectivity, shape=SHAPE):
    return region_components_ref.counters(plane_of(kind, density, above, shape), region, t, above, connectivity)


def assert_counters(got: RegionComponents, wanted, shape, region, what):
    c = got.counters()
    assert c.dtype == np.uint64 and c.shape == wanted.shape == regions_ref.grid(shape, region) + (35,), what
    assert got.region == regions_ref.shape_of(region) and got.shape == tuple(shape), what
    bad = np.argwhere(c != wanted)
    assert bad.size == 0, (f"{what}: t {got.threshold} above {got.above} connectivity {got.connectivity}: {len(bad)} counters "
                           f"differ, first (i, j, word) = {tuple(bad[0])}: {int(c[tuple(bad[0])])}, not {int(wanted[tuple(bad[0])])}")
    assert np.array_equal(got.by_size.sum(axis=2), got.count), what


def upload_all(ctx, planes):
    fields = []
    for p in planes:
        f = HipConcentration(ctx, p.shape)
        f.upload(ctx, np.array(p))
        fields.append(f)
    return fields


# ---- the lattice: every kind of plane under every region shape, both connectivities, both senses ------------------------------
@pytest.mark.parametrize("kind,density", KINDS)
def test_lattice_cases(built, kind, density):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    for above in (True, False):
        plane = plane_of(kind, density, above)
        field = upload_all(ctx, [plane])[0]
        for connectivity in (8, 4):
            whole = components_fields(ctx, [field], [[T0]], [above], connectivity)[0][0]
            for region in REGIONS:
                what = f"{kind} {density} above {above} connectivity {connectivity} region {region}"
                one = field.region_components(ctx, region, [T0], above, connectivity)
                assert len(one) == 1 and one[0].threshold == T0 and one[0].above == above and one[0].connectivity == connectivity
                wanted = want(kind, density, above, region, T0, connectivity)
                assert_counters(one[0], wanted, SHAPE, region, what)
                # the invariants, against the device's own whole-grid call and against the restatement's
                c = region_components_ref.invariants(plane, region, T0, above, connectivity, one[0].counters())
                assert int(c[..., 1].sum()) == whole.set_cells and int(c[..., 0].sum()) >= whole.count, what
                if region == (64, 1024):
                    assert c.shape == (1, 1, 35) and (int(c[0, 0, 0]), int(c[0, 0, 1]), int(c[0, 0, 2])) == (whole.count, whole.set_cells, whole.largest)
                    assert np.array_equal(c[0, 0, 3:], whole.by_size), what
                if kind == "full":                                         # any leak across a wall joins two regions
                    sizes = regions_ref.sizes(SHAPE, region).astype(np.uint64)
                    assert np.array_equal(c[..., 0], np.ones_like(sizes)) and np.array_equal(c[..., 2], sizes), what
                if kind == "empty":
                    assert not c.any(), what
            # four thresholds in one call equal four calls of one: borders inside tiles, borders on tile borders
            for region in REGIONS[:2]:
                four = field.region_components(ctx, region, THRESHOLDS, above, connectivity)
                assert [x.threshold for x in four] == [float(np.float32(t)) for t in THRESHOLDS]
                for k, t in enumerate(THRESHOLDS):
                    assert_counters(four[k], want(kind, density, above, region, t, connectivity), SHAPE, region,
                                    f"{kind} {density} above {above} connectivity {connectivity} region {region} nt 4 [{k}]")
        field.destroy()
    sim.context.close()


def test_a_checkerboard_leaks_through_no_corner(built):
    """Under 8-connectivity a checkerboard is one component of the grid and one per region: a union across a corner of four
    regions, or into the first column of the region to the right, would join two of them."""
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    plane = observe_cases.plane("checkerboard", SHAPE, T0, True, 1, special=False)
    field = upload_all(sim.context, [plane])[0]
    assert field.components(sim.context, [T0], True, 8)[0].count == 1
    for region in REGIONS:
        c = field.region_components(sim.context, region, [T0], True, 8)[0]
        sizes = regions_ref.sizes(SHAPE, region)
        assert np.array_equal(c.count, np.ones_like(c.count)), region
        assert np.array_equal(c.largest.astype(np.int64), c.set_cells.astype(np.int64)) and abs(int(c.set_cells.sum()) * 2 - SHAPE[0] * SHAPE[1]) <= 1
        assert np.all(np.abs(c.set_cells.astype(np.int64) * 2 - sizes) <= 1), region
        four = field.region_components(sim.context, region, [T0], True, 4)[0]
        assert np.array_equal(four.count, four.set_cells) and np.array_equal(four.set_cells, c.set_cells), region
    sim.context.close()


# ---- 1 to 4 planes in a call, each with its own thresholds and sense ------------------------------------------------------------
def test_field_lists(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    cases = [("planted", 0.593, True), ("lane_runs", 0.5, False), ("planted", 0.3, False), ("rings", 0.5, True)]
    fields = upload_all(ctx, [plane_of(*c) for c in cases])
    region = (5, 20)
    for n in (1, 2, 3, 4):
        got = region_components_fields(ctx, fields[:n], region, [[T0, 0.3]] * n, [c[2] for c in cases[:n]], 4)
        assert len(got) == n and all(len(g) == 2 for g in got)
        for p in range(n):
            for k, t in enumerate((T0, 0.3)):
                assert_counters(got[p][k], want(*cases[p], region, t, 4), SHAPE, region, f"field {p} of {n}, threshold {k}")
    sim.context.close()


# ---- a pitch that is no multiple of 64 and a column count that is no multiple of 4 -------------------------------------------------
def test_padded_pitch_and_ragged_columns(built):
    """A field's rows always begin on 16 bytes (the library rounds a pitch pad up to a multiple of 4), so this is as far from
    the aligned layout as a field gets: a pitch of 64 k + 4 floats and 533 columns, the last lane of a row one column wide."""
    shape = (37, 533)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], pitch_pad=3))
    for kind, density, above in (("planted", 0.593, True), ("lane_runs", 0.5, False), ("full", 0.5, True)):
        plane = plane_of(kind, density, above, shape)
        field = upload_all(sim.context, [plane])[0]
        for region, connectivity in (((5, 20), 8), ((16, 256), 4), ((7, 64), 8)):
            got = field.region_components(sim.context, region, [T0], above, connectivity)[0]
            assert_counters(got, want(kind, density, above, region, T0, connectivity, shape), shape, region, f"{kind} {region}")
    sim.context.close()


# ---- slab chains -------------------------------------------------------------------------------------------------------------
def chain_results(args, u0, v0, region, connectivity):
    sim = Simulation.new(Parameters(), args)
    species = species_from_arrays(sim, u0, v0)
    before = sim.context.stats()
    cu, cv = species.region_components(region, (0.25, 0.1), (0.5, 0.8), connectivity=connectivity)
    assert sim.context.stats() == before
    sim.context.close()
    return cu + cv


def test_slab_chains_give_the_same_bits(built):
    shape = (96, 300)
    u0, v0 = stress_fields(shape, 21)
    v0[63:65, ::3] = np.float32(np.nan)
    for region, connectivity, chains in (((16, 64), 8, [HipArgs(devices=[0] * 2), HipArgs(devices=[0] * 3), HipArgs(devices=[0], split=2)]),
                                         ((32, 320), 4, [HipArgs(devices=[0] * 3), HipArgs(devices=[0], split=3)])):
        one = chain_results(HipArgs(devices=[0]), u0, v0, region, connectivity)
        for k, (tu, tv) in enumerate(((0.5, 0.25), (0.8, 0.1))):
            assert_counters(one[k], region_components_ref.counters(u0, region, tu, False, connectivity), shape, region, f"one slab {region} U[{k}]")
            assert_counters(one[2 + k], region_components_ref.counters(v0, region, tv, True, connectivity), shape, region, f"one slab {region} V[{k}]")
        for args in chains:
            for a, b in zip(one, chain_results(args, u0, v0, region, connectivity)):
                assert np.array_equal(a.counters(), b.counters()), (region, args.devices, args.split)
    # two slabs: a seam at row 48, which is no multiple of 32 -- refused, and the context goes on working
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * 2))
    species = species_from_arrays(sim, u0, v0)
    with pytest.raises(capi.GsError) as e:
        species.region_components((32, 64))
    assert e.value.code == capi.GS_ERR_UNSUPPORTED
    _, cv = species.region_components((16, 64), (0.25,))
    assert_counters(cv[0], region_components_ref.counters(v0, (16, 64), 0.25, True, 8), shape, (16, 64), "after the refusal")
    sim.context.close()


# ---- no side effects; a second call returns the same bytes ----------------------------------------------------------------------
def test_no_side_effects_and_nothing_left_in_label_memory(built):
    shape = (64, 128)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = sim.make_species(list(shape))
    sim.perform_steps(species, 16)
    in_u, in_v, _, _ = species.in_out()
    planes = (in_u.make_scalar_view(sim.context).tobytes(), in_v.make_scalar_view(sim.context).tobytes())
    before = (sim.context.stats(), sim.context.info())
    first = species.region_components((16, 32), (0.25, 0.1, 0.05, 0.4), (0.5, 0.8, 0.3, 0.95))
    assert (sim.context.stats(), sim.context.info()) == before
    in_u, in_v, _, _ = species.in_out()
    assert (in_u.make_scalar_view(sim.context).tobytes(), in_v.make_scalar_view(sim.context).tobytes()) == planes
    # every (plane, threshold) is labelled in the same memory: a second call, and one in the reverse order of thresholds
    second = species.region_components((16, 32), (0.25, 0.1, 0.05, 0.4), (0.5, 0.8, 0.3, 0.95))
    turned = species.region_components((16, 32), (0.4, 0.05, 0.1, 0.25), (0.95, 0.3, 0.8, 0.5))
    for s in range(2):
        for k in range(4):
            assert first[s][k].counters().tobytes() == second[s][k].counters().tobytes(), (s, k)
            assert first[s][k].counters().tobytes() == turned[s][3 - k].counters().tobytes(), (s, k)
    # a following run is what it is without the calls
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    twin = other.make_species(list(shape))
    other.perform_steps(twin, 32)
    sim.perform_steps(species, 16)
    for mine, theirs in zip(species.in_out()[:2], twin.in_out()[:2]):
        assert mine.make_scalar_view(sim.context).tobytes() == theirs.make_scalar_view(other.context).tobytes()
    for s in (sim, other):
        s.context.close()


# ---- after real steps ----------------------------------------------------------------------------------------------------
def test_after_real_steps(built):
    shape, region, steps = (64, 128), (16, 32), 200
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
            connectivity = 8 if attach == "map" else 4
            cu, cv = species.region_components(region, (0.25, 0.1), (0.5, 0.8), connectivity=connectivity)
            assert (sim.context.stats(), sim.context.info()) == before
            in_u, in_v, _, _ = species.in_out()
            u, v = in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)
            what = f"boundary {boundary}, math {math}, {attach}"             # (wall cells count; components never wrap)
            for k, (tu, tv) in enumerate(((0.5, 0.25), (0.8, 0.1))):
                assert_counters(cu[k], region_components_ref.counters(u, region, tu, False, connectivity), shape, region, what)
                assert_counters(cv[k], region_components_ref.counters(v, region, tv, True, connectivity), shape, region, what)
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
            region_components_fields(sim.context, fields, (4, 16), [[0.25]] * len(fields), [True] * len(fields), 8)
        assert e.value.code == capi.GS_ERR_INVALID, fields
    for region, thresholds, connectivity in (((4, 18), [0.25], 8), ((0, 16), [0.25], 8), ((4, 16), [], 8), ((4, 16), [0.1] * 5, 8),
                                             ((4, 16), [float("nan")], 8), ((4, 16), [0.25], 6), ((4, 16), [0.25], 0)):
        with pytest.raises(capi.GsError) as e:
            a.region_components(sim.context, region, thresholds, True, connectivity)
        assert e.value.code == capi.GS_ERR_INVALID, (region, thresholds, connectivity)
    for shape in ((0, 16), (7, 0)):
        empty = HipConcentration(sim.context, shape)
        c = empty.region_components(sim.context, (4, 16), [0.25])[0]
        assert c.count.size == 0 and c.by_size.size == 0
    for s in (sim, other):
        s.context.close()


def test_result_cap(built):
    """32 x 9400 regions stay under GS_REGIONS_MAX; with four thresholds they are four results each, 32 x 9400 x 4 being over
    GS_REGION_COMPONENTS_MAX = 2^20 per field; with three they would fit, and with one the call counts (a region is 16 cells of
    one row: its components are its runs)."""
    shape, region = (32, 16 * 9400), (1, 16)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    field = HipConcentration(sim.context, shape)
    plane = stress_fields(shape, 3)[0]
    field.upload(sim.context, plane)
    assert 32 * 9400 * 4 > capi.GS_REGION_COMPONENTS_MAX >= 32 * 9400 * 3 and 32 * 9400 <= 1 << 22
    with pytest.raises(capi.GsError) as e:
        field.region_components(sim.context, region, [0.2, 0.4, 0.6, 0.8])
    assert e.value.code == capi.GS_ERR_INVALID and "results" in e.value.message
    c = field.region_components(sim.context, region, [0.5], True, 4)[0]
    bits = plane.reshape(32, 9400, 16) > np.float32(0.5)
    runs = bits[..., 0].astype(np.uint64) + (bits[..., 1:] & ~bits[..., :-1]).sum(axis=2).astype(np.uint64)
    assert c.count.shape == (32, 9400) and c.count.sum() > 32 * 9400 // 4
    assert np.array_equal(c.set_cells, bits.sum(axis=2).astype(np.uint64)) and np.array_equal(c.count, runs)
    sim.context.close()


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_the_driver_records_the_components(built, tmp_path):
    base = [sys.executable, "-m", "grayscott_amd.simulate", "-r", "64", "-c", "128", "-n", "2", "-e", "16", "--hip-feed-map", "0.01:0.06",
            "--hip-kill-map", "0.04:0.07", "--hip-regions", "16x32", "--hip-regions-every", "1", "--hip-region-threshold-v", "0.25,0.1"]
    region = (16, 32)
    with_flag, without = tmp_path / "with.h5", tmp_path / "without.h5"
    r = run_program(base + ["--hip-region-components", "4", "-o", str(with_flag)], cwd=ROOT)
    assert r.returncode == 0, r.stderr
    images = hdf5_min.read(str(with_flag))
    z = np.load(tmp_path / "with.regions.npz")
    assert int(z["comp_connectivity"]) == 4
    assert z["components_v"].shape == (2, 2, 4, 4, 35) and z["components_v"].dtype == np.uint64
    for k in range(2):                                                     # (the images are the V planes)
        for j, t in enumerate((0.25, 0.1)):
            assert np.array_equal(z["components_v"][k, j], region_components_ref.counters(images[k], region, t, True, 4)), (k, j)
    assert z["components_v"][..., 0].sum() > 0
    r = run_program(base + ["-o", str(without)], cwd=ROOT)
    assert r.returncode == 0, r.stderr
    old = np.load(tmp_path / "without.regions.npz")
    keys = {"region", "shape", "steps", "thresholds_v", "thresholds_u", "cells", "quads_v", "feed", "kill"}
    keys |= {f"{f}_{s}" for f in ("sum", "sum_sq", "min", "max", "nonfinite") for s in "uv"}
    assert set(old.files) == keys and set(z.files) == keys | {"components_v", "comp_connectivity"}
    for key in keys:
        assert old[key].tobytes() == z[key].tobytes(), key
