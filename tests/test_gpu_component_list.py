"""Component lists on the device (gs_field_component_list, gs_members_component_list) against the scipy restatement of their
rule (tests/component_list_ref.py) on the same plane: every record equal, in the same order, everywhere."""
import os
import re

import numpy as np
import pytest

from grayscott_amd import ComponentList, HipArgs, HipConcentration, Parameters, Simulation, capi
from tests import component_list_ref as ref
from tests import components_ref
from tests import morph_ref
from tests.children import ROOT, build_program, run_program
from tests.helpers import species_from_arrays, stress_fields
from tests.observe_cases import seam_rows

pytestmark = pytest.mark.gpu

T = components_ref.TILE_ROWS  # the labelling's tile height (kCompTileRows)


def comp_words(c) -> np.ndarray:
    return np.concatenate([np.array([c.count, c.set_cells, c.largest], np.uint64), c.by_size])


def assert_records(got: ComponentList, want: np.ndarray, what: str):
    print(f"{what}: ({got.rows}, {got.cols}) t {got.threshold} above {got.above} connectivity {got.connectivity} "
          f"min_size {got.min_size}: {got.count} records, {want.shape[0]} wanted")
    assert got.records.dtype == ref.DTYPE
    assert np.array_equal(got.records, want), f"{what}: {got.records[:4]} ..., not {want[:4]} ..."


def at_least(full: np.ndarray, min_size: int) -> np.ndarray:
    return full[full["size"] >= np.uint64(min_size)]


def check_plane(ctx, field, plane, t, above, conn, what, min_sizes=(1, 2, 5), identities=True):
    """The lists of ``field`` (holding ``plane``) for every min_size and one more than the largest, against one reference;
    with min_size 1 the four identities with ``field.components``.  Returns the full list."""
    full = ref.records(plane, t, above, conn)
    largest = int(full["size"].max()) if full.shape[0] else 0
    for min_size in tuple(min_sizes) + (largest + 1,):
        got = field.component_list(ctx, t, above, conn, min_size)
        assert (got.rows, got.cols, got.above, got.connectivity, got.min_size) == plane.shape + (above, conn, min_size)
        assert got.threshold == float(np.float32(t))
        assert_records(got, at_least(full, min_size), f"{what}, min_size {min_size}")
        if min_size == largest + 1:
            assert got.count == 0
        if min_size == 1 and identities:
            c = field.components(ctx, [t], above, conn)[0]
            assert np.array_equal(ref.counters(got.records), comp_words(c)), what
            assert (got.count, int(got.sizes.sum()), int(got.sizes.max()) if got.count else 0) == (c.count, c.set_cells, c.largest)
    return full


# ---- planted planes ---------------------------------------------------------------------------------------------------

COLUMN_SHAPES = [(1, 1), (2, 3), (5, 253), (3, 255), (4, 256), (3, 257), (2, 1023), (6, 1025)]
ROW_SHAPES = [(T - 1, 300), (T, 300), (T + 1, 300), (2 * T + 1, 300)]


@pytest.mark.parametrize("shape", COLUMN_SHAPES + ROW_SHAPES)
def test_planted_planes(built, shape):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    thresholds = [0.3, -1.5, 0.0, 2.0 ** -130]            # distinct, one of them sub-normal
    field = HipConcentration(sim.context, shape)
    for above in (True, False):
        for i, density in enumerate((0.02, 0.5, 0.593, 0.98)):
            t = thresholds[i % 4]
            p = morph_ref.planted(shape, t, 10 * i + i % 4, density, above)
            field.upload(sim.context, p)
            for conn in (4, 8):
                check_plane(sim.context, field, p, t, above, conn, f"density {density}")
    sim.context.close()


def test_all_set_and_empty_planes(built):
    """The all-set plane is one component over many tiles and workgroups -- every wave's adds go to one record --, whose sums
    have closed forms."""
    shape = rows, cols = (2 * T + 1, 513)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    field = HipConcentration(sim.context, shape)
    field.upload(sim.context, np.ones(shape, np.float32))
    for conn in (4, 8):
        got = check_plane(sim.context, field, np.ones(shape, np.float32), 0.5, True, conn, "all set")
        want = np.array([(rows * cols, cols * rows * (rows - 1) // 2, rows * cols * (cols - 1) // 2, 0, 0, 0, rows - 1, 0, cols - 1)],
                        ref.DTYPE)
        assert np.array_equal(got, want)
        one = field.component_list(sim.context, 0.5, True, conn)
        assert np.array_equal(one.centroids(), [[(rows - 1) / 2, (cols - 1) / 2]]) and one.touches_edge().all()
        assert np.array_equal(one.boxes(), [[0, rows - 1, 0, cols - 1]]) and np.array_equal(one.first_cells(), [[0, 0]])
        none = field.component_list(sim.context, 0.5, False, conn)                     # nothing is below 0.5
        assert none.count == 0 and none.records.dtype == ref.DTYPE and none.centroids().shape == (0, 2)
        assert none.boxes().shape == (0, 4) and none.touches_edge().shape == (0,)
    field.upload(sim.context, np.zeros(shape, np.float32))
    for conn in (4, 8):
        check_plane(sim.context, field, np.zeros(shape, np.float32), 0.5, True, conn, "empty")
    for empty_shape in ((0, 16), (7, 0)):
        empty = HipConcentration(sim.context, empty_shape)
        assert empty.component_list(sim.context, 0.1).count == 0
    sim.context.close()


ADVERSARIAL = {"serpentine": components_ref.serpentine, "comb": components_ref.comb, "rings": components_ref.rings,
               "checkerboard": components_ref.checkerboard, "staircase": components_ref.staircase}


@pytest.mark.parametrize("shape", [(2 * T + 1, 300), (50, 513)])
@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
def test_adversarial_shapes(built, name, shape):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    field = HipConcentration(sim.context, shape)
    p = ADVERSARIAL[name](shape)
    field.upload(sim.context, p)
    full = {conn: check_plane(sim.context, field, p, 0.5, True, conn, name) for conn in (4, 8)}
    if name == "serpentine":
        assert full[4].shape == (1,) and int(full[4]["size"][0]) == int(p.sum()) and int(full[4]["row_max"][0]) == shape[0] - 1
    if name == "checkerboard":
        assert full[4].shape[0] == (shape[0] * shape[1] + 1) // 2 and full[8].shape == (1,)
    sim.context.close()


def test_nan_infinite_and_zero_cells(built):
    shape = (40, 300)
    _, v = stress_fields(shape, 7)
    rng = np.random.default_rng(8)
    for value in (np.nan, np.inf, -np.inf, 0.0, -0.0):
        v[rng.integers(0, shape[0], 300), rng.integers(0, shape[1], 300)] = np.float32(value)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    field = HipConcentration(sim.context, shape)
    field.upload(sim.context, v)
    inf = float("inf")
    for t, above in ((0.25, True), (0.25, False), (0.0, True), (-0.0, False), (0.0, False), (inf, True), (inf, False),
                     (-inf, True), (-inf, False), (3.4028235e38, False)):
        for conn in (4, 8):
            check_plane(sim.context, field, v, t, above, conn, f"t {t}", min_sizes=(1, 3))
    sim.context.close()


# ---- slab layouts -------------------------------------------------------------------------------------------------------

def layout_planes(shape, slabs):
    rows, cols = shape
    rng = np.random.default_rng(11)
    planted = (rng.random(shape) < 0.5).astype(np.float32)
    for seam in seam_rows(rows, slabs):
        for r in (seam - 1, seam):
            planted[r] = rng.random(cols) < 0.6
    out = {"serpentine": components_ref.serpentine(shape), "planted": planted, "column": components_ref.column(shape)}
    for seam in seam_rows(rows, slabs):
        out[f"u at {seam}"] = components_ref.u_shape(shape, seam)
    return out


@pytest.mark.parametrize("shape", [(5, 300), (7, 257), (2 * T + 1, 300), (50, 513)])
def test_lists_do_not_depend_on_the_slab_layout(built, shape):
    rows, cols = shape
    wanted = {}
    for slabs in (1, 2, 3, 5):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0] * slabs))
        field = HipConcentration(sim.context, shape)
        before = sim.context.stats()
        for what, p in layout_planes(shape, max(slabs, 2)).items():
            field.upload(sim.context, p)
            for conn in (4, 8):
                key = (what, p.tobytes(), conn)
                if key not in wanted:
                    wanted[key] = ref.records(p, 0.5, True, conn)
                full = wanted[key]
                # (the column: every slab's piece is smaller than min_size = rows, the merged component is not)
                for min_size in (1, 2, 5, rows):
                    got = field.component_list(sim.context, 0.5, True, conn, min_size)
                    assert_records(got, at_least(full, min_size), f"{what}, {slabs} slabs, connectivity {conn}, min_size {min_size}")
                if what == "column":
                    assert at_least(full, rows).shape == (1,) and int(full["row_max"][0]) == rows - 1
        assert sim.context.stats() == before
        sim.context.close()


# ---- ensembles -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("members,shape", [(1, (16, 32)), (5, (16, 32)), (5, (64, 128))])
def test_ensemble_members_equal_lone_species(built, members, shape):
    params = [Parameters(feed_rate=0.01 + 0.05 * i / members, kill_rate=0.05 + 0.015 * (members - 1 - i) / members)
              for i in range(members)]
    sim = Simulation.new(params[0], HipArgs(devices=[0]))
    ens = sim.make_ensemble(shape, params)
    rng = np.random.default_rng(1)
    ens.upload(rng.random((members,) + shape, dtype=np.float32),
               (rng.random((members,) + shape, dtype=np.float32) * np.float32(0.5)).astype(np.float32))
    ens.perform_steps(23)
    # member i's last row and member i + 1's first row fully set: they stay separate components; member 3 has no V above 0.25
    u, v = ens.u_views(), ens.result_views()
    for i in range(members):
        for j, r in ((i, shape[0] - 1), (i + 1, 0)):
            if j < members:
                u[j, r], v[j, r] = np.float32(0.0), np.float32(0.5)
    if members > 3:
        v[3] = np.float32(0.125)
    ens.upload(u, v)
    for conn, min_size in ((8, 1), (4, 1), (8, 3)):
        lists = ens.component_lists(connectivity=conn, min_size=min_size)
        assert len(lists) == members
        ulists = ens.component_lists(species="u", threshold=0.5, above=False, connectivity=conn, min_size=min_size)
        for i in range(members):
            assert_records(lists[i], ref.records(v[i], 0.25, True, conn, min_size), f"member {i} V")
            assert_records(ulists[i], ref.records(u[i], 0.5, False, conn, min_size), f"member {i} U")
            assert lists[i].count == 0 if i == 3 else int(lists[i].sizes.max()) >= shape[1]
            lone = Simulation.new(params[i], HipArgs(devices=[0]))
            species = species_from_arrays(lone, u[i], v[i])
            assert_records(species.component_list(0.25, "v", True, conn, min_size), lists[i].records, f"member {i} alone, V")
            assert_records(species.component_list(0.5, "u", False, conn, min_size), ulists[i].records, f"member {i} alone, U")
            lone.context.close()
        if min_size == 1:
            counters = ens.components(connectivity=conn)
            for i in range(members):
                assert np.array_equal(ref.counters(lists[i].records), counters[i, 1, 0])
                assert np.array_equal(ref.counters(ulists[i].records), counters[i, 0, 0])
        if members > 2:                                     # a range that does not start at 0, across the empty member
            part = ens.component_lists(2, members - 2, connectivity=conn, min_size=min_size)
            assert len(part) == members - 2
            for i, got in enumerate(part):
                assert_records(got, lists[2 + i].records, f"member {2 + i} of a range")
    ens.destroy()
    sim.context.close()


def test_a_retired_member_reports_its_held_state(built):
    members, shape = 5, (45, 61)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ens = sim.make_ensemble(shape, Parameters(), members=members)
    rng = np.random.default_rng(3)
    ens.upload(rng.random((members,) + shape, dtype=np.float32),
               (rng.random((members,) + shape, dtype=np.float32) * np.float32(0.5)).astype(np.float32))
    ens.perform_steps(7)
    held = ens.component_lists(threshold=0.1)
    ens.retire([1, 3])
    for steps in (3, 4):                     # an odd and an even number of further runs' steps: both slots are in play
        ens.perform_steps(steps)
        now = ens.component_lists(threshold=0.1)
        v = ens.result_views()
        for i in range(members):
            assert_records(now[i], ref.records(v[i], 0.1, True, 8), f"member {i} after {steps} more steps")
        for i in (1, 3):
            assert np.array_equal(now[i].records, held[i].records)
    ens.destroy()
    sim.context.close()


def test_more_members_than_one_batch(built):
    """One member more than fit GS_COMPONENTS_BATCH_BYTES of label memory (8 bytes per cell): the last member is a batch of
    its own, and the offsets run through."""
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    m = re.search(r"#define GS_COMPONENTS_BATCH_BYTES \((\d+)u << (\d+)\)", header)
    shape = (64, 128)
    batch = (int(m.group(1)) << int(m.group(2))) // 8 // (shape[0] * shape[1])
    members = batch + 1
    assert members * shape[0] * shape[1] * 16 < 2 ** 30, "four planes of the ensemble: a second's worth of memory traffic"
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ens = sim.make_ensemble(shape, Parameters(), members=members)
    rng = np.random.default_rng(5)
    v = (rng.random((members,) + shape, dtype=np.float32) < np.float32(0.3)).astype(np.float32)
    v[7] = 0                                                  # an empty member inside the first batch
    ens.upload(None, v)
    lists = ens.component_lists(threshold=0.5, min_size=4)
    assert len(lists) == members and lists[7].count == 0
    for i in (0, 7, 8, batch - 1, batch):
        assert_records(lists[i], ref.records(v[i], 0.5, True, 8, 4), f"member {i} of {members}")
    tail = ens.component_lists(batch - 1, 2, threshold=0.5, min_size=4)
    assert np.array_equal(tail[0].records, lists[batch - 1].records) and np.array_equal(tail[1].records, lists[batch].records)
    ens.destroy()
    sim.context.close()


# ---- after real kernels ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1080, 1920), (200, 333)])
def test_the_producer_does_not_matter(built, shape):
    """The threshold is the median of the V plane the marching kernel leaves (every producer leaves the same bits): half the
    cells are set, in blobs of the smoothed noise.  The reference is computed once."""
    u0, v0 = stress_fields(shape, 9)
    ran, results, threshold = [], {}, None
    for name, kernel in (("marching", capi.GS_KERNEL_TB), ("tile", capi.GS_KERNEL_TILE), ("window", capi.GS_KERNEL_WINDOW),
                         ("auto", capi.GS_KERNEL_AUTO)):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0], kernel=kernel))
        species = species_from_arrays(sim, u0, v0)
        try:
            sim.perform_steps(species, 64)
        except capi.GsError as e:                      # a kernel without a form for this grid
            assert e.code == capi.GS_ERR_UNSUPPORTED, e
            sim.context.close()
            continue
        ran.append(name)
        if threshold is None:                          # (marching comes first)
            v = species.make_result_view()
            threshold = float(np.median(v))
            want = {conn: ref.records(v, threshold, True, conn, 2) for conn in (8, 4)}
            assert want[8].shape[0] > 1 and 0 < int(want[8]["size"].sum()) < v.size, "a pattern, not a full or empty plane"
        got = {conn: species.component_list(threshold, "v", True, conn, 2) for conn in (8, 4)}
        if name == "marching":
            for conn in (8, 4):
                assert_records(got[conn], want[conn], f"{name} ({sim.context.info()[0]})")
        results[name] = got
        sim.context.close()
    assert {"marching", "auto"} <= set(ran), ran
    if shape == (1080, 1920):
        assert "window" in ran and "tile" in ran, ran
    for name in ran:
        for conn in (8, 4):
            assert np.array_equal(results[name][conn].records, results["marching"][conn].records), name


def test_after_the_resident_kernel(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = stress_fields((24, 60), 2)            # few enough cells for the kernel that keeps the grid in LDS
    species = species_from_arrays(sim, u0, v0)
    sim.perform_steps(species, 64)
    v = species.make_result_view()
    t = float(np.median(v))
    for conn in (8, 4):
        assert_records(species.component_list(t, connectivity=conn), ref.records(v, t, True, conn), sim.context.info()[0])
    sim.context.close()


@pytest.mark.parametrize("shape", [(1080, 1920), (200, 333)])
def test_lists_have_no_side_effects(built, shape):
    u0, v0 = stress_fields(shape, 5)
    planes, infos = [], []
    for look in (False, True):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
        species = species_from_arrays(sim, u0, v0)
        for _ in range(3):
            sim.prepare_steps(species, 40)
            if look:
                species.component_list()
                sim.context.sync()
                before = (sim.context.stats(), sim.context.info())
                species.component_list(0.1, connectivity=4, min_size=3)
                species.component_list(0.5, "u", above=False)
                assert (sim.context.stats(), sim.context.info()) == before
        sim.context.sync()
        infos.append((sim.context.stats(), sim.context.info()))
        in_u, in_v, _, _ = species.in_out()
        planes.append((in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)))
        sim.context.close()
    assert infos[0][1] == infos[1][1], infos                     # launches and the kernel's name
    for key in ("passes", "steps", "launches", "ghost_refreshes", "window_fallbacks"):
        assert infos[0][0][key] == infos[1][0][key], (key, infos)
    assert planes[0][0].tobytes() == planes[1][0].tobytes()
    assert planes[0][1].tobytes() == planes[1][1].tobytes()


# ---- refusals that need handles -----------------------------------------------------------------------------------------

def test_refusals_that_need_handles(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    a, foreign = HipConcentration(sim.context, (8, 16)), HipConcentration(other.context, (8, 16))
    with pytest.raises(capi.GsError) as e:
        foreign.component_list(sim.context, 0.5)
    assert e.value.code == capi.GS_ERR_INVALID and "another context" in e.value.message
    for kwargs in ({"threshold": float("nan")}, {"threshold": 0.5, "connectivity": 6}, {"threshold": 0.5, "min_size": 0}):
        with pytest.raises(capi.GsError) as e:
            a.component_list(sim.context, **kwargs)
        assert e.value.code == capi.GS_ERR_INVALID, kwargs
    ens = sim.make_ensemble((8, 16), Parameters(), members=3)
    for first, count in ((3, 1), (2, 2), (0, 4)):
        with pytest.raises(capi.GsError) as e:
            ens.component_lists(first, count)
        assert e.value.code == capi.GS_ERR_INVALID, (first, count)
    theirs = other.make_ensemble((8, 16), Parameters(), members=3)
    h = capi.ctypes.c_void_p()
    assert sim.context._lib.gs_members_component_list(sim.context.handle, theirs.handle, 0, 1, 1, 0.5, 1, 8, 1,
                                                      capi.ctypes.byref(h)) == capi.GS_ERR_INVALID and not h
    with pytest.raises(ValueError):
        ens.component_lists(species="w")
    for s in (sim, other):
        s.context.close()


# ---- the sweep driver ------------------------------------------------------------------------------------------------------

def test_sweep_records_spots_without_changing_the_fields(built, tmp_path):
    from grayscott_amd import hdf5_min, sweep

    base = ["--feed", "0.02:0.05:3", "--kill", "0.05:0.062:2", "-r", "48", "-c", "72", "-s", "30"]
    sweep.main(base + ["-o", str(tmp_path / "plain.h5")])
    sweep.main(base + ["--spots-every", "10", "--spot-threshold-v", "0.1", "--spot-min-size", "2", "--spot-connectivity", "4",
                       "-o", str(tmp_path / "spots.h5")])
    sweep.main(base + ["--spots-every", "30", "--spot-threshold-v", "0.1", "--spot-min-size", "2", "--spot-connectivity", "4",
                       "--no-fields", "-o", str(tmp_path / "nof.h5")])
    assert (tmp_path / "plain.h5").read_bytes() == (tmp_path / "spots.h5").read_bytes()
    assert not (tmp_path / "plain.spots.npz").exists() and not (tmp_path / "nof.h5").exists()
    z = np.load(tmp_path / "spots.spots.npz")
    assert list(z["steps"]) == [10, 20, 30] and int(z["connectivity"]) == 4 and int(z["min_size"]) == 2
    assert float(z["threshold"]) == float(np.float32(0.1))
    assert z["offsets"].shape == (3 * 6 + 1,) and z["records"].dtype == ref.DTYPE and int(z["offsets"][-1]) == z["records"].shape[0]
    v = hdf5_min.read(str(tmp_path / "spots.h5"))
    found = 0
    for i in range(6):
        want = ref.records(v[i], 0.1, True, 4, 2)
        assert np.array_equal(z["records"][z["offsets"][12 + i]:z["offsets"][12 + i + 1]], want), i
        found += want.shape[0]
    assert found > 0, "a sweep with no spot to list checks nothing"
    z2 = np.load(tmp_path / "nof.spots.npz")
    assert list(z2["steps"]) == [30] and np.array_equal(z2["records"], z["records"][z["offsets"][12]:])


def test_cpp_mirror_component_lists(built, tmp_path):
    exe = build_program("component_list_mirror", tmp_path)
    members, rows, cols = 4, 72, 200
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(members), str(rows), str(cols), "31", str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    lists, at = [], 0
    for _ in range(3 + members):
        n = int(np.frombuffer(raw, np.uint64, 1, at)[0])
        lists.append(np.frombuffer(raw, ref.DTYPE, n, at + 8))
        at += 8 + 48 * n
    planes = np.frombuffer(raw[at:], np.float32).reshape(2, rows, cols)
    assert np.array_equal(lists[0], ref.records(planes[1], 0.25, True, 8))
    assert np.array_equal(lists[1], ref.records(planes[1], 0.1, True, 4, 3)) and lists[1].shape[0] > 0
    assert np.array_equal(lists[2], ref.records(planes[0], 0.5, False, 8))
    for i in range(members):
        assert np.array_equal(lists[3 + i], lists[0]), i
