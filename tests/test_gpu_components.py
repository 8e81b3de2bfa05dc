"""Connected components on the device (gs_fields_components, gs_members_components) against the union-find restatement of
their rule (tests/components_ref.py) on the same plane: every counter equal, everywhere."""
import numpy as np
import pytest

from grayscott_amd import Components, HipArgs, HipConcentration, Parameters, Simulation, capi
from grayscott_amd.simulation import components_fields
from tests import components_ref as ref
from tests import morph_ref
from tests.children import build_program, run_program
from tests.helpers import species_from_arrays, stress_fields
from tests.observe_cases import seam_rows

pytestmark = pytest.mark.gpu

T = ref.TILE_ROWS  # the kernel's tile height (kCompTileRows), restated in tests/components_ref.py
TV, TU = (0.25, 0.1, 0.05, 0.4), (0.5, 0.8, 0.3, 0.95)   # V is set above its thresholds, U below


def words(c: Components) -> np.ndarray:
    return np.concatenate([np.array([c.count, c.set_cells, c.largest], np.uint64), c.by_size])


def assert_same(c: Components, plane: np.ndarray, what: str):
    want = ref.counters(plane, c.threshold, c.above, c.connectivity)
    got = words(c)
    print(f"{what}: {plane.shape} t {c.threshold} above {c.above} connectivity {c.connectivity}: components {c.count} "
          f"set {c.set_cells} largest {c.largest}")
    assert c.by_size.dtype == np.uint64 and c.by_size.shape == (32,)
    assert np.array_equal(got, want), f"{what}: {list(map(int, got))}, not {list(map(int, want))}"
    assert int(c.by_size.sum()) == c.count


def check_species(species, nt=4, what="", connectivities=(8, 4)):
    in_u, in_v, _, _ = species.in_out()
    ctx = species.context()
    u, v = in_u.make_scalar_view(ctx), in_v.make_scalar_view(ctx)
    out = []
    for conn in connectivities:
        cu, cv = species.components(TV[:nt], TU[:nt], connectivity=conn)
        assert len(cu) == nt and len(cv) == nt
        for k in range(nt):
            assert (cu[k].above, cv[k].above) == (False, True)
            assert_same(cu[k], u, f"{what} U[{k}]")
            assert_same(cv[k], v, f"{what} V[{k}]")
        out.append(np.stack([words(c) for c in cu + cv]))
    return np.stack(out)


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
            k = i % 4
            p = morph_ref.planted(shape, thresholds[k], 10 * i + k, density, above)
            field.upload(sim.context, p)
            for conn in (4, 8):
                four = field.components(sim.context, thresholds, above, conn)        # nt = 4 in one call
                assert [c.threshold for c in four] == [float(np.float32(x)) for x in thresholds]
                for c in four:
                    assert_same(c, p, f"density {density}, nt 4")
                one = field.components(sim.context, [thresholds[k]], above, conn)   # ... equals a call with nt = 1
                assert len(one) == 1 and np.array_equal(words(one[0]), words(four[k]))
    # 1 to 4 planes in a call, each with its own thresholds and sense
    planes = [morph_ref.planted(shape, thresholds[k], 40 + k, 0.5, k % 2 == 0) for k in range(4)]
    fields = []
    for p in planes:
        f = HipConcentration(sim.context, shape)
        f.upload(sim.context, p)
        fields.append(f)
    for n in (1, 2, 3, 4):
        got = components_fields(sim.context, fields[:n], [[thresholds[k], 0.7] for k in range(n)], [k % 2 == 0 for k in range(n)], 4)
        assert len(got) == n
        for k in range(n):
            assert_same(got[k][0], planes[k], f"field {k} of {n}")
            assert_same(got[k][1], planes[k], f"field {k} of {n}, second threshold")
    sim.context.close()


ADVERSARIAL = {"serpentine": ref.serpentine, "comb": ref.comb, "rings": ref.rings, "checkerboard": ref.checkerboard,
               "staircase": ref.staircase, "full": lambda s: np.ones(s, np.float32), "empty": lambda s: np.zeros(s, np.float32)}


@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
def test_adversarial_shapes(built, name):
    shape = (200, 333)
    rows, cols = shape
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    field = HipConcentration(sim.context, shape)
    p = ADVERSARIAL[name](shape)
    field.upload(sim.context, p)
    got = {}
    for conn in (4, 8):
        got[conn] = field.components(sim.context, [0.5], True, conn)[0]
        assert_same(got[conn], p, f"{name}")
    four, eight = got[4], got[8]
    if name == "serpentine":
        assert four.count == 1 and eight.count == 1 and four.largest == four.set_cells == int(p.sum())
    if name == "checkerboard":
        assert four.count == (rows * cols + 1) // 2 and int(four.by_size[0]) == four.count and four.largest == 1
        assert eight.count == 1 and eight.largest == four.count
    if name == "staircase":
        assert eight.count == 1 and eight.largest == 200 and four.count == 200 and four.largest == 1
    if name == "full":
        assert four.count == 1 and four.largest == rows * cols and int(four.by_size[16]) == 1
    if name == "empty":
        assert not words(four).any() and not words(eight).any()
    if name == "rings":
        assert four.count == 50 and eight.count == 50                  # every other ring of 100
    sim.context.close()


def test_infinite_thresholds_and_nan_cells(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    shape = (T + 3, 259)
    u0, v0 = morph_ref.planted(shape, 0.5, 3, 0.5, False), morph_ref.planted(shape, 0.25, 4)
    species = species_from_arrays(sim, u0, v0)
    in_u, in_v, _, _ = species.in_out()
    inf = float("inf")
    for t, above in ((-inf, True), (inf, True), (inf, False), (-inf, False), (3.4028235e38, False)):
        for conn in (4, 8):
            assert_same(in_v.components(sim.context, [t], above, conn)[0], v0, f"t {t}")
    cu, cv = species.components(TV, TU)
    mu, mv = species.morphology(TV, TU)
    for k in range(4):
        assert cu[k].set_cells == mu[k].area and cv[k].set_cells == mv[k].area
        assert cu[k].holes(mu[k]) >= 0 and cv[k].holes(mv[k]) >= 0
    sim.context.close()


def test_refusals_that_need_handles_and_the_empty_plane(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    a, b = HipConcentration(sim.context, (8, 16)), HipConcentration(sim.context, (8, 17))
    foreign = HipConcentration(other.context, (8, 16))
    for fields in ([a, b], [a, foreign], [a] * 5):
        with pytest.raises(capi.GsError) as e:
            components_fields(sim.context, fields, [[0.5]] * len(fields), [True] * len(fields))
        assert e.value.code == capi.GS_ERR_INVALID, fields
    for thresholds, conn in (([], 8), ([0.1] * 5, 8), ([float("nan")], 8), ([0.1], 6), ([0.1], 0)):
        with pytest.raises(capi.GsError) as e:
            a.components(sim.context, thresholds, True, conn)
        assert e.value.code == capi.GS_ERR_INVALID, (thresholds, conn)
    ens = sim.make_ensemble((8, 16), Parameters(), members=3)
    for first, count in ((3, 1), (2, 2), (0, 4)):
        with pytest.raises(capi.GsError) as e:
            ens.components(first, count)
        assert e.value.code == capi.GS_ERR_INVALID, (first, count)
    for shape in ((0, 16), (7, 0)):
        empty = HipConcentration(sim.context, shape)
        for c in empty.components(sim.context, [0.1, 0.2]):
            assert not words(c).any()
    for s in (sim, other):
        s.context.close()


# ---- after real kernels ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1080, 1920), (200, 333)])
def test_the_producer_does_not_matter(built, shape):
    """The thresholds are the medians of the planes the marching kernel leaves (every producer leaves the same bits): half
    the cells are set, in blobs of the smoothed noise -- neither an empty nor a full plane.  The reference is computed once."""
    u0, v0 = stress_fields(shape, 9)
    ran, results, thresholds = [], {}, None
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
        in_u, in_v, _, _ = species.in_out()
        if thresholds is None:                         # (marching comes first)
            u, v = in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)
            thresholds = (float(np.median(u)), float(np.median(v)))
        got = []
        for conn in (8, 4):
            cu, cv = species.components([thresholds[1]], [thresholds[0]], connectivity=conn)
            if name == "marching":
                assert_same(cu[0], u, f"{name} ({sim.context.info()[0]}) U")
                assert_same(cv[0], v, f"{name} ({sim.context.info()[0]}) V")
                assert cu[0].count > 1 and cv[0].count > 1 and 0 < cv[0].set_cells < v.size, "a pattern, not a full or empty plane"
            got.append(np.stack([words(cu[0]), words(cv[0])]))
        results[name] = np.stack(got)
        sim.context.close()
    assert {"marching", "auto"} <= set(ran), ran
    if shape == (1080, 1920):
        assert "window" in ran and "tile" in ran, ran
    for name in ran:                                   # (every producer computes the same bits)
        assert np.array_equal(results[name], results["marching"]), name


def test_after_the_resident_kernel(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = stress_fields((24, 60), 2)            # few enough cells for the kernel that keeps the grid in LDS
    species = species_from_arrays(sim, u0, v0)
    sim.perform_steps(species, 64)
    check_species(species, what=sim.context.info()[0])
    sim.context.close()


@pytest.mark.parametrize("shape", [(1080, 1920), (200, 333)])
def test_components_have_no_side_effects(built, shape):
    u0, v0 = stress_fields(shape, 5)
    planes, infos = [], []
    for look in (False, True):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
        species = species_from_arrays(sim, u0, v0)
        for _ in range(3):
            sim.prepare_steps(species, 40)
            if look:
                species.components()
                sim.context.sync()
                before = (sim.context.stats(), sim.context.info())
                species.components(TV[:2], TU[:2], connectivity=4)
                species.u.in_out()[0].components(sim.context, [0.5], above=False)
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


# ---- slab layout --------------------------------------------------------------------------------------------------------

def layout_planes(shape, slabs):
    """(U, V) pairs: V set above 0.25 carries the pattern, U set below 0.5 carries it too (U = 1 - pattern)."""
    rows, cols = shape
    rng = np.random.default_rng(11)
    planted = (rng.random(shape) < 0.5).astype(np.float32)
    for seam in seam_rows(rows, slabs):
        for r in (seam - 1, seam):
            planted[r] = rng.random(cols) < 0.6
    patterns = {"serpentine": ref.serpentine(shape), "column": ref.column(shape), "planted": planted,
                "u": ref.u_shape(shape, seam_rows(rows, slabs)[0])}
    return {k: ((1 - p).astype(np.float32), (p * np.float32(0.5)).astype(np.float32)) for k, p in patterns.items()}


@pytest.mark.parametrize("shape,slabs", [((50, 333), 3), ((9, 256), 2), ((5, 70), 4)])   # (the last: one-row slabs)
def test_components_do_not_depend_on_the_slab_layout(built, shape, slabs):
    for what, (u0, v0) in layout_planes(shape, slabs).items():
        got = {}
        for name, devices in (("one", [0]), ("many", [0] * slabs)):
            sim = Simulation.new(Parameters(), HipArgs(devices=devices))
            species = species_from_arrays(sim, u0, v0)
            before = sim.context.stats()
            fresh = check_species(species, nt=1, what=f"{what}, {name}: right after upload")       # ghost rows stale
            assert sim.context.stats() == before
            later = fresh
            if shape[0] >= 4 * slabs:                 # (one-row slabs are observed as uploaded: too short to step)
                sim.perform_steps(species, 5)
                before = sim.context.stats()
                later = check_species(species, nt=2, what=f"{what}, {name}: after 5 steps")
                assert sim.context.stats() == before, (before, sim.context.stats())
            got[name] = (fresh, later)
            sim.context.close()
        assert np.array_equal(got["one"][0], got["many"][0]) and np.array_equal(got["one"][1], got["many"][1]), what


# ---- ensembles -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("members,shape,check", [(512, (64, 128), [0, 1, 255, 511]), (7, (100, 130), list(range(7)))])
def test_ensemble_members_equal_lone_species(built, members, shape, check):
    params = [Parameters(feed_rate=0.01 + 0.05 * i / members, kill_rate=0.05 + 0.015 * (members - 1 - i) / members)
              for i in range(members)]
    sim = Simulation.new(params[0], HipArgs(devices=[0]))
    ens = sim.make_ensemble(shape, params)
    rng = np.random.default_rng(1)
    ens.upload(rng.random((members,) + shape, dtype=np.float32),
               (rng.random((members,) + shape, dtype=np.float32) * np.float32(0.5)).astype(np.float32))
    ens.perform_steps(23)
    # member i's last row and member i + 1's first row fully set: they stay separate components
    u, v = ens.u_views(), ens.result_views()
    for i in check:
        for j, r in ((i, shape[0] - 1), (i + 1, 0)):
            if j < members:
                u[j, r], v[j, r] = np.float32(0.0), np.float32(0.5)
    ens.upload(u, v)
    nt = 2
    for conn in (8, 4):
        allc = ens.components(v_thresholds=TV[:nt], u_thresholds=TU[:nt], connectivity=conn)
        assert allc.shape == (members, 2, nt, 35) and allc.dtype == np.uint64
        assert np.all(allc[..., 3:].sum(axis=3) == allc[..., 0])
        part = ens.components(2, 3, v_thresholds=TV[:nt], u_thresholds=TU[:nt], connectivity=conn)
        assert part.tobytes() == allc[2:5].tobytes()
        one = ens.components(1, 2, v_thresholds=TV[1:2], u_thresholds=TU[1:2], connectivity=conn)
        assert one.shape == (2, 2, 1, 35) and np.array_equal(one[:, :, 0], allc[1:3, :, 1])
        for i in check:
            for k in range(nt):
                assert np.array_equal(allc[i, 0, k], ref.counters(u[i], TU[k], False, conn)), f"member {i} U[{k}]"
                assert np.array_equal(allc[i, 1, k], ref.counters(v[i], TV[k], True, conn)), f"member {i} V[{k}]"
                c = Components.from_counters(allc[i, 1, k], TV[k], True, conn)
                assert c.largest >= shape[1]                      # (the planted row)
            lone = Simulation.new(params[i], HipArgs(devices=[0]))
            species = species_from_arrays(lone, u[i], v[i])
            cu, cv = species.components(TV[:nt], TU[:nt], connectivity=conn)
            assert np.array_equal(np.stack([words(c) for c in cu]), allc[i, 0]), f"member {i} alone, U"
            assert np.array_equal(np.stack([words(c) for c in cv]), allc[i, 1]), f"member {i} alone, V"
            lone.context.close()
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
    held = ens.components(v_thresholds=TV[:2], u_thresholds=TU[:2])
    ens.retire([1, 3])
    for steps in (3, 4):                     # an odd and an even number of further runs' steps: both slots are in play
        ens.perform_steps(steps)
        now = ens.components(v_thresholds=TV[:2], u_thresholds=TU[:2])
        u, v = ens.u_views(), ens.result_views()
        for i in range(members):
            for k in range(2):
                assert np.array_equal(now[i, 0, k], ref.counters(u[i], TU[k], False, 8)), (steps, i, k)
                assert np.array_equal(now[i, 1, k], ref.counters(v[i], TV[k], True, 8)), (steps, i, k)
        assert np.array_equal(now[[1, 3]], held[[1, 3]])
    ens.destroy()
    sim.context.close()


# ---- the sweep driver ------------------------------------------------------------------------------------------------------

def test_sweep_records_components_without_changing_the_fields(built, tmp_path):
    from grayscott_amd import hdf5_min, sweep

    base = ["--feed", "0.02:0.05:3", "--kill", "0.05:0.062:2", "-r", "48", "-c", "72", "-s", "30"]
    sweep.main(base + ["-o", str(tmp_path / "plain.h5")])
    sweep.main(base + ["--components-every", "10", "--comp-threshold-v", "0.25,0.1", "--comp-threshold-u", "0.5,0.8",
                       "--comp-connectivity", "4", "-o", str(tmp_path / "comp.h5")])
    sweep.main(base + ["--components-every", "30", "--comp-threshold-v", "0.25,0.1", "--comp-connectivity", "4", "--no-fields",
                       "-o", str(tmp_path / "nof.h5")])
    assert (tmp_path / "plain.h5").read_bytes() == (tmp_path / "comp.h5").read_bytes()
    assert not (tmp_path / "plain.components.npz").exists() and not (tmp_path / "nof.h5").exists()
    z = np.load(tmp_path / "comp.components.npz")
    assert list(z["steps"]) == [10, 20, 30] and int(z["connectivity"]) == 4
    assert z["components"].shape == (3, 6, 2, 2) and z["by_size"].shape == (3, 6, 2, 2, 32) and z["by_size"].dtype == np.uint64
    v = hdf5_min.read(str(tmp_path / "comp.h5"))
    for i in range(6):
        for k, t in enumerate((0.25, 0.1)):
            want = ref.counters(v[i], t, True, 4)
            got = [z["components"][-1, i, 1, k], z["set_cells"][-1, i, 1, k], z["largest"][-1, i, 1, k]]
            assert got == list(want[:3]) and np.array_equal(z["by_size"][-1, i, 1, k], want[3:]), (i, k)
    z2 = np.load(tmp_path / "nof.components.npz")
    assert list(z2["steps"]) == [30] and z2["components"][-1, :, 1].tobytes() == z["components"][-1, :, 1].tobytes()


def test_cpp_mirror_components(built, tmp_path):
    exe = build_program("components_mirror", tmp_path)
    members, rows, cols = 4, 72, 200
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(members), str(rows), str(cols), "31", str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    n = (2 + members) * 4 * 35
    c = np.frombuffer(raw[:8 * n], np.uint64).reshape(2 + members, 2, 2, 35)
    planes = np.frombuffer(raw[8 * n:], np.float32).reshape(2, rows, cols)
    for j, conn in enumerate((8, 4)):
        for k, (tu, tv) in enumerate(((0.5, 0.25), (0.8, 0.1))):
            assert np.array_equal(c[j, 0, k], ref.counters(planes[0], tu, False, conn))
            assert np.array_equal(c[j, 1, k], ref.counters(planes[1], tv, True, conn))
    for i in range(members):
        assert c[2 + i].tobytes() == c[0].tobytes(), i
