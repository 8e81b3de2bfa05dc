"""Bit-quad counts on the device (gs_fields_morphology, gs_members_morphology) against the numpy restatement of their rule
(tests/morph_ref.py) on the downloaded plane: all six counters equal, everywhere."""
import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Morphology, Parameters, Simulation, capi
from grayscott_amd.simulation import morphology_fields, quad_measures
from tests import morph_ref
from tests.children import build_program, run_program
from tests.helpers import species_from_arrays, stress_fields

pytestmark = pytest.mark.gpu

H = morph_ref.UNIT_ROWS  # the kernel's unit height (kQuadRows in gs_morphology.hip), restated in tests/morph_ref.py
TV, TU = (0.25, 0.1, 0.05, 0.4), (0.5, 0.8, 0.3, 0.95)   # V is set above its thresholds, U below


def assert_same(m: Morphology, plane: np.ndarray, what: str):
    want = morph_ref.quads(plane, m.threshold, m.above)
    got = m.quads
    print(f"{what}: {plane.shape} t {m.threshold} above {m.above}: quads {list(map(int, got))} area {m.area} "
          f"perimeter {m.perimeter} euler8 {m.euler8} euler4 {m.euler4}")
    assert got.dtype == np.uint64 and got.shape == (6,)
    assert int(got.sum()) == (plane.shape[0] + 1) * (plane.shape[1] + 1) and m.cells == plane.size, what
    assert np.array_equal(got, want), f"{what}: {list(map(int, got))}, not {list(map(int, want))}"
    assert m.area == int(np.count_nonzero(morph_ref.set_cells(plane, m.threshold, m.above)))


def check_species(species, nt=4, what=""):
    in_u, in_v, _, _ = species.in_out()
    ctx = species.context()
    mu, mv = species.morphology(TV[:nt], TU[:nt])
    u, v = in_u.make_scalar_view(ctx), in_v.make_scalar_view(ctx)
    assert len(mu) == nt and len(mv) == nt
    for k in range(nt):
        assert (mu[k].above, mv[k].above) == (False, True)
        assert_same(mu[k], u, f"{what} U[{k}]")
        assert_same(mv[k], v, f"{what} V[{k}]")
    return np.stack([m.quads for m in mu + mv])


# ---- planted planes ---------------------------------------------------------------------------------------------------

COLUMN_SHAPES = [(1, 1), (2, 3), (5, 253), (3, 255), (4, 256), (3, 257), (2, 1023), (6, 1025)]
ROW_SHAPES = [(H - 1, 300), (H, 300), (H + 1, 300), (2 * H + 1, 300)]


@pytest.mark.parametrize("shape", COLUMN_SHAPES + ROW_SHAPES)
def test_planted_planes(built, shape):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    thresholds = [0.3, -1.5, 0.0, 2.0 ** -130]            # distinct, one of them sub-normal
    field = HipConcentration(sim.context, shape)
    for above in (True, False):
        for i, density in enumerate((0.02, 0.5, 0.98)):
            planes = [morph_ref.planted(shape, t, 10 * i + k, density, above) for k, t in enumerate(thresholds)]
            for k, (t, p) in enumerate(zip(thresholds, planes)):
                field.upload(sim.context, p)
                four = field.morphology(sim.context, thresholds, above)        # nt = 4 in one call
                assert [m.threshold for m in four] == [float(np.float32(x)) for x in thresholds]
                for m in four:
                    assert_same(m, p, f"density {density}, plane {k}, nt 4")
                for j, x in enumerate(thresholds):                              # ... equals four calls with nt = 1
                    one = field.morphology(sim.context, [x], above)
                    assert len(one) == 1 and np.array_equal(one[0].quads, four[j].quads), (k, j)
                assert_same(field.morphology(sim.context, [t], above)[0], p, f"density {density}, plane {k}, nt 1")
    # 1 to 4 planes in a call, each with its own thresholds and sense
    planes = [morph_ref.planted(shape, thresholds[k], 40 + k, 0.5, k % 2 == 0) for k in range(4)]
    fields = []
    for p in planes:
        f = HipConcentration(sim.context, shape)
        f.upload(sim.context, p)
        fields.append(f)
    for n in (1, 2, 3, 4):
        got = morphology_fields(sim.context, fields[:n], [[thresholds[k], 0.7] for k in range(n)], [k % 2 == 0 for k in range(n)])
        assert len(got) == n
        for k in range(n):
            assert_same(got[k][0], planes[k], f"field {k} of {n}")
            assert_same(got[k][1], planes[k], f"field {k} of {n}, second threshold")
    sim.context.close()


def test_full_empty_and_infinite_thresholds(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    shape = (H + 3, 259)
    field = HipConcentration(sim.context, shape)
    p = morph_ref.planted(shape, 0.5, 3)
    field.upload(sim.context, p)
    inf = float("inf")
    for t, above in ((-inf, True), (inf, True), (inf, False), (-inf, False), (3.4028235e38, False)):
        assert_same(field.morphology(sim.context, [t], above)[0], p, f"t {t}")
    field.upload(sim.context, np.ones(shape, np.float32))
    m = field.morphology(sim.context, [0.5])[0]
    assert_same(m, np.ones(shape, np.float32), "all set")
    assert (m.area, m.perimeter, m.euler4, m.euler8) == (shape[0] * shape[1], 2 * (shape[0] + shape[1]), 1, 1)
    sim.context.close()


def test_refusals_that_need_handles_and_the_empty_plane(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    a, b = HipConcentration(sim.context, (8, 16)), HipConcentration(sim.context, (8, 17))
    foreign = HipConcentration(other.context, (8, 16))
    for fields in ([a, b], [a, foreign], [a] * 5):
        with pytest.raises(capi.GsError) as e:
            morphology_fields(sim.context, fields, [[0.5]] * len(fields), [True] * len(fields))
        assert e.value.code == capi.GS_ERR_INVALID, fields
    for thresholds in ([], [0.1] * 5, [float("nan")], [0.1, float("nan")]):
        with pytest.raises(capi.GsError) as e:
            a.morphology(sim.context, thresholds)
        assert e.value.code == capi.GS_ERR_INVALID, thresholds
    ens = sim.make_ensemble((8, 16), Parameters(), members=3)
    for first, count in ((3, 1), (2, 2), (0, 0), (0, 4)):
        with pytest.raises(capi.GsError) as e:
            ens.morphologies(first, count)
        assert e.value.code == capi.GS_ERR_INVALID, (first, count)
    theirs = other.make_ensemble((8, 16), Parameters(), members=3)
    with pytest.raises(capi.GsError) as e:
        Ensemble_morphologies_on(sim, theirs)
    assert e.value.code == capi.GS_ERR_INVALID
    for shape in ((0, 16), (7, 0)):
        empty = HipConcentration(sim.context, shape)
        for m in empty.morphology(sim.context, [0.1, 0.2]):
            assert m.cells == 0 and list(m.quads) == [0] * 6
    for s in (sim, other):
        s.context.close()


def Ensemble_morphologies_on(sim, ens):
    """``ens.morphologies()`` through the context of ``sim``."""
    import ctypes

    out = np.zeros((ens.members, 2, 1, 6), np.uint64)
    thr, sense = (ctypes.c_float * 2)(0.5, 0.25), (ctypes.c_int32 * 2)(0, 1)
    capi.check(capi.load().gs_members_morphology(sim.context.handle, ens.handle, 0, ens.members, thr, sense, 1,
                                                 out.ctypes.data_as(ctypes.POINTER(capi.GsMorphology))))


# ---- after real kernels: the pitch padding holds what they left there ---------------------------------------------------

@pytest.mark.parametrize("shape", [(1080, 1920), (200, 333)])
def test_the_producer_does_not_matter(built, shape):
    u0, v0 = stress_fields(shape, 9)
    ran, results = [], {}
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
        results[name] = check_species(species, what=f"{name} ({sim.context.info()[0]})")
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


def test_right_after_an_unsynchronised_window_call(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = sim.make_species([1080, 1920])
    sim.perform_steps(species, 64)           # tuned and settled
    sim.prepare_steps(species, 64)           # enqueued only
    mu, mv = species.morphology(TV[:1], TU[:1])
    name, _ = sim.context.info()
    assert "window" in name, name
    in_u, in_v, _, _ = species.in_out()
    assert_same(mu[0], in_u.make_scalar_view(sim.context), "U")
    assert_same(mv[0], in_v.make_scalar_view(sim.context), "V")
    sim.context.close()


# ---- slab layout --------------------------------------------------------------------------------------------------------

def seam_planes(shape, slabs, seed):
    """U and V with set cells (U below 0.5, V above 0.25) planted on both sides of every seam of `slabs` equal-as-can-be slabs."""
    rows, cols = shape
    rng = np.random.default_rng(seed)
    u, v = stress_fields(shape, seed)
    for i in range(1, slabs):
        for seam in {i * rows // slabs, (i * rows + slabs - 1) // slabs}:
            for r in (seam - 1, seam):
                if 0 <= r < rows:
                    on = rng.random(cols) < 0.6
                    u[r] = np.where(on, np.float32(0.1), np.float32(0.9))
                    v[r] = np.where(on, np.float32(0.45), np.float32(0.01))
    return u, v


@pytest.mark.parametrize("shape,slabs", [((50, 333), 3), ((9, 256), 2)])
def test_morphology_does_not_depend_on_the_slab_layout(built, shape, slabs):
    u0, v0 = seam_planes(shape, slabs, 11)
    got = {}
    for name, devices in (("one", [0]), ("many", [0] * slabs)):
        sim = Simulation.new(Parameters(), HipArgs(devices=devices))
        species = species_from_arrays(sim, u0, v0)
        before = sim.context.stats()
        fresh = check_species(species, what=f"{name}: right after upload")       # ghost rows stale
        assert sim.context.stats() == before
        sim.perform_steps(species, 5)
        before = sim.context.stats()
        later = check_species(species, what=f"{name}: after 5 steps")
        assert sim.context.stats() == before, (before, sim.context.stats())
        got[name] = (fresh, later)
        sim.context.close()
    assert np.array_equal(got["one"][0], got["many"][0]) and np.array_equal(got["one"][1], got["many"][1])


@pytest.mark.parametrize("shape", [(1080, 1920), (200, 333)])
def test_morphology_has_no_side_effects(built, shape):
    u0, v0 = stress_fields(shape, 5)
    planes, infos = [], []
    for look in (False, True):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
        species = species_from_arrays(sim, u0, v0)
        for _ in range(3):
            sim.prepare_steps(species, 40)
            if look:
                species.morphology()
                sim.context.sync()
                before = (sim.context.stats(), sim.context.info())
                species.morphology(TV, TU)
                species.u.in_out()[0].morphology(sim.context, [0.5], above=False)
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
    # member i's last row and member i + 1's first row fully set: neither may see the other
    u, v = ens.u_views(), ens.result_views()
    for i in check:
        for j, r in ((i, shape[0] - 1), (i + 1, 0)):
            if j < members:
                u[j, r], v[j, r] = np.float32(0.0), np.float32(0.5)
    ens.upload(u, v)
    nt = 4
    allm = ens.morphologies(v_thresholds=TV, u_thresholds=TU)
    assert allm.shape == (members, 2, nt, 6) and allm.dtype == np.uint64
    assert np.all(allm.sum(axis=3) == (shape[0] + 1) * (shape[1] + 1))
    part = ens.morphologies(2, 3, v_thresholds=TV, u_thresholds=TU)
    assert part.tobytes() == allm[2:5].tobytes()
    one = ens.morphologies(1, 2, v_thresholds=TV[1:2], u_thresholds=TU[1:2])
    assert one.shape == (2, 2, 1, 6) and np.array_equal(one[:, :, 0], allm[1:3, :, 1])
    area, perimeter, euler4, euler8 = quad_measures(allm)
    assert area.shape == (members, 2, nt)
    for i in check:
        for k in range(nt):
            assert np.array_equal(allm[i, 0, k], morph_ref.quads(u[i], TU[k], False)), f"member {i} U[{k}]"
            assert np.array_equal(allm[i, 1, k], morph_ref.quads(v[i], TV[k], True)), f"member {i} V[{k}]"
            want = morph_ref.measures(allm[i, 1, k])
            assert (area[i, 1, k], perimeter[i, 1, k], euler4[i, 1, k], euler8[i, 1, k]) == (
                want["area"], want["perimeter"], want["euler4"], want["euler8"])
        lone = Simulation.new(params[i], HipArgs(devices=[0]))
        species = species_from_arrays(lone, u[i], v[i])
        mu, mv = species.morphology(TV, TU)
        assert np.array_equal(np.stack([m.quads for m in mu]), allm[i, 0]), f"member {i} alone, U"
        assert np.array_equal(np.stack([m.quads for m in mv]), allm[i, 1]), f"member {i} alone, V"
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
    held = ens.morphologies(v_thresholds=TV[:2], u_thresholds=TU[:2])
    ens.retire([1, 3])
    for steps in (3, 4):                     # an odd and an even number of further runs' steps: both slots are in play
        ens.perform_steps(steps)
        now = ens.morphologies(v_thresholds=TV[:2], u_thresholds=TU[:2])
        u, v = ens.u_views(), ens.result_views()
        for i in range(members):
            for k in range(2):
                assert np.array_equal(now[i, 0, k], morph_ref.quads(u[i], TU[k], False)), (steps, i, k)
                assert np.array_equal(now[i, 1, k], morph_ref.quads(v[i], TV[k], True)), (steps, i, k)
        assert np.array_equal(now[[1, 3]], held[[1, 3]])
        assert not np.array_equal(now[[0, 2, 4]], held[[0, 2, 4]])
    ens.destroy()
    sim.context.close()


# ---- the sweep driver and the C++ mirror -----------------------------------------------------------------------------------

def test_sweep_records_morphology_without_changing_the_fields(built, tmp_path):
    from grayscott_amd import hdf5_min, sweep

    base = ["--feed", "0.02:0.05:3", "--kill", "0.05:0.062:2", "-r", "48", "-c", "72", "-s", "30"]
    sweep.main(base + ["-o", str(tmp_path / "plain.h5")])
    sweep.main(base + ["--morphology-every", "4", "--summary-every", "4", "--morph-threshold-v", "0.25,0.1",
                       "--morph-threshold-u", "0.5,0.8", "-o", str(tmp_path / "morph.h5")])
    sweep.main(base + ["--morphology-every", "30", "--morph-threshold-v", "0.25,0.1", "--no-fields", "-o", str(tmp_path / "nof.h5")])
    assert (tmp_path / "plain.h5").read_bytes() == (tmp_path / "morph.h5").read_bytes()
    assert not (tmp_path / "plain.morphology.npz").exists() and not (tmp_path / "nof.h5").exists()
    z = np.load(tmp_path / "morph.morphology.npz")
    steps = [4, 8, 12, 16, 20, 24, 28, 30]
    assert list(z["steps"]) == steps and list(np.load(tmp_path / "morph.summary.npz")["steps"]) == steps
    assert z["quads"].shape == (8, 6, 2, 2, 6) and z["quads"].dtype == np.uint64
    assert list(z["thresholds_v"]) == [np.float32(0.25), np.float32(0.1)] and list(z["thresholds_u"]) == [np.float32(0.5), np.float32(0.8)]
    assert np.all(z["quads"].sum(axis=4) == 49 * 73)
    for key in ("area_fraction", "perimeter", "euler4", "euler8"):
        assert z[key].shape == (8, 6, 2, 2), key
    v = hdf5_min.read(str(tmp_path / "morph.h5"))
    for i in range(6):
        for k, t in enumerate((0.25, 0.1)):
            want = morph_ref.quads(v[i], t, True)
            assert np.array_equal(z["quads"][-1, i, 1, k], want), (i, k)
            m = morph_ref.measures(want)
            assert z["euler8"][-1, i, 1, k] == m["euler8"] and z["euler4"][-1, i, 1, k] == m["euler4"]
            assert z["perimeter"][-1, i, 1, k] == m["perimeter"] and z["area_fraction"][-1, i, 1, k] == m["area"] / (48 * 72)
    z2 = np.load(tmp_path / "nof.morphology.npz")
    assert list(z2["steps"]) == [30] and z2["quads"].shape == (1, 6, 2, 2, 6)
    assert z2["quads"][-1, :, 1].tobytes() == z["quads"][-1, :, 1].tobytes()


def test_cpp_mirror_morphology(built, tmp_path):
    exe = build_program("morphology_mirror", tmp_path)
    members, rows, cols = 4, 72, 200
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(members), str(rows), str(cols), "31", str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    n = (1 + members) * 4 * 6
    c = np.frombuffer(raw[:8 * n], np.uint64).reshape(1 + members, 2, 2, 6)
    planes = np.frombuffer(raw[8 * n:], np.float32).reshape(2, rows, cols)
    for k, (tu, tv) in enumerate(((0.5, 0.25), (0.8, 0.1))):
        assert np.array_equal(c[0, 0, k], morph_ref.quads(planes[0], tu, False))
        assert np.array_equal(c[0, 1, k], morph_ref.quads(planes[1], tv, True))
    for i in range(members):
        assert c[1 + i].tobytes() == c[0].tobytes(), i
