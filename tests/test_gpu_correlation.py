"""Two-point pair counts on the device (gs_fields_correlation, gs_members_correlation) against the numpy restatement of
their rule (tests/corr_ref.py) on the downloaded plane: every counter equal, everywhere."""
import ctypes

import numpy as np
import pytest

from grayscott_amd import Correlation, HipArgs, HipConcentration, Parameters, Simulation, capi, correlation_fields
from tests import corr_ref, morph_ref
from tests.children import build_program, run_program
from tests.helpers import species_from_arrays, stress_fields

pytestmark = pytest.mark.gpu

H = corr_ref.UNIT_ROWS  # the kernel's unit height (kPairRows in gs_correlation.hip), restated in tests/corr_ref.py
TV, TU = (0.25, 0.1, 0.05, 0.4), (0.5, 0.8, 0.3, 0.95)   # V is set above its thresholds, U below

_wanted = {}


def want(plane, t, above, lag):
    """The restatement, computed once per (plane bytes, threshold, sense, lag)."""
    key = (plane.shape, hash(plane.tobytes()), float(np.float32(t)), bool(above), lag)
    if key not in _wanted:
        _wanted[key] = corr_ref.pairs(plane, t, above, lag)
    return _wanted[key]


def assert_same(c: Correlation, plane: np.ndarray, what: str):
    w = want(plane, c.threshold, c.above, c.max_lag)
    got = c.pairs
    print(f"{what}: {plane.shape} t {c.threshold} above {c.above} L {c.max_lag}: set {int(got[0, 0])} "
          f"lag 1 {[int(x) for x in got[:, 1]]}")
    assert got.dtype == np.uint64 and got.shape == (4, c.max_lag + 1)
    assert np.array_equal(got, w), f"{what}: first difference at {np.argwhere(got != w)[:4].tolist()}"
    assert (c.rows, c.cols) == plane.shape
    assert np.all(got.astype(np.int64) <= corr_ref.totals(c.rows, c.cols, c.max_lag))


def check_species(species, nt=4, lag=16, what=""):
    in_u, in_v, _, _ = species.in_out()
    ctx = species.context()
    cu, cv = species.correlation(TV[:nt], TU[:nt], max_lag=lag)
    u, v = in_u.make_scalar_view(ctx), in_v.make_scalar_view(ctx)
    assert len(cu) == nt and len(cv) == nt
    for k in range(nt):
        assert (cu[k].above, cv[k].above) == (False, True)
        assert_same(cu[k], u, f"{what} U[{k}]")
        assert_same(cv[k], v, f"{what} V[{k}]")
    return np.stack([c.pairs for c in cu + cv])


# ---- planted planes ---------------------------------------------------------------------------------------------------

def planted_planes(shape, t, above):
    rows, cols = shape
    on, off = (np.float32(t + 1.0), np.float32(t - 1.0)) if above else (np.float32(t - 1.0), np.float32(t + 1.0))
    out = {}
    for name, density in (("half", 0.5), ("eighth", 0.125)):
        out[name] = morph_ref.planted(shape, t, int(density * 16) + rows + cols, density, above)  # NaN, inf, == t, sub-normals
    out["stripes"] = corr_ref.stripes(shape, 6, 2, float(off), float(on))
    corners = np.full(shape, off, np.float32)
    for r, c in ((0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)):
        corners[r, c] = on
    out["corners"] = corners
    out["all"] = np.full(shape, on, np.float32)
    out["none"] = np.full(shape, off, np.float32)
    return out


COLUMN_SHAPES = [(70, 1), (9, 63), (9, 64), (9, 65), (70, 255), (9, 256), (70, 257), (9, 513), (70, 333)]
ROW_SHAPES = [(H - 1, 70), (H, 70), (H + 1, 300), (1, 300), (2 * H + 1, 65)]


@pytest.mark.parametrize("shape", COLUMN_SHAPES + ROW_SHAPES)
def test_planted_planes(built, shape):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    field = HipConcentration(sim.context, shape)
    t = 0.3
    for above in (True, False):
        for name, p in planted_planes(shape, t, above).items():
            field.upload(sim.context, p)
            for lag in (1, 7, 64):                      # 64 exceeds the rows or the columns of most shapes: those lags count 0
                c = field.correlation(sim.context, [t], lag, above)[0]
                assert_same(c, p, f"{name} L {lag}")
                if name == "all":
                    assert np.array_equal(c.pairs.astype(np.int64), corr_ref.totals(shape[0], shape[1], lag))
                if name == "none":
                    assert not c.pairs.any()
    sim.context.close()


@pytest.mark.parametrize("shape", [(70, 333), (H + 1, 300)])
def test_four_thresholds_in_one_call_equal_four_calls(built, shape):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    thresholds = [0.3, -1.5, 0.0, 2.0 ** -130]            # distinct, one of them sub-normal
    field = HipConcentration(sim.context, shape)
    for above in (True, False):
        for k, t in enumerate(thresholds):
            p = morph_ref.planted(shape, t, 10 + k, 0.5, above)
            field.upload(sim.context, p)
            four = field.correlation(sim.context, thresholds, 24, above)
            assert [c.threshold for c in four] == [float(np.float32(x)) for x in thresholds]
            for j, x in enumerate(thresholds):
                assert_same(four[j], p, f"plane {k}, threshold {j} of 4")
                one = field.correlation(sim.context, [x], 24, above)
                assert len(one) == 1 and np.array_equal(one[0].pairs, four[j].pairs), (k, j)
            for nt in (2, 3):
                some = field.correlation(sim.context, thresholds[:nt], 24, above)
                assert all(np.array_equal(some[j].pairs, four[j].pairs) for j in range(nt))
    # 1 to 4 planes in a call, each with its own thresholds and sense
    planes = [morph_ref.planted(shape, thresholds[k], 40 + k, 0.5, k % 2 == 0) for k in range(4)]
    fields = []
    for p in planes:
        f = HipConcentration(sim.context, shape)
        f.upload(sim.context, p)
        fields.append(f)
    for n in (1, 2, 3, 4):
        got = correlation_fields(sim.context, fields[:n], [[thresholds[k], 0.7] for k in range(n)],
                                 [k % 2 == 0 for k in range(n)], 9)
        assert len(got) == n
        for k in range(n):
            assert_same(got[k][0], planes[k], f"field {k} of {n}")
            assert_same(got[k][1], planes[k], f"field {k} of {n}, second threshold")
    sim.context.close()


def test_infinite_thresholds_and_d0_is_the_area(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    shape = (H + 3, 259)
    field = HipConcentration(sim.context, shape)
    p = morph_ref.planted(shape, 0.5, 3)
    field.upload(sim.context, p)
    inf = float("inf")
    for t, above in ((-inf, True), (inf, True), (inf, False), (-inf, False), (3.4028235e38, False), (0.5, True)):
        c = field.correlation(sim.context, [t], 5, above)[0]
        assert_same(c, p, f"t {t}")
        m = field.morphology(sim.context, [t], above)[0]
        assert [int(x) for x in c.pairs[:, 0]] == [m.area] * 4
    sim.context.close()


def members_correlation_on(sim, ens, nt=1, lag=4):
    """``gs_members_correlation`` of ``ens`` through the context of ``sim``, which need not be its own (the Python mirror
    always takes the ensemble's): raises the call's refusal.  The counts land in a buffer nobody reads."""
    out = (ctypes.c_uint64 * (ens.members * 2 * 4 * 4 * 65))()
    thr, sense = (ctypes.c_float * 8)(*([0.5] * 8)), (ctypes.c_int32 * 2)(0, 1)
    capi.check(capi.load().gs_members_correlation(sim.context.handle, ens.handle, 0, ens.members, thr, sense, nt, lag, out))


def test_refusals_and_the_empty_plane(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    lib = capi.load()
    a, b = HipConcentration(sim.context, (8, 16)), HipConcentration(sim.context, (8, 17))
    foreign = HipConcentration(other.context, (8, 16))
    for fields in ([a, b], [a, foreign], [a] * 5):
        with pytest.raises(capi.GsError) as e:
            correlation_fields(sim.context, fields, [[0.5]] * len(fields), [True] * len(fields), 4)
        assert e.value.code == capi.GS_ERR_INVALID, fields
    for thresholds in ([], [0.1] * 5, [float("nan")], [0.1, float("nan")]):
        with pytest.raises(capi.GsError) as e:
            a.correlation(sim.context, thresholds, 4)
        assert e.value.code == capi.GS_ERR_INVALID, thresholds
    for lag in (0, -1, 65, 1 << 20):
        with pytest.raises(capi.GsError) as e:
            a.correlation(sim.context, [0.1], lag)
        assert e.value.code == capi.GS_ERR_INVALID, lag
    # null arguments, and the argument checks come before any handle is looked at: a foreign field with a bad lag, nt or
    # threshold is refused for the argument (the message names it)
    out = np.zeros(4 * 65 * 8, np.uint64)
    po = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    thr, nan, sense = (ctypes.c_float * 4)(0.5, 0.5, 0.5, 0.5), (ctypes.c_float * 4)(float("nan"), 0, 0, 0), (ctypes.c_int32 * 4)(1, 1, 1, 1)
    handles = (ctypes.c_void_p * 1)(foreign.handle)
    assert lib.gs_fields_correlation(None, handles, 1, thr, sense, 1, 4, po) == capi.GS_ERR_INVALID
    assert lib.gs_fields_correlation(sim.context.handle, None, 1, thr, sense, 1, 4, po) == capi.GS_ERR_INVALID
    assert lib.gs_fields_correlation(sim.context.handle, handles, 1, None, sense, 1, 4, po) == capi.GS_ERR_INVALID
    assert lib.gs_fields_correlation(sim.context.handle, handles, 1, thr, None, 1, 4, po) == capi.GS_ERR_INVALID
    assert lib.gs_fields_correlation(sim.context.handle, handles, 1, thr, sense, 1, 4, None) == capi.GS_ERR_INVALID
    for args, word in (((thr, sense, 5, 4), "thresholds"), ((nan, sense, 1, 4), "NaN"), ((thr, sense, 1, 65), "lag")):
        assert lib.gs_fields_correlation(sim.context.handle, handles, 1, *args, po) == capi.GS_ERR_INVALID
        assert word in lib.gs_last_error().decode(), (word, lib.gs_last_error())
    ens = sim.make_ensemble((8, 16), Parameters(), members=3)
    for first, count in ((3, 1), (2, 2), (0, 0), (0, 4)):
        with pytest.raises(capi.GsError) as e:
            ens.correlations(first, count, max_lag=4)
        assert e.value.code == capi.GS_ERR_INVALID, (first, count)
    for kw in ({"max_lag": 0}, {"max_lag": 65}, {"v_thresholds": [float("nan")]}, {"v_thresholds": [0.1] * 5, "u_thresholds": [0.1] * 5}):
        with pytest.raises(capi.GsError) as e:
            ens.correlations(**kw)
        assert e.value.code == capi.GS_ERR_INVALID, kw
    theirs = other.make_ensemble((8, 16), Parameters(), members=3)
    with pytest.raises(capi.GsError) as e:
        members_correlation_on(sim, theirs)
    assert e.value.code == capi.GS_ERR_INVALID
    for word, kw in (("lag", {"lag": 65}), ("thresholds", {"nt": 5})):   # ... before the foreign ensemble is looked at
        with pytest.raises(capi.GsError) as e:
            members_correlation_on(sim, theirs, **kw)
        assert e.value.code == capi.GS_ERR_INVALID and word in str(e.value), (word, str(e.value))
    for shape in ((0, 16), (7, 0)):
        empty = HipConcentration(sim.context, shape)
        for c in empty.correlation(sim.context, [0.1, 0.2], 8):
            assert c.pairs.shape == (4, 9) and not c.pairs.any()
    for s in (sim, other):
        s.context.close()


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
        results[name] = check_species(species, nt=2, what=f"{name} ({sim.context.info()[0]})")
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
    check_species(species, lag=64, what=sim.context.info()[0])
    sim.context.close()


def test_right_after_an_unsynchronised_window_call(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = sim.make_species([1080, 1920])
    sim.perform_steps(species, 64)           # tuned and settled
    sim.prepare_steps(species, 64)           # enqueued only
    cu, cv = species.correlation(TV[:1], TU[:1], max_lag=8)
    name, _ = sim.context.info()
    assert "window" in name, name
    in_u, in_v, _, _ = species.in_out()
    assert_same(cu[0], in_u.make_scalar_view(sim.context), "U")
    assert_same(cv[0], in_v.make_scalar_view(sim.context), "V")
    sim.context.close()


# ---- slab layout --------------------------------------------------------------------------------------------------------

def seam_planes(shape, seed):
    """U and V with cells set at density 1/2 (U below 0.5, V above 0.25) everywhere: every seam has set cells on both sides
    at every lag."""
    rng = np.random.default_rng(seed)
    on = rng.random(shape) < 0.5
    u = np.where(on, np.float32(0.1), np.float32(0.9)).astype(np.float32)
    v = np.where(rng.random(shape) < 0.5, np.float32(0.45), np.float32(0.01)).astype(np.float32)
    return u, v


@pytest.mark.parametrize("shape,slabs,lag", [((50, 333), 3, 16), ((9, 256), 2, 4)])
def test_correlation_does_not_depend_on_the_slab_layout(built, shape, slabs, lag):
    u0, v0 = seam_planes(shape, 11)
    got = {}
    for name, devices in (("one", [0]), ("many", [0] * slabs)):
        sim = Simulation.new(Parameters(), HipArgs(devices=devices))
        species = species_from_arrays(sim, u0, v0)
        before = sim.context.stats()
        fresh = check_species(species, lag=lag, what=f"{name}: right after upload")       # ghost rows stale
        assert sim.context.stats() == before
        sim.perform_steps(species, 5)
        before = sim.context.stats()
        later = check_species(species, lag=lag, what=f"{name}: after 5 steps")
        assert sim.context.stats() == before, (before, sim.context.stats())
        got[name] = (fresh, later)
        sim.context.close()
    assert np.array_equal(got["one"][0], got["many"][0]) and np.array_equal(got["one"][1], got["many"][1])


def test_a_slab_shorter_than_the_lag_is_unsupported(built):
    u0, v0 = seam_planes((50, 333), 11)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * 3))
    species = species_from_arrays(sim, u0, v0)
    with pytest.raises(capi.GsError) as e:
        species.correlation(TV[:1], TU[:1], max_lag=32)
    assert e.value.code == capi.GS_ERR_UNSUPPORTED
    check_species(species, nt=1, lag=16, what="3 slabs after the refusal")
    sim.context.close()
    one = Simulation.new(Parameters(), HipArgs(devices=[0]))                 # a lone slab takes any lag
    check_species(species_from_arrays(one, u0, v0), nt=1, lag=64, what="one slab")
    one.context.close()


@pytest.mark.parametrize("shape", [(1080, 1920), (200, 333)])
def test_correlation_has_no_side_effects(built, shape):
    u0, v0 = stress_fields(shape, 5)
    planes, infos = [], []
    for look in (False, True):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
        species = species_from_arrays(sim, u0, v0)
        for _ in range(3):
            sim.prepare_steps(species, 40)
            if look:
                species.correlation()
                sim.context.sync()
                before = (sim.context.stats(), sim.context.info())
                species.correlation(TV, TU, max_lag=64)
                species.u.in_out()[0].correlation(sim.context, [0.5], 3, above=False)
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


def test_correlation_leaves_the_ghost_rows_of_a_slab_chain_alone(built):
    """A field's ghost depth is not read out by any call, but it shows: were it touched, the pass after the look would
    refresh the ghost rows (``ghost_refreshes``) or step on stale ones (other bits)."""
    u0, v0 = seam_planes((50, 333), 4)
    stats, planes = [], []
    for look in (False, True):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0] * 3))
        species = species_from_arrays(sim, u0, v0)
        for _ in range(3):
            sim.perform_steps(species, 7)
            if look:
                before = sim.context.stats()
                species.correlation(TV, TU, max_lag=16)
                assert sim.context.stats() == before
        sim.context.sync()
        stats.append(sim.context.stats())
        in_u, in_v, _, _ = species.in_out()
        planes.append((in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)))
        sim.context.close()
    print(stats)
    for key in ("passes", "steps", "launches", "ghost_refreshes"):
        assert stats[0][key] == stats[1][key], (key, stats)
    assert stats[0]["ghost_refreshes"] >= 1, stats                       # (the one after the upload: the counter is alive)
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
    # member i's last rows and member i + 1's first rows fully set: neither may see the other
    u, v = ens.u_views(), ens.result_views()
    for i in check:
        for j, r in ((i, slice(shape[0] - 3, shape[0])), (i + 1, slice(0, 3))):
            if j < members:
                u[j, r], v[j, r] = np.float32(0.0), np.float32(0.5)
    ens.upload(u, v)
    nt, lag = 4, 20
    allc = ens.correlations(v_thresholds=TV, u_thresholds=TU, max_lag=lag)
    assert allc.shape == (members, 2, nt, 4, lag + 1) and allc.dtype == np.uint64
    part = ens.correlations(2, 3, v_thresholds=TV, u_thresholds=TU, max_lag=lag)
    assert part.tobytes() == allc[2:5].tobytes()
    one = ens.correlations(1, 2, v_thresholds=TV[1:2], u_thresholds=TU[1:2], max_lag=lag)
    assert one.shape == (2, 2, 1, 4, lag + 1) and np.array_equal(one[:, :, 0], allc[1:3, :, 1])
    for i in check:
        for k in range(nt):
            assert np.array_equal(allc[i, 0, k], want(u[i], TU[k], False, lag)), f"member {i} U[{k}]"
            assert np.array_equal(allc[i, 1, k], want(v[i], TV[k], True, lag)), f"member {i} V[{k}]"
        lone = Simulation.new(params[i], HipArgs(devices=[0]))
        species = species_from_arrays(lone, u[i], v[i])
        cu, cv = species.correlation(TV, TU, max_lag=lag)
        assert np.array_equal(np.stack([c.pairs for c in cu]), allc[i, 0]), f"member {i} alone, U"
        assert np.array_equal(np.stack([c.pairs for c in cv]), allc[i, 1]), f"member {i} alone, V"
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
    held = ens.correlations(v_thresholds=TV[:2], u_thresholds=TU[:2], max_lag=6)
    ens.retire([1, 3])
    for steps in (3, 4):                     # an odd and an even number of further runs' steps: both slots are in play
        ens.perform_steps(steps)
        now = ens.correlations(v_thresholds=TV[:2], u_thresholds=TU[:2], max_lag=6)
        u, v = ens.u_views(), ens.result_views()
        for i in range(members):
            for k in range(2):
                assert np.array_equal(now[i, 0, k], want(u[i], TU[k], False, 6)), (steps, i, k)
                assert np.array_equal(now[i, 1, k], want(v[i], TV[k], True, 6)), (steps, i, k)
        assert np.array_equal(now[[1, 3]], held[[1, 3]])
        assert not np.array_equal(now[[0, 2, 4]], held[[0, 2, 4]])
    ens.destroy()
    sim.context.close()


# ---- the sweep driver and the C++ mirror -----------------------------------------------------------------------------------

def test_sweep_records_correlations_without_changing_the_fields(built, tmp_path):
    from grayscott_amd import hdf5_min, sweep

    base = ["--feed", "0.02:0.05:3", "--kill", "0.05:0.062:2", "-r", "48", "-c", "72", "-s", "30"]
    sweep.main(base + ["-o", str(tmp_path / "plain.h5")])
    sweep.main(base + ["--correlation-every", "4", "--summary-every", "4", "--corr-threshold-v", "0.25,0.1",
                       "--corr-threshold-u", "0.5,0.8", "--corr-lags", "12", "-o", str(tmp_path / "corr.h5")])
    sweep.main(base + ["--correlation-every", "30", "--corr-threshold-v", "0.25,0.1", "--corr-lags", "12", "--no-fields",
                       "-o", str(tmp_path / "nof.h5")])
    assert (tmp_path / "plain.h5").read_bytes() == (tmp_path / "corr.h5").read_bytes()
    assert not (tmp_path / "plain.correlation.npz").exists() and not (tmp_path / "nof.h5").exists()
    z = np.load(tmp_path / "corr.correlation.npz")
    steps = [4, 8, 12, 16, 20, 24, 28, 30]
    assert list(z["steps"]) == steps and list(np.load(tmp_path / "corr.summary.npz")["steps"]) == steps
    assert z["pairs"].shape == (8, 6, 2, 2, 4, 13) and z["pairs"].dtype == np.uint64
    assert int(z["max_lag"]) == 12 and list(z["shape"]) == [48, 72]
    assert list(z["thresholds_v"]) == [np.float32(0.25), np.float32(0.1)] and list(z["thresholds_u"]) == [np.float32(0.5), np.float32(0.8)]
    assert np.array_equal(z["pairs_total"], corr_ref.totals(48, 72, 12))
    v = hdf5_min.read(str(tmp_path / "corr.h5"))
    for i in range(6):
        for k, t in enumerate((0.25, 0.1)):
            assert np.array_equal(z["pairs"][-1, i, 1, k], corr_ref.pairs(v[i], t, True, 12)), (i, k)
    z2 = np.load(tmp_path / "nof.correlation.npz")
    assert list(z2["steps"]) == [30] and z2["pairs"].shape == (1, 6, 2, 2, 4, 13)
    assert z2["pairs"][-1, :, 1].tobytes() == z["pairs"][-1, :, 1].tobytes()


def test_cpp_mirror_correlation(built, tmp_path):
    exe = build_program("correlation_mirror", tmp_path)
    members, rows, cols, lag = 4, 72, 200, 10
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(members), str(rows), str(cols), "31", str(lag), str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    n = (1 + members) * 4 * 4 * (lag + 1)
    c = np.frombuffer(raw[:8 * n], np.uint64).reshape(1 + members, 2, 2, 4, lag + 1)
    planes = np.frombuffer(raw[8 * n:], np.float32).reshape(2, rows, cols)
    for k, (tu, tv) in enumerate(((0.5, 0.25), (0.8, 0.1))):
        assert np.array_equal(c[0, 0, k], corr_ref.pairs(planes[0], tu, False, lag))
        assert np.array_equal(c[0, 1, k], corr_ref.pairs(planes[1], tv, True, lag))
    for i in range(members):
        assert c[1 + i].tobytes() == c[0].tobytes(), i
