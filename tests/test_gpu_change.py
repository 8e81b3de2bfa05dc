"""Two states compared on the device (gs_fields_compare, gs_members_compare) against the numpy restatement of the rule
(tests/change_ref.py), bit for bit -- sums and the maximum as f64 bit patterns, equal counts --, and the device copies
behind snapshots and restores (gs_fields_copy, gs_members_copy)."""
import json

import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, Simulation, capi
from grayscott_amd.simulation import CHANGE_DTYPE, compare_fields, copy_fields
from tests import change_ref
from tests.children import build_program, run_program
from tests.helpers import species_from_arrays, stress_fields

pytestmark = pytest.mark.gpu

RULES = {"clipped": capi.GS_BOUNDARY_CLIPPED, "zero_halo": capi.GS_BOUNDARY_ZERO_HALO,
         "periodic": capi.GS_BOUNDARY_PERIODIC, "neumann": capi.GS_BOUNDARY_NEUMANN}


def planes_of(species):
    in_u, in_v, _, _ = species.in_out()
    ctx = species.context()
    return in_u.make_scalar_view(ctx), in_v.make_scalar_view(ctx)


def assert_same(got, want, what):
    assert change_ref.same(got, want), f"{what}: {change_ref.as_dict(got)} != {change_ref.as_dict(want)}"


def uploaded(sim, array):
    plane = HipConcentration(sim.context, array.shape)
    plane.upload(sim.context, array)
    return plane


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (7, 13), (37, 1029), (64, 128), (1080, 1920), (4096, 4096)])
def test_change_since_matches_the_restatement(built, rule, shape):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], boundary=RULES[rule], place_candidates=0))
    u0, v0 = stress_fields(shape, 7)
    species = species_from_arrays(sim, u0, v0)
    sim.perform_steps(species, 9)
    snap = species.snapshot()
    before = planes_of(species)
    sim.perform_steps(species, 4)
    u, v = species.change_since(snap)
    after = planes_of(species)
    assert_same(u, change_ref.change(after[0], before[0]), "U")
    assert_same(v, change_ref.change(after[1], before[1]), "V")
    assert u.cells == shape[0] * shape[1] and u.nonfinite == 0 and u.comparable == u.cells
    assert u.differing > 0 and u.max_abs > 0.0 and not u.equal
    snap.close()
    sim.context.close()


def test_planted_cells_are_counted_and_skipped(built):
    rows, cols = 37, 1029
    rng = np.random.default_rng(3)
    # O: the order-sensitive magnitudes as they are; U: the same with every special case at random positions
    oa, ob = change_ref.order_sensitive((rows, cols), 4)
    plain, wrong = change_ref.change(oa, ob), change_ref.ascending(oa, ob)
    assert change_ref.bits(plain["sum_abs"]) != change_ref.bits(wrong["sum_abs"])
    assert change_ref.bits(plain["sum_sq"]) != change_ref.bits(wrong["sum_sq"])
    ua, ub = oa.copy(), ob.copy()
    nan2 = np.array([0x7fc00001], np.uint32).view(np.float32)[0]
    nan3 = np.array([0xffc00002], np.uint32).view(np.float32)[0]
    pairs = [(np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.inf, np.inf), (np.inf, -np.inf), (-np.inf, 2.0),
             (0.0, -0.0), (-0.0, 0.0), (1e-45, -1e-45), (-1e-45, -1e-45), (1e-40, 3e-39), (nan2, nan2), (nan2, nan3),
             (2.0 ** 80, -2.0 ** 80), (2.0 ** 80, 1.0), (1.0, 1.0)]
    unlike = sum(1 for x, y in pairs if not (np.isfinite(x) and np.isfinite(y)))
    pos = rng.choice(rows * cols, size=6 * len(pairs), replace=False)
    for i, p in enumerate(pos):
        x, y = pairs[i % len(pairs)]
        ua.flat[p], ub.flat[p] = x, y
    # V: the only comparable cell is a pair of sub-normals
    va = np.full((rows, cols), np.nan, np.float32)
    vb = np.full((rows, cols), np.inf, np.float32)
    va[5, 7], vb[5, 7] = 1e-45, -1e-45
    va[6, 7], vb[9, 1000] = 1.0, 1.0                       # finite in one plane only: not comparable
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    dev = [uploaded(sim, x) for x in (ua, va, oa, ub, vb, ob)]
    cu, cv, co = compare_fields(sim.context, dev[:3], dev[3:])
    assert_same(co, plain, "order-sensitive planes")
    want = change_ref.change(ua, ub)
    assert_same(cu, want, "U")
    assert want["nonfinite"] == 6 * unlike == 48 and cu.comparable == rows * cols - 48
    assert np.isfinite(cu.sum_abs) and np.isfinite(cu.sum_sq) and cu.max_abs == 2.0 ** 81
    assert cu.differing == int(np.count_nonzero(ua.view(np.uint32) != ub.view(np.uint32)))
    assert_same(cv, change_ref.change(va, vb), "V")
    assert cv.comparable == 1 and cv.differing == rows * cols
    assert cv.max_abs == cv.sum_abs == 2.0 ** -148 and cv.sum_sq == 2.0 ** -296
    # the other way round: the same magnitudes
    ru, _ = compare_fields(sim.context, dev[3:5], dev[:2])
    assert_same(ru, change_ref.change(ub, ua), "U reversed")
    assert (ru.sum_abs, ru.sum_sq, ru.max_abs) == (cu.sum_abs, cu.sum_sq, cu.max_abs)
    # pairs with two comparable cells and with none
    two = dev[1].change_from(sim.context, uploaded(sim, np.full((rows, cols), 1.0, np.float32)))
    assert two.comparable == 2 and two.max_abs == 1.0 - 2.0 ** -149
    lost = np.full((rows, cols), -np.inf, np.float32)
    bad = uploaded(sim, lost).change_from(sim.context, dev[0])
    assert bad.nonfinite == rows * cols and bad.comparable == 0
    assert bad.differing == int(np.count_nonzero(lost.view(np.uint32) != ua.view(np.uint32))) == rows * cols - 6
    assert all(change_ref.bits(getattr(bad, f)) == 0 for f in ("sum_abs", "sum_sq", "max_abs"))
    sim.context.close()


def test_identity(built):
    shape = (123, 457)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = stress_fields(shape, 2)
    u0[3, 5] = np.nan                                       # the same bits on both sides: not differing, not comparable
    species = species_from_arrays(sim, u0, v0)
    in_u, in_v, _, _ = species.in_out()
    zero = change_ref.change(v0, v0)
    for c in compare_fields(sim.context, [in_v, in_v], [in_v, in_v]) + [in_v.change_from(sim.context, in_v)]:
        assert_same(c, zero, "a plane against itself")
        assert c.equal
    su = in_u.change_from(sim.context, in_u)
    assert su.equal and su.nonfinite == 1 and su.max_abs == 0.0
    snap = species.snapshot()
    fresh = species.change_since(snap)
    assert fresh[0].equal and fresh[1].equal and fresh[0].nonfinite == 1 and fresh[1].sum_abs == 0.0
    u0[3, 5] = 0.5
    in_u.upload(sim.context, u0)
    sim.perform_steps(species, 3)
    a, b = planes_of(species), (snap.u.make_scalar_view(sim.context), snap.v.make_scalar_view(sim.context))
    assert b[1].tobytes() == v0.tobytes()
    u, v = species.change_since(snap)
    assert u.differing == np.count_nonzero(a[0].view(np.uint32) != b[0].view(np.uint32))
    assert v.differing == np.count_nonzero(a[1].view(np.uint32) != b[1].view(np.uint32))
    snap.update(species)
    assert all(c.equal for c in species.change_since(snap))
    snap.close()
    sim.context.close()


def test_change_does_not_depend_on_the_slab_layout(built):
    shape = (1000, 777)
    u0, v0 = stress_fields(shape, 11)
    got = {}
    for name, args in [("1", HipArgs(devices=[0])), ("2", HipArgs(devices=[0] * 2)), ("3", HipArgs(devices=[0] * 3)),
                       ("5", HipArgs(devices=[0] * 5)), ("split2", HipArgs(devices=[0], split=2))]:
        sim = Simulation.new(Parameters(), args)
        species = species_from_arrays(sim, u0, v0)
        sim.perform_steps(species, 9)
        snap = species.snapshot()
        if name == "1":
            before = planes_of(species)
        sim.perform_steps(species, 13)
        got[name] = species.change_since(snap)
        if name == "1":
            after = planes_of(species)
            want = change_ref.change(after[0], before[0]), change_ref.change(after[1], before[1])
        sim.context.close()
    for name, (u, v) in got.items():
        assert_same(u, want[0], f"U, {name} slabs")
        assert_same(v, want[1], f"V, {name} slabs")


def test_change_right_after_an_unsynchronised_window_call(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = sim.make_species([1080, 1920])
    sim.perform_steps(species, 64)           # tuned and settled
    snap = species.snapshot()
    before = planes_of(species)
    sim.prepare_steps(species, 64)           # enqueued only
    u, v = species.change_since(snap)
    name, _ = sim.context.info()
    assert "window" in name, name
    after = planes_of(species)
    assert_same(u, change_ref.change(after[0], before[0]), "U")
    assert_same(v, change_ref.change(after[1], before[1]), "V")
    sim.context.close()


@pytest.mark.parametrize("shape", [(1080, 1920), (200, 333)])
def test_comparisons_and_snapshots_have_no_side_effects(built, shape):
    u0, v0 = stress_fields(shape, 5)
    planes = []
    for compare in (False, True):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
        species = species_from_arrays(sim, u0, v0)
        snap = species.snapshot() if compare else None
        for _ in range(3):
            sim.prepare_steps(species, 40)
            if compare:
                species.change_since(snap)
                sim.context.sync()
                before = (sim.context.stats(), sim.context.info())
                species.change_since(snap)
                species.u.in_out()[0].change_from(sim.context, snap.u)
                snap.update(species)
                other = species.snapshot()
                assert (sim.context.stats(), sim.context.info()) == before
                other.close()
        sim.context.sync()
        planes.append(planes_of(species))
        sim.context.close()
    assert planes[0][0].tobytes() == planes[1][0].tobytes()
    assert planes[0][1].tobytes() == planes[1][1].tobytes()


def wall_mask(shape):
    m = np.zeros(shape, np.float32)
    m[shape[0] // 3, : 2 * shape[1] // 3] = 1.0
    m[: shape[0] // 2, shape[1] // 2] = 1.0
    return m


@pytest.mark.parametrize("case", ["one_slab", "three_slabs", "periodic", "neumann", "neumann_three_slabs", "map", "mask"])
def test_snapshot_and_restore(built, case):
    """20 steps, snapshot, 20 steps, restore, 20 steps: the state after the first 40 steps, bit for bit."""
    shape = (150, 203)
    args = {"one_slab": HipArgs(devices=[0]), "three_slabs": HipArgs(devices=[0] * 3),
            "periodic": HipArgs(devices=[0], boundary=capi.GS_BOUNDARY_PERIODIC),
            "neumann": HipArgs(devices=[0], boundary=capi.GS_BOUNDARY_NEUMANN),
            "neumann_three_slabs": HipArgs(devices=[0] * 3, boundary=capi.GS_BOUNDARY_NEUMANN),
            "map": HipArgs(devices=[0] * 2), "mask": HipArgs(devices=[0] * 2)}[case]
    sim = Simulation.new(Parameters(), args)
    if case == "map":
        feed = np.linspace(0.01, 0.06, shape[1], dtype=np.float32)[None, :].repeat(shape[0], 0)
        kill = np.linspace(0.045, 0.065, shape[0], dtype=np.float32)[:, None].repeat(shape[1], 1)
        sim.set_param_map(feed, kill)
    if case == "mask":
        sim.set_mask(wall_mask(shape))
    u0, v0 = stress_fields(shape, 9)
    species = species_from_arrays(sim, u0, v0)
    sim.perform_steps(species, 20)
    snap = species.snapshot()
    sim.perform_steps(species, 20)
    want = planes_of(species)
    gone = species.change_since(snap)
    assert not gone[0].equal and not gone[1].equal
    species.restore(snap)
    assert all(c.equal for c in species.change_since(snap))
    sim.perform_steps(species, 20)
    got = planes_of(species)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    # an odd number of steps (the species' planes swap roles), then back again
    sim.perform_steps(species, 7)
    species.restore(snap)
    sim.perform_steps(species, 20)
    got = planes_of(species)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    snap.close()
    sim.context.close()


@pytest.mark.parametrize("rule", ["clipped", "periodic", "neumann"])
@pytest.mark.parametrize("shape", [(32, 64), (45, 61), (100, 130)])  # resident form, then tile forms (61, 130: cols % 4 != 0)
def test_ensemble_members_equal_lone_species(built, rule, shape):
    members = 5
    params = [Parameters(feed_rate=0.01 + 0.006 * i, kill_rate=0.05 + 0.002 * (members - 1 - i)) for i in range(members)]
    sim = Simulation.new(params[0], HipArgs(devices=[0], boundary=RULES[rule]))
    ens = sim.make_ensemble(shape, params)
    rng = np.random.default_rng(1)
    ens.upload(rng.random((members,) + shape, dtype=np.float32),
               (rng.random((members,) + shape, dtype=np.float32) * np.float32(0.5)).astype(np.float32))
    ens.perform_steps(23)
    snap = ens.snapshot()
    u0, v0 = ens.u_views(), ens.result_views()
    assert snap.u_views().tobytes() == u0.tobytes() and snap.result_views().tobytes() == v0.tobytes()
    assert ens.changes_since(snap)["differing"].sum() == 0
    ens.perform_steps(11)
    every = ens.changes_since(snap)
    assert every.shape == (members, 2) and every.dtype == CHANGE_DTYPE
    part = ens.changes_since(snap, 1, 3)
    assert part.tobytes() == every[1:4].tobytes()
    u1, v1 = ens.u_views(), ens.result_views()
    for i in range(members):
        lone = Simulation.new(params[i], HipArgs(devices=[0], boundary=RULES[rule]))
        species = species_from_arrays(lone, u0[i], v0[i])
        kept = species.snapshot()
        species.u.in_out()[0].upload(lone.context, u1[i])
        species.v.in_out()[0].upload(lone.context, v1[i])
        su, sv = species.change_since(kept)
        assert_same(every[i, 0], su, f"member {i} U")
        assert_same(every[i, 1], sv, f"member {i} V")
        assert_same(su, change_ref.change(u1[i], u0[i]), f"member {i} U restated")
        assert_same(sv, change_ref.change(v1[i], v0[i]), f"member {i} V restated")
        lone.context.close()
    # a sub-range copied back: the other members stay as they were
    ens.copy_from(snap, 1, 3)
    u2, v2 = ens.u_views(), ens.result_views()
    for i in range(members):
        want_u, want_v = (u0, v0) if 1 <= i < 4 else (u1, v1)
        assert u2[i].tobytes() == want_u[i].tobytes() and v2[i].tobytes() == want_v[i].tobytes(), i
    # ... and the members that went back take the same steps again
    ens.perform_steps(11)
    assert ens.u_views(1, 3).tobytes() == u1[1:4].tobytes() and ens.result_views(1, 3).tobytes() == v1[1:4].tobytes()
    snap.destroy()
    ens.destroy()
    sim.context.close()


def test_refusals(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    a, b, c = (HipConcentration(sim.context, (20, 30)) for _ in range(3))
    small = HipConcentration(sim.context, (20, 29))
    foreign = HipConcentration(other.context, (20, 30))
    ctx = sim.context

    def refused(call):
        with pytest.raises(capi.GsError) as e:
            call()
        assert e.value.code == capi.GS_ERR_INVALID, e.value

    refused(lambda: compare_fields(ctx, [a], [small]))
    refused(lambda: compare_fields(ctx, [a, small], [b, small]))
    refused(lambda: compare_fields(ctx, [a], [foreign]))
    refused(lambda: compare_fields(ctx, [foreign], [a]))
    refused(lambda: compare_fields(ctx, [], []))
    refused(lambda: compare_fields(ctx, [a] * 5, [b] * 5))
    refused(lambda: copy_fields(ctx, [a], [small]))
    refused(lambda: copy_fields(ctx, [a], [foreign]))
    refused(lambda: copy_fields(ctx, [foreign], [a]))
    refused(lambda: copy_fields(ctx, [], []))
    refused(lambda: copy_fields(ctx, [a, b, c, small, a], [b, c, a, small, c]))
    refused(lambda: copy_fields(ctx, [a], [a]))
    refused(lambda: copy_fields(ctx, [a, b], [b, b]))
    refused(lambda: copy_fields(ctx, [a, a], [b, c]))
    assert compare_fields(ctx, [a], [b])[0].equal          # nothing was written by a refused call
    e = sim.make_ensemble((16, 24), Parameters(), members=4)
    same = sim.make_ensemble((16, 24), Parameters(), members=4, seed=False)
    fewer = sim.make_ensemble((16, 24), Parameters(), members=3)
    wider = sim.make_ensemble((16, 25), Parameters(), members=4)
    far = other.make_ensemble((16, 24), Parameters(), members=4)
    refused(lambda: e.changes_since(same, 3, 2))
    refused(lambda: e.changes_since(same, 4, 1))
    refused(lambda: e.changes_since(same, 0, 0))
    refused(lambda: e.changes_since(fewer))
    refused(lambda: e.changes_since(wider))
    refused(lambda: e.changes_since(far))
    refused(lambda: same.copy_from(e, 2, 3))
    refused(lambda: same.copy_from(fewer))
    refused(lambda: same.copy_from(wider))
    refused(lambda: same.copy_from(far))
    refused(lambda: same.copy_from(same))
    assert e.changes_since(e)["differing"].sum() == 0      # an ensemble against itself: all zeros
    assert e.changes_since(same)["differing"].sum() > 0
    same.copy_from(e)
    assert e.changes_since(same)["differing"].sum() == 0
    sim.context.close()
    other.context.close()


def test_sweep_steady_state(built, tmp_path):
    from grayscott_amd import hdf5_min, sweep

    base = ["--feed", "0.02:0.05:2", "--kill", "0.05:0.062:2", "-r", "64", "-c", "128", "-s", "120"]
    sweep.main(base + ["-o", str(tmp_path / "plain.h5")])
    sweep.main(base + ["--steady-every", "50", "--steady-tol", "1e-3", "-o", str(tmp_path / "steady.h5")])
    assert (tmp_path / "plain.h5").read_bytes() == (tmp_path / "steady.h5").read_bytes()
    assert not (tmp_path / "plain.steady.npz").exists()
    z = np.load(tmp_path / "steady.steady.npz")
    assert list(z["steps"]) == [50, 100, 120] and z["steps"].dtype == np.int64
    for name in ("max_abs", "sum_abs", "sum_sq"):
        assert z[name].shape == (4, 3, 2) and z[name].dtype == np.float64, name
    for name in ("differing", "nonfinite"):
        assert z[name].shape == (4, 3, 2) and z[name].dtype == np.uint64, name
    assert z["settled_step"].shape == (4,) and z["settled_step"].dtype == np.int64
    assert list(z["settled_step"]) == list(sweep.settled_steps([50, 100, 120], z["max_abs"], 1e-3))
    side = json.load(open(tmp_path / "steady.json"))
    assert side["steps"] == 120 and [m["settled_step"] for m in side["members"]] == list(z["settled_step"])
    assert "settled_step" not in json.load(open(tmp_path / "plain.json"))["members"][0]
    # the records are Ensemble.changes_since's: the same run by hand
    args = sweep.parse(base)
    sim = Simulation.new(sweep.member_params(args)[0], HipArgs(devices=[0]))
    ens = sim.make_ensemble((64, 128), sweep.member_params(args))
    snap, done = ens.snapshot(), 0
    for k, at in enumerate([50, 100, 120]):
        ens.perform_steps(at - done)
        done = at
        rec = ens.changes_since(snap)
        for name in change_ref.FIELDS:
            assert rec[name].tobytes() == np.ascontiguousarray(z[name][:, k]).tobytes(), (name, at)
        snap.copy_from(ens)
    assert ens.result_views().tobytes() == hdf5_min.read(str(tmp_path / "steady.h5")).tobytes()
    sim.context.close()
    # any change is within an infinite tolerance: the run ends at the first check
    sweep.main(base + ["--steady-every", "50", "--steady-tol", "inf", "--steady-stop", "-o", str(tmp_path / "stop.h5")])
    side = json.load(open(tmp_path / "stop.json"))
    assert side["steps"] == 50 and [m["settled_step"] for m in side["members"]] == [50] * 4
    z = np.load(tmp_path / "stop.steady.npz")
    assert list(z["steps"]) == [50] and list(z["settled_step"]) == [50] * 4 and z["max_abs"].shape == (4, 1, 2)
    # the seed rectangle is still diffusing: nobody settles within a zero tolerance, and the run goes to its end
    sweep.main(base[:-1] + ["10", "--steady-every", "5", "--steady-tol", "0", "--steady-stop", "--no-fields",
                            "-o", str(tmp_path / "zero.h5")])
    side = json.load(open(tmp_path / "zero.json"))
    assert side["steps"] == 10 and [m["settled_step"] for m in side["members"]] == [-1] * 4
    z = np.load(tmp_path / "zero.steady.npz")
    assert list(z["steps"]) == [5, 10] and list(z["settled_step"]) == [-1] * 4 and (z["max_abs"] > 0).all()


def test_cpp_mirror_changes(built, tmp_path):
    exe = build_program("change_mirror", tmp_path)
    members, rows, cols = 4, 72, 200
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(members), str(rows), str(cols), "31", str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    n = 40 * (2 + 2 * members)
    rec = np.frombuffer(raw[:n], CHANGE_DTYPE)
    v = np.frombuffer(raw[n:], np.float32).reshape(3, rows, cols)
    assert change_ref.same(rec[1], change_ref.change(v[1], v[0]))
    assert v[2].tobytes() == v[1].tobytes()               # restored, then the same steps again
    for i in range(members):
        assert rec[2 + 2 * i].tobytes() == rec[0].tobytes() and rec[3 + 2 * i].tobytes() == rec[1].tobytes(), i
