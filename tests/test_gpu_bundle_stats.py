"""Bundle statistics on the GPU (gs_members_bundle_stats): every result plane, bit pattern for bit pattern (NaN sign and
payload aside, as for the time statistics), against the numpy restatement of the rule (tests/bundle_stats_ref.py) -- at the
shapes where the kernel can go wrong, for spans shorter and longer than its load-ahead depth, from a first member that
misaligns the bases, into result ensembles that hold a canary; every code alone and all together; held to the time
statistics of a one-member ensemble; with retired members; the results as ordinary ensembles, stepped with an active set in
force; a noisy ensemble against tests/noise_ref.py; the sweep's --bundle-stats end to end; and every refusal with its code."""
import ctypes
import functools
import json
import sys

import numpy as np
import pytest

from tests import bundle_stats_ref as ref
from tests.children import ROOT, run_program

pytestmark = pytest.mark.gpu

T_U, T_V = 0.5, 0.25
ABOVE = (False, True)                       # U is set below its threshold, V above
CANARY_U, CANARY_V = np.float32(123.25), np.float32(-77.5)
SHAPES = [(5, 7), (37, 53), (64, 128), (100, 300)]
SPANS = [1, 2, 3, 7, 33]


def both_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert ref.same_bits(got, want), f"{what}: {ref.describe(got, want)}"


@functools.lru_cache(maxsize=None)
def members_of(shape, count, span, seed):
    """U and V of ``count`` members (bundles of ``span``): helpers.stress_fields with the special values planted.  Shared, read-only."""
    from tests.helpers import stress_fields

    u, v = stress_fields((count,) + shape, seed)
    ref.plant(u, span, seed, T_U)
    ref.plant(v, span, seed + 1, T_V)
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


@functools.lru_cache(maxsize=None)
def restated(shape, count, span, seed, above=ABOVE):
    u, v = members_of(shape, count, span, seed)
    return {"u": ref.bundles(u, span, T_U, above[0]), "v": ref.bundles(v, span, T_V, above[1])}


@pytest.fixture(scope="module")
def sim(built):
    from grayscott_amd import HipArgs, Parameters, Simulation

    s = Simulation.new(Parameters(), HipArgs(devices=[0]))
    yield s
    s.context.close()


def canaries(sim, names, members, shape):
    from grayscott_amd import Ensemble

    out = {}
    for name in names:
        out[name] = Ensemble(sim.context, members, shape)
        out[name].upload(np.full((members,) + shape, CANARY_U), np.full((members,) + shape, CANARY_V))
    return out


def hold_canary(e, members, what):
    u, v = e.u_views(), e.result_views()
    for m in members:
        assert (u[m] == CANARY_U).all() and (v[m] == CANARY_V).all(), f"{what}: member {m} lost its canary"


def destroy(*ensembles):
    for e in ensembles:
        e.destroy()


def loaded(sim, shape, pad, count, span, seed):
    """An ensemble of ``pad`` members of ones in front of the ``count`` members of members_of."""
    from grayscott_amd import Parameters

    u, v = members_of(shape, count, span, seed)
    ens = sim.make_ensemble(shape, Parameters(), seed=False, members=pad + count)
    if pad:
        ens.upload(np.ones((pad,) + shape, np.float32), np.ones((pad,) + shape, np.float32))
    ens.upload(u, v, first=pad)
    return ens


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_spans_and_offsets(sim, shape, span):
    """Two bundles from member 1 on (on the odd shapes the first member's base is then misaligned), all five results together
    into members 2, 3 of result ensembles of 5 that hold a canary; then every code alone, which gives the same bits."""
    count, seed = 2 * span, 100 * span + shape[1]
    want = restated(shape, count, span, seed)
    ens = loaded(sim, shape, 1, count, span, seed)
    out = canaries(sim, ref.RESULTS, 5, shape)
    got = ens.bundle_stats(span, ref.RESULTS, v_threshold=T_V, u_threshold=T_U, above=ABOVE, first=1, count=count, out=out,
                           out_first=2)
    assert sorted(got) == sorted(ref.RESULTS) and all(got[name] is out[name] for name in ref.RESULTS)
    together = {}
    for name in ref.RESULTS:
        hold_canary(out[name], (0, 1, 4), f"{name} of {shape} span {span}")
        together[name] = (out[name].u_views(2, 2), out[name].result_views(2, 2))
        both_bits(together[name][0], want["u"][name], f"{name} of U, {shape} span {span}")
        both_bits(together[name][1], want["v"][name], f"{name} of V, {shape} span {span}")
    for name in ref.RESULTS:
        alone = ens.bundle_stats(span, (name,), v_threshold=T_V, u_threshold=T_U, above=ABOVE, first=1, count=count)
        assert list(alone) == [name] and alone[name].members == 2
        both_bits(alone[name].u_views(), together[name][0], f"{name} of U alone, {shape} span {span}")
        both_bits(alone[name].result_views(), together[name][1], f"{name} of V alone, {shape} span {span}")
        destroy(alone[name])
    destroy(ens, *out.values())


@pytest.mark.parametrize("above", [(True, True), (True, False), (False, False)])
def test_occupancy_senses(sim, above):
    shape, span, count, seed = (37, 53), 7, 14, 5
    want = restated(shape, count, span, seed, above)
    ens = loaded(sim, shape, 0, count, span, seed)
    got = ens.bundle_stats(span, "occupancy", v_threshold=T_V, u_threshold=T_U, above=above)["occupancy"]
    both_bits(got.u_views(), want["u"]["occupancy"], f"occupancy of U, above {above}")
    both_bits(got.result_views(), want["v"]["occupancy"], f"occupancy of V, above {above}")
    # a species without a threshold is never set
    bare = ens.bundle_stats(span, "occupancy", v_threshold=T_V)["occupancy"]
    assert not bare.u_views().any()
    both_bits(bare.result_views(), restated(shape, count, span, seed, (True, True))["v"]["occupancy"], "occupancy of V alone")
    destroy(ens, got, bare)


@pytest.mark.parametrize("shape,span", [((37, 53), 5), ((64, 128), 33)])
def test_one_bundle_of_the_whole_ensemble(sim, shape, span):
    want = restated(shape, span, span, 9)
    ens = loaded(sim, shape, 0, span, span, 9)
    got = ens.bundle_stats(span, ref.RESULTS, v_threshold=T_V, u_threshold=T_U, above=ABOVE)
    for name in ref.RESULTS:
        assert got[name].members == 1
        both_bits(got[name].u_views(), want["u"][name], f"{name} of U, one bundle of {span}")
        both_bits(got[name].result_views(), want["v"][name], f"{name} of V, one bundle of {span}")
    destroy(ens, *got.values())


def test_held_to_the_time_statistics(sim):
    """A bundle's planes are the time statistics of a one-member ensemble sampled through the bundle's members in order."""
    from grayscott_amd import Parameters

    shape, span, count, seed = (37, 53), 7, 14, 21
    u, v = members_of(shape, count, span, seed)
    ens = loaded(sim, shape, 0, count, span, seed)
    got = ens.bundle_stats(span, ref.RESULTS, v_threshold=T_V, u_threshold=T_U, above=ABOVE)
    solo = sim.make_ensemble(shape, Parameters(), seed=False, members=1)
    for b in range(2):
        stats = solo.time_stats(("sum", "squares", "extremes", "crossings"), v_threshold=T_V, u_threshold=T_U, above=ABOVE)
        for j in range(span):
            m = b * span + j
            solo.upload(u[m:m + 1], v[m:m + 1])
            stats.accumulate(j)
        assert stats.samples == span
        for name in ref.RESULTS:
            both_bits(got[name].u_views(b, 1), getattr(stats, name)("u"), f"{name} of U of bundle {b} against the time statistics")
            both_bits(got[name].result_views(b, 1), getattr(stats, name)("v"), f"{name} of V of bundle {b} against the time statistics")
        stats.close()
    destroy(ens, solo, *got.values())


def test_retired_members_contribute_their_retained_state(sim):
    from grayscott_amd import Parameters

    shape = (16, 32)
    params = [Parameters(feed_rate=0.014 + 0.004 * i, kill_rate=0.054 + 0.002 * i) for i in range(6)]
    ens = sim.make_ensemble(shape, params)
    ens.perform_steps(10)
    ens.retire([1, 4])
    ens.perform_steps(11)
    assert list(ens.active()) == [True, False, True, True, False, True]
    u, v = ens.u_views(), ens.result_views()
    got = ens.bundle_stats(3, ref.RESULTS, v_threshold=T_V, u_threshold=T_U, above=ABOVE)
    for name in ref.RESULTS:
        both_bits(got[name].u_views(), ref.bundles(u, 3, T_U, ABOVE[0])[name], f"{name} of U with retired members")
        both_bits(got[name].result_views(), ref.bundles(v, 3, T_V, ABOVE[1])[name], f"{name} of V with retired members")
    # the call leaves the members, their flags and their step counts as they were
    assert ens.u_views().tobytes() == u.tobytes() and ens.result_views().tobytes() == v.tobytes()
    assert list(ens.steps_taken()) == [21, 10, 21, 21, 10, 21]
    destroy(ens, *got.values())


def test_results_are_ordinary_ensembles(sim):
    from grayscott_amd import Parameters
    from tests import summary_ref

    shape, span, count, seed = (37, 53), 3, 12, 33
    want = restated(shape, count, span, seed)
    ens = loaded(sim, shape, 0, count, span, seed)
    mean = ens.bundle_stats(span, "mean")["mean"]
    s = mean.summaries()
    for b in range(count // span):
        assert summary_ref.same(s[b, 0], summary_ref.summary(want["u"]["mean"][b])), f"summary of the mean of U, bundle {b}"
        assert summary_ref.same(s[b, 1], summary_ref.summary(want["v"]["mean"][b])), f"summary of the mean of V, bundle {b}"
    destroy(mean)
    # written into an ensemble with an active set in force, whose slots have diverged: the stale / mirror bookkeeping
    params = [Parameters(feed_rate=0.02 + 0.005 * i, kill_rate=0.055 + 0.002 * i) for i in range(4)]
    smooth = sim.make_ensemble(shape, params)        # finite members, so that the steps that follow mean something
    smooth.perform_steps(4)
    members = np.concatenate([smooth.u_views()] * 3), np.concatenate([smooth.result_views()] * 3)
    members[0][1::3] *= np.float32(0.5)
    members[1][2::3] += np.float32(0.125)
    src = sim.make_ensemble(shape, Parameters(), seed=False, members=12)
    src.upload(*members)
    res, twin = sim.make_ensemble(shape, params), sim.make_ensemble(shape, params)
    for e in (res, twin):
        e.set_active(np.array([1, 0, 1, 0], np.uint8))
        e.perform_steps(5)
    got = src.bundle_stats(3, "mean", out={"mean": res})
    assert got["mean"] is res
    planes = res.u_views(), res.result_views()
    both_bits(planes[0], ref.bundles(members[0], 3)["mean"], "the mean of U written into an ensemble with an active set")
    both_bits(planes[1], ref.bundles(members[1], 3)["mean"], "the mean of V written into an ensemble with an active set")
    twin.upload(*planes)
    assert list(res.active()) == list(twin.active()) == [True, False, True, False]
    assert list(res.steps_taken()) == list(twin.steps_taken()) == [5, 0, 5, 0]
    for e in (res, twin):
        e.perform_steps(3)
    assert res.u_views().tobytes() == twin.u_views().tobytes() and res.result_views().tobytes() == twin.result_views().tobytes()
    both_bits(res.u_views(1, 1), planes[0][1:2], "an inactive result member keeps the plane written into it")
    assert not np.array_equal(res.u_views(0, 1), planes[0][0:1])
    for e in (res, twin):
        e.reactivate([1, 3])
        e.perform_steps(2)
    assert res.u_views().tobytes() == twin.u_views().tobytes() and res.result_views().tobytes() == twin.result_views().tobytes()
    destroy(ens, smooth, src, res, twin)


def test_noisy_ensemble_end_to_end(sim):
    """4 realisations of 3 parameter points of 16 x 32 after 20 steps, against the restatement over tests/noise_ref.py's members."""
    import oracle
    from grayscott_amd import Parameters
    from tests import noise_ref as N
    from tests.helpers import oracle_params

    shape, reps, steps = (16, 32), 4, 20
    points = [Parameters(feed_rate=0.02 + 0.01 * i, kill_rate=0.055 + 0.003 * i) for i in range(3)]
    params = [p for p in points for _ in range(reps)]
    ens = sim.make_ensemble(shape, params)
    ens.set_noise(0.02, 0.01, seed=np.array([40 + i % reps for i in range(len(params))], np.uint64))
    ens.perform_steps(steps)
    u0, v0 = oracle.init_species(*shape)
    runs = [N.run(u0, v0, steps, dict(sigma_u=np.float32(0.02), sigma_v=np.float32(0.01), seed=40 + i % reps, step=0),
                  params=oracle_params(p)) for i, p in enumerate(params)]
    u, v = np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs])
    assert ens.u_views().tobytes() == u.tobytes() and ens.result_views().tobytes() == v.tobytes()
    got = ens.bundle_stats(reps, ref.RESULTS, v_threshold=T_V, u_threshold=T_U, above=ABOVE)
    for name in ref.RESULTS:
        assert got[name].members == 3
        both_bits(got[name].u_views(), ref.bundles(u, reps, T_U, ABOVE[0])[name], f"{name} of U of the noisy ensemble")
        both_bits(got[name].result_views(), ref.bundles(v, reps, T_V, ABOVE[1])[name], f"{name} of V of the noisy ensemble")
    assert got["variance"].result_views().max() > 0                       # the realisations differ
    destroy(ens, *got.values())


def test_sweep_end_to_end(sim, tmp_path):
    from grayscott_amd import hdf5_min, sweep

    base = ["--feed", "0.02:0.04:2", "--kill", "0.055:0.062:2", "-r", "16", "-c", "32", "-s", "12", "--realisations", "4",
            "--noise", "0.01:0.005", "--noise-seed", "7"]
    flags = ["--bundle-stats", "--bundle-threshold-v", "0.25"]
    for d, extra in (("a", flags), ("b", flags), ("c", []), ("d", flags + ["--no-fields"])):
        (tmp_path / d).mkdir()
        r = run_program([sys.executable, "-m", "grayscott_amd.sweep"] + base + extra + ["-o", str(tmp_path / d / "run.h5")],
                        cwd=ROOT, limit=300)
        assert r.returncode == 0, r.stderr
    read = lambda d, name: open(tmp_path / d / name, "rb").read()
    # twice: byte-identical; with --no-fields: the same file, and no HDF5 file
    assert read("a", "run.bundles.npz") == read("b", "run.bundles.npz") == read("d", "run.bundles.npz")
    assert not (tmp_path / "d" / "run.h5").exists()
    # without the flag: no such file, the HDF5 file is the same bytes and the sidecar lacks the one key
    assert not (tmp_path / "c" / "run.bundles.npz").exists() and read("c", "run.h5") == read("a", "run.h5")
    side = json.load(open(tmp_path / "a" / "run.json"))
    assert side.pop("bundle_stats") == {"file": "run.bundles.npz", "span": 4, "threshold_v": 0.25}
    assert read("c", "run.json").decode() == json.dumps(side, indent=1)
    # the planes: V from the final planes in the HDF5 file, U from the same run made here
    v = hdf5_min.read(str(tmp_path / "a" / "run.h5"))
    args = sweep.parse(base + flags + ["-o", str(tmp_path / "e" / "run.h5")])
    ens = sim.make_ensemble((16, 32), sweep.member_params(args))
    ens.set_noise(args.noise[0], args.noise[1], seed=np.array([seed for _, seed in sweep.member_seeds(args)], np.uint64))
    ens.perform_steps(12)
    assert ens.result_views().tobytes() == v.tobytes()
    u = ens.u_views()
    destroy(ens)
    want_u, want_v = ref.bundles(u, 4), ref.bundles(v, 4, 0.25, True)
    with np.load(tmp_path / "a" / "run.bundles.npz") as z:
        assert sorted(z.files) == sorted(["mean_u", "mean_v", "variance_u", "variance_v", "min_v", "max_v", "occupancy_v", "feed",
                                          "kill", "span"])
        for name in ("mean", "variance", "min", "max", "occupancy"):
            both_bits(z[name + "_v"], want_v[name], f"{name}_v of the sweep")
        for name in ("mean", "variance"):
            both_bits(z[name + "_u"], want_u[name], f"{name}_u of the sweep")
        assert z["mean_v"].shape == (4, 16, 32) and int(z["span"]) == 4
        assert list(z["feed"]) == [0.02, 0.04, 0.02, 0.04] and list(z["kill"]) == [0.055, 0.055, 0.062, 0.062]


def test_refusals(sim):
    from grayscott_amd import Ensemble, GsError, HipArgs, Parameters, Simulation, capi

    INV, lib, ctx = capi.GS_ERR_INVALID, capi.load(), sim.context
    shape = (16, 40)
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    chain = Simulation.new(Parameters(), HipArgs(devices=[0, 0]))
    ens = sim.make_ensemble(shape, Parameters(), members=8)
    outs = canaries(sim, ("a", "b", "c", "d", "e", "f"), 4, shape)
    a, b = outs["a"], outs["b"]
    wide, short, foreign = Ensemble(ctx, 4, (16, 44)), Ensemble(ctx, 3, shape), Ensemble(other.context, 4, shape)
    t, ab = (ctypes.c_float * 2)(T_U, T_V), (ctypes.c_int32 * 2)(0, 1)
    nan = (ctypes.c_float * 2)(T_U, float("nan"))
    MEAN, VAR, OCC, ARR = capi.GS_TSTAT_MEAN, capi.GS_TSTAT_VARIANCE, capi.GS_TSTAT_OCCUPANCY, capi.GS_TSTAT_ARRIVAL

    def call(first=0, count=8, span=2, which=(MEAN, VAR), thresholds=t, above=ab, out=(a, b), out_first=0, e=ens, context=ctx,
             n=None, null_which=False, null_out=False):
        codes = (ctypes.c_int32 * max(len(which), 1))(*which)
        targets = (ctypes.c_void_p * max(len(out), 1))(*[None if o is None else o.handle.value for o in out])
        status = lib.gs_members_bundle_stats(context.handle, None if e is None else e.handle, first, count, span,
                                             None if null_which else codes, len(which) if n is None else n, thresholds, above,
                                             None if null_out else targets, out_first)
        if status != capi.GS_OK:
            for o in outs.values():
                hold_canary(o, range(4), "after a refusal")
        return status

    def refill():
        for o in (a, b):
            assert not (o.u_views() == CANARY_U).all()
            o.upload(np.full((4,) + shape, CANARY_U), np.full((4,) + shape, CANARY_V))

    # a null argument
    assert call(e=None) == INV and call(null_which=True) == INV and call(null_out=True) == INV and call(out=(a, None)) == INV
    # a bad span, a count that is no multiple of it
    assert call(span=0) == INV and call(count=7, span=2) == INV and call(count=8, span=3) == INV
    # a range outside the ensemble
    assert call(first=2, count=8) == INV and call(first=8, count=2) == INV and call(first=9, count=0) == INV
    assert call(first=2 ** 63, count=2 ** 63, span=2 ** 62) == INV
    # n outside 1..5, an unknown or repeated code, ARRIVAL
    assert call(which=(), out=()) == INV and call(n=6) == INV and call(n=-1) == INV
    assert call(which=(MEAN, VAR, 2, 3, OCC, MEAN), out=tuple(outs.values())) == INV
    assert call(which=(MEAN, MEAN)) == INV and call(which=(MEAN, ARR)) == INV and call(which=(6, MEAN)) == INV
    assert call(which=(-1,), out=(a,)) == INV
    # the occupancy without thresholds, or with a NaN threshold
    assert call(which=(OCC,), out=(a,), thresholds=None) == INV and call(which=(OCC,), out=(a,), above=None) == INV
    assert call(which=(MEAN, OCC), thresholds=nan) == INV
    assert call(thresholds=None, above=None) == capi.GS_OK                       # ignored without the occupancy ...
    refill()
    # out[i]: the source itself, named twice, of another shape or context, too short
    assert call(out=(a, ens)) == INV and call(out=(a, a)) == INV and call(out=(a, wide)) == INV and call(out=(foreign, b)) == INV
    assert call(out=(a, short)) == INV and call(out_first=1) == INV and call(out_first=2 ** 64 - 1) == INV
    assert call(count=4, out_first=2) == capi.GS_OK                              # ... and this fits: members 2, 3
    for o in (a, b):
        hold_canary(o, (0, 1), "in front of the members written")
    refill()
    # an ensemble or a context of another kind
    assert call(context=other.context) == INV
    assert call(e=None, context=chain.context) == capi.GS_ERR_UNSUPPORTED
    # count == 0: GS_OK, nothing is written
    assert call(count=0) == capi.GS_OK and call(first=8, count=0) == capi.GS_OK
    for o in outs.values():
        hold_canary(o, range(4), "after a call for no members")
    # the Python method: the code and nothing left behind; names it does not know
    with pytest.raises(GsError) as err:
        ens.bundle_stats(3)
    assert err.value.code == INV
    with pytest.raises(GsError) as err:
        ens.bundle_stats(2, "occupancy")
    assert err.value.code == INV
    with pytest.raises(ValueError):
        ens.bundle_stats(2, "arrival")
    destroy(ens, wide, short, foreign, *outs.values())
    other.context.close()
    chain.context.close()
