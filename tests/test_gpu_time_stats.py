"""Time statistics on the GPU (gs_time_stats_*, gs_members_time_stats_*): every raw accumulator and every result plane, bit
pattern for bit pattern, against the numpy restatement of the rule (tests/time_stats_ref.py) -- at the shapes where the kernel
can go wrong, for all 15 group sets, both senses of the threshold, planes salted with the special values; through
Simulation.perform_steps under the clipped and the periodic rule, with a mask, over 1 and 3 slabs; ensembles with a retired
member; and every refusal of include/gs_hip.h with its error code."""
import ctypes

import numpy as np
import pytest

from tests import time_stats_ref as ref

pytestmark = pytest.mark.gpu

T_U, T_V = 0.5, 0.25
ALL_NAMES = ("sum", "squares", "extremes", "crossings")


def both_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert ref.same_bits(got, want), f"{what}: {ref.describe(got, want)}"


def read_plane(ctx, plane):
    a = plane.make_scalar_view(ctx)
    plane.destroy()
    return a


def check_species(ctx, stats, accs, groups, what):
    """Every raw accumulator and every result plane of U and V against the restatement's."""
    for sp in ("u", "v"):
        for name in ref.raw_names(groups):
            both_bits(stats.raw(name, sp), accs[sp].raw(name), f"{what}: raw {name} of {sp}")
        for name in ref.result_names(groups):
            both_bits(read_plane(ctx, getattr(stats, name)(sp)), accs[sp].result(name), f"{what}: {name} of {sp}")


def fresh_accs(shape, groups, above):
    crossing = bool(groups & ref.CROSSINGS)
    return {"u": ref.Accumulators(shape, groups, T_U if crossing else None, above[0]),
            "v": ref.Accumulators(shape, groups, T_V if crossing else None, above[1])}


def make_stats(species, groups, above):
    crossing = bool(groups & ref.CROSSINGS)
    return species.time_stats(groups, v_threshold=T_V if crossing else None, u_threshold=T_U if crossing else None, above=above)


def salted_case(shape, args, groups, above, seed):
    """Six salted samples uploaded into the in-planes and accumulated with the stamps of the issue."""
    from grayscott_amd import Parameters, Simulation
    from tests.helpers import species_from_arrays

    sim = Simulation.new(Parameters(), args)
    ctx = sim.context
    us, vs = ref.sample_planes(shape, seed, T_U), ref.sample_planes(shape, seed + 100, T_V)
    species = species_from_arrays(sim, us[0], vs[0])
    stats = make_stats(species, groups, above)
    accs = fresh_accs(shape, groups, above)
    for k, stamp in enumerate(ref.STAMPS):
        in_u, in_v, _, _ = species.in_out()
        in_u.upload(ctx, us[k])
        in_v.upload(ctx, vs[k])
        stats.accumulate(stamp)
        accs["u"].accumulate(us[k], stamp)
        accs["v"].accumulate(vs[k], stamp)
    assert stats.samples == len(ref.STAMPS)
    check_species(ctx, stats, accs, groups, f"{shape} groups {groups} above {above}")
    stats.close()
    ctx.close()


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (5, 255), (5, 256), (5, 257), (37, 301), (2, 1030)])
@pytest.mark.parametrize("above", [(True, True), (False, False)])
def test_shapes_where_the_kernel_can_go_wrong(built, shape, above):
    from grayscott_amd import HipArgs

    salted_case(shape, HipArgs(devices=[0]), ref.ALL, above, shape[0] * 1000 + shape[1])


@pytest.mark.parametrize("groups", range(1, 16))
def test_every_group_set(built, groups):
    from grayscott_amd import HipArgs

    salted_case((37, 301), HipArgs(devices=[0]), groups, (False, True), 40 + groups)


@pytest.mark.parametrize("layout", ["pitch_pad", "three_slabs"])
def test_padded_rows_and_unequal_slabs(built, layout):
    """``pitch_pad``: a pitch that is no multiple of 64.  It does NOT reach the ragged (VEC = false) kernel form: the library
    rounds the pad up to a multiple of 4, so a field's rows always begin on 16 bytes.  That form is reached through ensembles
    whose column count is no multiple of 4: test_ragged_form_on_wide_members and test_ensembles_with_a_retired_member."""
    from grayscott_amd import HipArgs

    args = HipArgs(devices=[0], pitch_pad=3) if layout == "pitch_pad" else HipArgs(devices=[0, 0, 0])
    salted_case((64, 300), args, ref.ALL, (False, True), 7)


def integration_run(args, mask=None, probe=False):
    """64 x 300: 40 steps, then a sample every 8 steps up to step 200; the restatement is fed with downloads of the same
    states.  Returns the raw accumulators (for the 1-against-3-slabs comparison)."""
    from grayscott_amd import Parameters, Simulation

    shape = (64, 300)
    sim = Simulation.new(Parameters(), args)
    ctx = sim.context
    species = sim.make_species(shape)
    if mask is not None:
        sim.set_mask(mask)
    stats = make_stats(species, ref.ALL, (False, True))
    accs = fresh_accs(shape, ref.ALL, (False, True))
    sim.perform_steps(species, 40)
    for step in range(40, 201, 8):
        if step > 40:
            sim.perform_steps(species, 8)
        in_u, in_v, _, _ = species.in_out()
        u, v = in_u.make_scalar_view(ctx), in_v.make_scalar_view(ctx)
        before = ctx.stats()
        stats.accumulate(step)
        if probe:
            # an accumulate leaves the fields and the context's counters as they were
            after = ctx.stats()
            assert {k: after[k] for k in ("launches", "steps", "passes", "ghost_refreshes")} == \
                {k: before[k] for k in ("launches", "steps", "passes", "ghost_refreshes")}
            assert in_u.make_scalar_view(ctx).tobytes() == u.tobytes() and in_v.make_scalar_view(ctx).tobytes() == v.tobytes()
        accs["u"].accumulate(u, step)
        accs["v"].accumulate(v, step)
    assert stats.samples == 21
    check_species(ctx, stats, accs, ref.ALL, f"integration {args.devices} boundary {args.boundary}")
    raws = {(sp, name): stats.raw(name, sp) for sp in ("u", "v") for name in ref.RAW_GROUP}
    assert accs["v"].result("variance").max() > 0 and (accs["v"].first_stamp != ref.NEVER).any()
    return sim, species, stats, accs, raws


def close(sim, stats):
    stats.close()
    sim.context.close()


def test_integration_clipped_one_and_three_slabs(built):
    from grayscott_amd import HipArgs

    sim, _, stats, _, one = integration_run(HipArgs(devices=[0]), probe=True)
    close(sim, stats)
    sim, _, stats, _, three = integration_run(HipArgs(devices=[0, 0, 0]))
    close(sim, stats)
    for key in one:
        both_bits(three[key], one[key], f"3 slabs against 1: {key}")


def test_integration_periodic(built):
    from grayscott_amd import HipArgs, capi

    sim, _, stats, _, _ = integration_run(HipArgs(devices=[0], boundary=capi.GS_BOUNDARY_PERIODIC))
    close(sim, stats)


def test_integration_with_a_mask(built):
    from grayscott_amd import HipArgs

    mask = np.zeros((64, 300), np.uint8)
    mask[10:50, 140] = 1
    mask[30, 20:120] = 1
    sim, _, stats, _, _ = integration_run(HipArgs(devices=[0]), mask=mask)
    close(sim, stats)


def test_reset_and_observables_of_result_planes(built):
    from grayscott_amd import HipArgs, HipConcentration

    sim, species, stats, accs, _ = integration_run(HipArgs(devices=[0]))
    ctx = sim.context
    # variance("v").summary() and max("v").morphology((0.25,)) equal those of a field uploaded from the restatement's plane
    for name, observe in (("variance", lambda f: f.summary(ctx)), ("max", lambda f: f.morphology(ctx, (0.25,))[0])):
        plane = getattr(stats, name)("v")
        twin = HipConcentration(ctx, (64, 300))
        twin.upload(ctx, accs["v"].result(name))
        got, want = observe(plane), observe(twin)
        if name == "variance":
            assert got == want and got.nonfinite == 0 and got.max > 0
        else:
            assert np.array_equal(got.quads, want.quads) and got.area > 0
        plane.destroy()
        twin.destroy()
    # after reset the object is bit for bit a fresh one
    stats.reset()
    assert stats.samples == 0
    empty = fresh_accs((64, 300), ref.ALL, (False, True))
    for sp in ("u", "v"):
        for name in ref.RAW_GROUP:
            both_bits(stats.raw(name, sp), empty[sp].raw(name), f"after reset: {name} of {sp}")
    in_u, in_v, _, _ = species.in_out()
    u, v = in_u.make_scalar_view(ctx), in_v.make_scalar_view(ctx)
    other = make_stats(species, ref.ALL, (False, True))
    for s in (stats, other):
        s.accumulate(5)
    empty["u"].accumulate(u, 5)
    empty["v"].accumulate(v, 5)
    check_species(ctx, stats, empty, ref.ALL, "after reset and one sample")
    check_species(ctx, other, empty, ref.ALL, "a fresh object after one sample")
    other.close()
    close(sim, stats)


@pytest.mark.parametrize("members,shape", [(5, (9, 30)), (3, (8, 64))])
def test_ensembles_with_a_retired_member(built, members, shape):
    from grayscott_amd import HipArgs, Parameters, Simulation

    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    params = [Parameters(feed_rate=0.014 + 0.004 * i, kill_rate=0.054 + 0.002 * i) for i in range(members)]
    ens = sim.make_ensemble(shape, params)
    rng = np.random.default_rng(members)
    ens.upload(rng.random((members,) + shape, dtype=np.float32), (rng.random((members,) + shape, dtype=np.float32) * np.float32(0.5)))
    stats = ens.time_stats(ALL_NAMES, v_threshold=T_V, u_threshold=T_U, above=(False, True))
    accs = fresh_accs((members,) + shape, ref.ALL, (False, True))
    for k, stamp in enumerate(ref.STAMPS):
        ens.perform_steps(5 + k)
        if k == 3:
            ens.retire([1])                                  # sampled on: it repeats its state
        u, v = ens.u_views(), ens.result_views()
        stats.accumulate(stamp)
        accs["u"].accumulate(u, stamp)
        accs["v"].accumulate(v, stamp)
    assert stats.samples == 6 and not ens.active()[1]
    for sp in ("u", "v"):
        for name in ref.RAW_GROUP:
            both_bits(stats.raw(name, sp), accs[sp].raw(name), f"members: raw {name} of {sp}")
        for name in ref.RESULT_GROUPS:
            both_bits(getattr(stats, name)(sp), accs[sp].result(name), f"members: {name} of {sp}")
    # a range of members: planes 0 / 1 of members [1, 3)
    part = ens.time_stats(("sum", "extremes"), first=1, count=2)
    part.accumulate(1)
    both_bits(part.max("v"), ens.result_views(1, 2), "a member range's maximum after one sample")
    both_bits(part.raw("sum", "u"), ens.u_views(1, 2).astype(np.float64), "a member range's sum after one sample")
    part.close()
    stats.close()
    ens.destroy()
    sim.context.close()


@pytest.mark.parametrize("members,shape", [(3, (5, 301)), (3, (2, 1031)), (3, (1, 2101))])
def test_ragged_form_on_wide_members(built, members, shape):
    """The ragged kernel form (per-column loads and stores) on rows wider than one block of 256 columns: members whose column
    count is no multiple of 4 and whose cells no power of two above it divides, so the plane is scanned as it lies.  301, 1031
    and 2101 columns put the ragged last quad into the second, a later and the first block of an unrolled group and make the
    column loop run once and several times at every unroll depth: one group (8 blocks), two (4), three and four (2)."""
    from grayscott_amd import HipArgs, Parameters, Simulation

    assert shape[1] % 4 != 0 and all((members * shape[0] * shape[1]) % w for w in (512, 1024, 2048, 4096))
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ens = sim.make_ensemble(shape, [Parameters()] * members)
    full = (members,) + shape
    us, vs = ref.sample_planes(full, shape[1], T_U), ref.sample_planes(full, shape[1] + 1, T_V)
    for groups, above in ((1, (True, True)), (4, (True, True)), (8, (False, True)), (3, (True, True)), (12, (True, False)),
                          (7, (True, True)), (15, (False, True)), (15, (True, False))):
        crossing = bool(groups & ref.CROSSINGS)
        stats = ens.time_stats(groups, v_threshold=T_V if crossing else None, u_threshold=T_U if crossing else None, above=above)
        accs = fresh_accs(full, groups, above)
        for k, stamp in enumerate(ref.STAMPS):
            ens.upload(us[k], vs[k])
            stats.accumulate(stamp)
            accs["u"].accumulate(us[k], stamp)
            accs["v"].accumulate(vs[k], stamp)
        for sp in ("u", "v"):
            for name in ref.raw_names(groups):
                both_bits(stats.raw(name, sp), accs[sp].raw(name), f"{shape} groups {groups}: raw {name} of {sp}")
            for name in ref.result_names(groups):
                both_bits(getattr(stats, name)(sp), accs[sp].result(name), f"{shape} groups {groups}: {name} of {sp}")
        stats.close()
    ens.destroy()
    sim.context.close()


def test_the_context_frees_what_is_left(built):
    """Time statistics are owned by their context: closing it frees them, and closing them afterwards is a no-op."""
    from grayscott_amd import HipArgs, Parameters, Simulation

    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = sim.make_species((16, 40))
    kept, closed = species.time_stats(ALL_NAMES, v_threshold=T_V), species.time_stats(("sum",))
    kept.accumulate(1)
    closed.close()
    sim.context.close()
    kept.close()
    with pytest.raises(Exception):
        kept.samples


def test_refusals(built):
    from grayscott_amd import GsError, HipArgs, HipConcentration, Parameters, Simulation, capi

    INV, lib = capi.GS_ERR_INVALID, capi.load()
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    chain = Simulation.new(Parameters(), HipArgs(devices=[0, 0]))
    ctx, h = sim.context, ctypes.c_void_p()
    t, a = (ctypes.c_float * 4)(0.25, 0.25, 0.25, 0.25), (ctypes.c_int32 * 4)(1, 1, 1, 1)
    nan = (ctypes.c_float * 4)(0.25, float("nan"), 0.25, 0.25)

    def create(n, groups, thresholds=t, above=a):
        status = lib.gs_time_stats_create(ctx.handle, ctypes.byref(h), 16, 40, n, groups, thresholds, above)
        assert status != capi.GS_OK and not h.value
        return status

    assert create(2, 0) == INV and create(2, 16) == INV and create(2, 0x80000001) == INV       # groups
    assert create(2, 8, None, a) == INV and create(2, 15, t, None) == INV and create(2, 8, nan) == INV   # crossings
    assert create(0, 1) == INV and create(5, 1) == INV and create(-1, 1) == INV                # planes
    # an allocation failure (1.2 TB of accumulators) is a status code and leaves nothing behind
    status = lib.gs_time_stats_create(ctx.handle, ctypes.byref(h), 100000, 60000, 4, 15, t, a)
    assert status == capi.GS_ERR_NOMEM and not h.value and b"time statistics" in lib.gs_last_error()
    species, foreign = sim.make_species((16, 40)), other.make_species((16, 40))
    small = sim.make_species((16, 44))
    stats = species.time_stats(("sum", "extremes"))
    fields = lambda s, n=2: (ctypes.c_void_p * 4)(*[f.handle for f in s.in_out()[:n]])
    acc = lambda f, n, stamp: lib.gs_time_stats_accumulate(ctx.handle, stats.handle, f, n, stamp)
    assert acc(fields(foreign), 2, 1) == INV and acc(fields(small), 2, 1) == INV               # another context, another shape
    assert acc(fields(species), 1, 1) == INV and acc(fields(species), 3, 1) == INV              # the wrong count
    assert acc(fields(species), 2, 0xFFFFFFFF) == INV                                           # the reserved stamp
    assert lib.gs_time_stats_accumulate(other.context.handle, stats.handle, fields(species), 2, 1) == INV
    out = HipConcentration(ctx, (16, 40))
    result = lambda plane, which, target=out: lib.gs_time_stats_result(ctx.handle, stats.handle, plane, which, target.handle)
    assert result(1, capi.GS_TSTAT_MEAN) == INV                                                 # no sample yet
    assert stats.samples == 0
    stats.accumulate(1)
    assert result(1, capi.GS_TSTAT_MEAN) == capi.GS_OK
    for which in (capi.GS_TSTAT_VARIANCE, capi.GS_TSTAT_OCCUPANCY, capi.GS_TSTAT_ARRIVAL, 6, -1):   # group not selected, no such plane
        assert result(1, which) == INV, which
    assert result(2, capi.GS_TSTAT_MEAN) == INV and result(-1, capi.GS_TSTAT_MIN) == INV
    assert result(1, capi.GS_TSTAT_MEAN, foreign.in_out()[0]) == INV and result(1, capi.GS_TSTAT_MEAN, small.in_out()[0]) == INV
    buf = np.zeros((16, 40), np.float64)
    raw = lambda plane, which: lib.gs_time_stats_download(ctx.handle, stats.handle, plane, which, buf.ctypes.data_as(ctypes.c_void_p))
    assert raw(0, capi.GS_TSTAT_RAW_SUM) == capi.GS_OK
    assert lib.gs_time_stats_download(ctx.handle, stats.handle, 0, capi.GS_TSTAT_RAW_SUM, None) == INV
    for which in (capi.GS_TSTAT_RAW_SQUARES, capi.GS_TSTAT_RAW_SET_COUNT, capi.GS_TSTAT_RAW_FIRST_STAMP, 6, -1):
        assert raw(0, which) == INV, which
    assert raw(2, capi.GS_TSTAT_RAW_SUM) == INV
    with pytest.raises(GsError) as e:
        stats.variance("v")
    assert e.value.code == INV
    # the forms do not mix; members outside the ensemble; an ensemble of another shape
    ens = sim.make_ensemble((16, 40), [Parameters()] * 3)
    assert lib.gs_members_time_stats_accumulate(ctx.handle, stats.handle, ens.handle, 1) == INV
    assert lib.gs_members_time_stats_result(ctx.handle, stats.handle, 0, 0, buf.ctypes.data_as(ctypes.c_void_p)) == INV
    mcreate = lambda e, first, count, groups=1, th=t, ab=a: lib.gs_members_time_stats_create(
        ctx.handle, ctypes.byref(h), e, first, count, groups, th, ab)
    assert mcreate(ens.handle, 2, 2) == INV and mcreate(ens.handle, 0, 0) == INV and mcreate(None, 0, 1) == INV and not h.value
    assert mcreate(ens.handle, 0, 3, 0) == INV and mcreate(ens.handle, 0, 3, 8, None, None) == INV and not h.value
    mstats = ens.time_stats(("sum",))
    assert lib.gs_time_stats_accumulate(ctx.handle, mstats.handle, fields(species), 2, 1) == INV
    assert lib.gs_time_stats_result(ctx.handle, mstats.handle, 0, 0, out.handle) == INV
    wide = sim.make_ensemble((16, 44), [Parameters()] * 3)
    few = sim.make_ensemble((16, 40), [Parameters()] * 2)
    for e in (wide, few):
        assert lib.gs_members_time_stats_accumulate(ctx.handle, mstats.handle, e.handle, 1) == INV
    assert lib.gs_members_time_stats_accumulate(ctx.handle, mstats.handle, ens.handle, 0xFFFFFFFF) == INV
    assert lib.gs_members_time_stats_result(ctx.handle, mstats.handle, 0, 0, buf.ctypes.data_as(ctypes.c_void_p)) == INV   # no sample
    assert mstats.samples == 0
    # an ensemble on a context that refuses ensembles: that context's own error
    with pytest.raises(GsError) as e:
        chain.make_ensemble((16, 40), [Parameters()] * 2)
    status = lib.gs_members_time_stats_create(chain.context.handle, ctypes.byref(h), None, 0, 1, 1, t, a)
    assert status == e.value.code == capi.GS_ERR_UNSUPPORTED and not h.value
    # destroyed with another context: refused, and the object lives on
    assert lib.gs_time_stats_destroy(other.context.handle, stats.handle) == INV
    assert stats.samples == 1
    for x in (mstats, stats):
        x.close()
    for e in (ens, wide, few):
        e.destroy()
    for s in (sim, other, chain):
        s.context.close()
