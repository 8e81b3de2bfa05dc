"""Regional state comparison on the device (gs_fields_region_compare) against its definition (tests/region_change_ref.py):
every region cropped from both planes and handed to the whole-grid restatement.  Every case runs under both forced routes
(GS_HIP_REGION_CHANGE_ROUTE = records, wave) and under the library's own choice, and every region is bit-equal to the
reference by change_ref.same -- sums and the maximum as f64 bit patterns, equal counts."""
import contextlib
import os

import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, RegionChange, Simulation, capi
from grayscott_amd.simulation import compare_fields, region_compare_fields, region_grid
from tests import change_ref, region_change_ref, regions_ref
from tests.helpers import species_from_arrays, stress_fields

pytestmark = pytest.mark.gpu

ROUTES = ("records", "wave", None)  # None: the library's choice
VARIABLE = "GS_HIP_REGION_CHANGE_ROUTE"


@contextlib.contextmanager
def route(name):
    """The route switch for the calls inside (the library reads it at every call)."""
    before = os.environ.get(VARIABLE)
    if name is None:
        os.environ.pop(VARIABLE, None)
    else:
        os.environ[VARIABLE] = name
    try:
        yield
    finally:
        if before is None:
            os.environ.pop(VARIABLE, None)
        else:
            os.environ[VARIABLE] = before


def assert_changes(got: RegionChange, want, shape, region, what):
    assert got.sum_abs.shape == want.shape and got.shape == tuple(shape) and got.region == regions_ref.shape_of(region), what
    assert np.array_equal(got.size, regions_ref.sizes(shape, region)), what
    assert got.differing.dtype == got.nonfinite.dtype == np.uint64 and got.sum_abs.dtype == np.float64, what
    for at in np.ndindex(want.shape):
        assert change_ref.same(got.at(*at), want[at]), f"{what}: region {at}: {change_ref.as_dict(got.at(*at))}, not {change_ref.as_dict(want[at])}"


def check_pair(ctx, fa, fb, a, b, region, what):
    """Plane a against plane b under every route; the reference is formed once."""
    fa.upload(ctx, a)
    fb.upload(ctx, b)
    want = region_change_ref.changes(a, b, region)
    for name in ROUTES:
        with route(name):
            assert_changes(fa.region_change_from(ctx, fb, region), want, a.shape, region, f"{what}, route {name}")
    return want


NAN2 = np.array([0x7fc00001], np.uint32).view(np.float32)[0]
NAN3 = np.array([0xffc00002], np.uint32).view(np.float32)[0]
SPECIAL = [(np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.inf, np.inf), (np.inf, -np.inf), (-np.inf, 2.0), (0.0, -0.0),
           (-0.0, 0.0), (1e-45, -1e-45), (-1e-45, -1e-45), (1e-40, 3e-39), (NAN2, NAN2), (NAN2, NAN3), (2.0 ** 80, -2.0 ** 80),
           (2.0 ** 80, 1.0), (1.0, 1.0)]


def special_pair(shape, seed):
    """Order-sensitive planes with NaN, +-inf, sub-normals, +0 against -0 and NaNs of equal and of different payload planted
    at random cells (about one cell in twelve)."""
    a, b = change_ref.order_sensitive(shape, seed)
    rng = np.random.default_rng(seed + 1000)
    size = a.size
    pos = rng.choice(size, size=max(min(size // 12, 6 * len(SPECIAL)), min(size, 4)), replace=False)
    for k, p in enumerate(pos):
        a.flat[p], b.flat[p] = SPECIAL[(k + seed) % len(SPECIAL)]
    return a, b


def pairs_for(shape, seed):
    yield "order-sensitive", change_ref.order_sensitive(shape, seed)
    yield "special", special_pair(shape, seed + 1)
    u, v = stress_fields(shape, seed + 2)
    yield "a == b", (u, u.copy())


# ---- columns: the column cases of tests/test_gpu_regions.py --------------------------------------------------------------------
COLUMN_CASES = [((5, 16), 16), ((5, 40), 16), ((3, 263), 16), ((3, 263), 64), ((3, 263), 256), ((3, 263), 260), ((4, 256), 16),
                ((4, 256), 256), ((3, 257), 256), ((2, 1025), 252), ((2, 1025), 512), ((6, 531), 132)]


@pytest.mark.parametrize("shape,rw", COLUMN_CASES)
def test_columns(built, shape, rw):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    fa, fb = HipConcentration(sim.context, shape), HipConcentration(sim.context, shape)
    for rh in (2, shape[0]):
        for kind, (a, b) in pairs_for(shape, 7 * rw + shape[1]):
            check_pair(sim.context, fa, fb, a, b, (rh, rw), f"{kind} {shape} ({rh}, {rw})")
    sim.context.close()


# ---- rows: ragged last region rows of one row and of none, around the unroll depth and around the band height ------------------
B_VALUES = (region_change_ref.UNROLL, region_change_ref.BAND)
ROW_HEIGHTS = sorted({rh for B in B_VALUES for rh in (1, 2, B - 1, B, B + 1)})


@pytest.mark.parametrize("rh", ROW_HEIGHTS)
def test_rows(built, rh):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    for rows in (2 * rh + 1, 3 * rh):
        shape = (rows, 300)
        fa, fb = HipConcentration(sim.context, shape), HipConcentration(sim.context, shape)
        for rw in (64, 256, 260):                                        # the narrow branch, its widest region, the wide branch
            for kind, (a, b) in pairs_for(shape, rh):
                check_pair(sim.context, fa, fb, a, b, (rh, rw), f"{kind} {shape} ({rh}, {rw})")
    sim.context.close()


def test_regions_of_several_bands_and_the_librarys_choice(built):
    """Regions of two bands and more, ragged in the last band: where the library itself takes the record route."""
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    B = region_change_ref.BAND
    for shape, region in (((5 * B + 3, 300), (2 * B, 64)), ((5 * B + 3, 300), (2 * B + 1, 256)), ((4 * B, 531), (3 * B - 1, 132)),
                          ((3 * B + 1, 1025), (10 ** 6, 512))):
        fa, fb = HipConcentration(sim.context, shape), HipConcentration(sim.context, shape)
        a, b = special_pair(shape, shape[0])
        check_pair(sim.context, fa, fb, a, b, region, f"{shape} {region}")
    sim.context.close()


# ---- contents ------------------------------------------------------------------------------------------------------------------
def test_a_wrong_fold_order_would_show(built):
    """On the order-sensitive planes of these seeds plain ascending column order gives other bits in at least half of the
    regions (a ragged region of five columns folds the same way in both orders): the device agrees with the rule, not with
    that order."""
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    for shape, region, seed in (((37, 1029), (16, 256), 4), ((37, 1029), (8, 64), 5), ((40, 600), (32, 512), 6)):
        a, b = change_ref.order_sensitive(shape, seed)
        fa, fb = HipConcentration(sim.context, shape), HipConcentration(sim.context, shape)
        want = check_pair(sim.context, fa, fb, a, b, region, f"{shape} {region}")
        wrong = 0
        for (at, ca), (_, cb) in zip(regions_ref.crops(a, region), regions_ref.crops(b, region)):
            other = change_ref.ascending(ca, cb)
            wrong += (change_ref.bits(other["sum_abs"]) != change_ref.bits(want[at]["sum_abs"])
                      or change_ref.bits(other["sum_sq"]) != change_ref.bits(want[at]["sum_sq"]))
        assert 2 * wrong >= want.size, (shape, region, wrong, want.size)
    sim.context.close()


def test_special_cells_are_counted_and_skipped(built):
    shape, region = (37, 1029), (8, 132)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    fa, fb = HipConcentration(sim.context, shape), HipConcentration(sim.context, shape)
    a, b = special_pair(shape, 3)
    want = check_pair(sim.context, fa, fb, a, b, region, "special")
    assert want["nonfinite"].sum() > 0 and np.all(np.isfinite(want["sum_abs"])) and np.all(np.isfinite(want["sum_sq"]))
    # a region whose only comparable cell is a pair of sub-normals, one with none, +0 against -0, NaNs of two payloads
    a = np.full(shape, np.nan, np.float32)
    b = np.full(shape, np.inf, np.float32)
    a[1, 5], b[1, 5] = 1e-45, -1e-45
    a[8:16, 132:264], b[8:16, 132:264] = 0.0, -0.0
    a[16:24, 0:132], b[16:24, 0:132] = NAN2, NAN2
    a[16:24, 132:264], b[16:24, 132:264] = NAN2, NAN3
    want = check_pair(sim.context, fa, fb, a, b, region, "planted regions")
    with route(None):
        got = fa.region_change_from(sim.context, fb, region)
    assert got.at(0, 0).comparable == 1 and got.at(0, 0).max_abs == got.at(0, 0).sum_abs == 2.0 ** -148
    assert got.at(0, 1).comparable == 0 and change_ref.bits(got.at(0, 1).max_abs) == 0 and got.at(0, 1).differing == 8 * 132
    assert got.at(1, 1).differing == 8 * 132 and got.at(1, 1).nonfinite == 0 and got.at(1, 1).max_abs == 0.0
    assert got.at(2, 0).differing == 0 and got.at(2, 0).nonfinite == 8 * 132
    assert got.at(2, 1).differing == 8 * 132 and got.at(2, 1).nonfinite == 8 * 132
    steady = got.steady(1.0)                                             # +0 against -0 moves by 0.0: the only steady region
    assert steady.shape == want.shape and steady[1, 1] and steady.sum() == 1
    # a plane against itself: all zeros, whatever it holds
    for name in ROUTES:
        with route(name):
            zero = fa.region_change_from(sim.context, fa, region)
        assert not zero.sum_abs.any() and not zero.sum_sq.any() and not zero.max_abs.any() and not zero.differing.any(), name
        assert np.array_equal(zero.nonfinite, region_change_ref.changes(a, a, region)["nonfinite"]), name
    sim.context.close()


# ---- invariants ----------------------------------------------------------------------------------------------------------------
def test_invariants_against_the_whole_grid_comparison(built):
    shape = (83, 531)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    a, b = special_pair(shape, 12)
    fa, fb = HipConcentration(sim.context, shape), HipConcentration(sim.context, shape)
    fa.upload(sim.context, a)
    fb.upload(sim.context, b)
    whole = compare_fields(sim.context, [fa], [fb])[0]
    assert change_ref.same(whole, change_ref.change(a, b))
    for name in ROUTES:
        with route(name):
            for region in ((shape[0], 532), (83, 1024), (1000, 2 ** 31 - 4), 2 ** 31 - 4):   # one region covers the grid
                one = fa.region_change_from(sim.context, fb, region)
                assert one.sum_abs.shape == (1, 1) and change_ref.same(one.at(0, 0), whole), (name, region)
                assert one.at(0, 0).cells == whole.cells
            for region in ((16, 64), (40, 256), (7, 16)):
                got = fa.region_change_from(sim.context, fb, region)
                assert int(got.differing.sum()) == whole.differing and int(got.nonfinite.sum()) == whole.nonfinite, (name, region)
                assert change_ref.bits(float(got.max_abs.max())) == change_ref.bits(whole.max_abs), (name, region)
                assert int(got.size.sum()) == whole.cells
    sim.context.close()


# ---- field lists -----------------------------------------------------------------------------------------------------------------
def test_field_lists(built):
    shape, region = (45, 300), (32, 64)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    pairs = [special_pair(shape, 40 + k) for k in range(4)]
    fa, fb = [], []
    for a, b in pairs:
        for arr, to in ((a, fa), (b, fb)):
            f = HipConcentration(sim.context, shape)
            f.upload(sim.context, arr)
            to.append(f)
    want = [region_change_ref.changes(a, b, region) for a, b in pairs]
    for name in ROUTES:
        with route(name):
            for n in (1, 2, 3, 4):
                got = region_compare_fields(sim.context, fa[:n], fb[:n], region)
                assert len(got) == n
                for k in range(n):
                    assert_changes(got[k], want[k], shape, region, f"pair {k} of {n}, route {name}")
            mixed = region_compare_fields(sim.context, [fa[0], fb[1], fa[2]], [fb[0], fb[1], fb[0]], region)   # any pairing, one plane twice
            assert_changes(mixed[0], want[0], shape, region, "mixed 0")
            assert not mixed[1].differing.any()
            assert_changes(mixed[2], region_change_ref.changes(pairs[2][0], pairs[0][1], region), shape, region, "mixed 2")
    sim.context.close()


def test_species_against_its_snapshot(built):
    shape, region = (64, 128), (16, 32)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = sim.make_species(list(shape))
    sim.perform_steps(species, 40)
    snap = species.snapshot()
    in_u, in_v, _, _ = species.in_out()
    before = (in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context))
    for name in ROUTES:
        with route(name):
            su, sv = species.region_changes_since(snap, region)
        assert not su.differing.any() and not sv.differing.any() and sv.steady(0.0).all(), name
    sim.perform_steps(species, 8)
    in_u, in_v, _, _ = species.in_out()
    after = (in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context))
    want = [region_change_ref.changes(after[k], before[k], region) for k in range(2)]
    whole = species.change_since(snap)
    for name in ROUTES:
        with route(name):
            got = species.region_changes_since(snap, region)
        for k in range(2):
            assert_changes(got[k], want[k], shape, region, f"species {k}, route {name}")
            assert int(got[k].differing.sum()) == whole[k].differing and float(got[k].max_abs.max()) == whole[k].max_abs
    assert got[1].differing.any() and not got[1].steady(0.0).all()        # the seeded square moves; far corners do not
    snap.close()
    sim.context.close()


# ---- slab chains -------------------------------------------------------------------------------------------------------------
def chain_results(args, planes, region):
    sim = Simulation.new(Parameters(), args)
    species = species_from_arrays(sim, planes[0], planes[1])
    snap = species.snapshot()
    species.in_out()[0].upload(sim.context, planes[2])
    species.in_out()[1].upload(sim.context, planes[3])
    before = sim.context.stats()
    out = {}
    for name in ROUTES:
        with route(name):
            out[name] = species.region_changes_since(snap, region)
    assert sim.context.stats() == before
    snap.close()
    sim.context.close()
    return out


def test_slab_chains_give_the_same_bits(built):
    shape = (96, 300)
    ua, ub = special_pair(shape, 21)
    va, vb = change_ref.order_sensitive(shape, 22)
    planes = (ub, vb, ua, va)                                             # the snapshot holds ub, vb; the state ua, va
    for region, chains in (((16, 64), [HipArgs(devices=[0] * 2), HipArgs(devices=[0] * 3), HipArgs(devices=[0], split=2)]),
                           ((32, 256), [HipArgs(devices=[0] * 3)])):
        want = (region_change_ref.changes(ua, ub, region), region_change_ref.changes(va, vb, region))
        one = chain_results(HipArgs(devices=[0]), planes, region)
        for name in ROUTES:
            assert_changes(one[name][0], want[0], shape, region, f"one slab, U, route {name}")
            assert_changes(one[name][1], want[1], shape, region, f"one slab, V, route {name}")
        for args in chains:
            got = chain_results(args, planes, region)
            for name in ROUTES:
                for k in range(2):
                    for f in change_ref.FIELDS:
                        assert getattr(one[name][k], f).tobytes() == getattr(got[name][k], f).tobytes(), (region, args.devices, args.split, name, f)
    # two slabs: a seam at row 48, which is no multiple of 32 -- and three slabs, whose seams at 32 and 64 are no multiples of 48
    for devices, region in (([0] * 2, (32, 64)), ([0] * 3, (48, 64))):
        sim = Simulation.new(Parameters(), HipArgs(devices=devices))
        species = species_from_arrays(sim, ua, va)
        snap = species.snapshot()
        for name in ROUTES:
            with route(name), pytest.raises(capi.GsError) as e:
                species.region_changes_since(snap, region)
            assert e.value.code == capi.GS_ERR_UNSUPPORTED, (devices, name)
        snap.close()
        sim.context.close()


# ---- no side effects -----------------------------------------------------------------------------------------------------------
def test_an_interrupted_run_gives_the_bits_of_an_uninterrupted_one(built):
    shape, region = (64, 128), (32, 32)
    walls = np.zeros(shape, np.float32)
    walls[:, 40] = 1.0
    seen = {}
    for observed in (True, False):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0], boundary=capi.GS_BOUNDARY_PERIODIC))
        species = sim.make_species(list(shape))
        sim.set_mask(walls)
        sim.perform_steps(species, 24)
        snap = species.snapshot()
        sim.perform_steps(species, 8)
        if observed:
            before = (sim.context.stats(), sim.context.info())
            for name in ROUTES:
                with route(name):
                    got = species.region_changes_since(snap, region)
                in_u, in_v, _, _ = species.in_out()
                v = in_v.make_scalar_view(sim.context)
                assert_changes(got[1], region_change_ref.changes(v, snap.v.make_scalar_view(sim.context), region), shape, region,
                               f"with a mask, route {name}")                # wall cells count
            assert (sim.context.stats(), sim.context.info()) == before
        sim.perform_steps(species, 8)
        in_u, in_v, _, _ = species.in_out()
        seen[observed] = (in_u.make_scalar_view(sim.context).tobytes(), in_v.make_scalar_view(sim.context).tobytes())
        snap.close()
        sim.context.close()
    assert seen[True] == seen[False]


# ---- refusals that need handles ---------------------------------------------------------------------------------------------
def test_refusals_that_need_handles_and_the_empty_plane(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    a, b = HipConcentration(sim.context, (8, 32)), HipConcentration(sim.context, (8, 33))
    foreign = HipConcentration(other.context, (8, 32))
    a.upload(sim.context, stress_fields((8, 32), 1)[0])
    for first, second in (([a, b], [a, a]), ([a], [b]), ([a], [foreign]), ([foreign], [a]), ([a] * 5, [a] * 5)):
        with pytest.raises(capi.GsError) as e:
            region_compare_fields(sim.context, first, second, (4, 16))
        assert e.value.code == capi.GS_ERR_INVALID, (first, second)
    with pytest.raises(ValueError):
        region_compare_fields(sim.context, [a, a], [a], (4, 16))
    for region in ((4, 0), (4, 8), (4, 12), (4, 18), (0, 16), (-1, 16), (4, -16)):
        with pytest.raises(capi.GsError) as e:
            a.region_change_from(sim.context, a, region)
        assert e.value.code == capi.GS_ERR_INVALID, region
    # the region count: a small real field with more rows than GS_REGIONS_MAX allows columns for is accepted
    assert region_grid(4097, 16, (1, 16)) == (4097, 1)
    tall = HipConcentration(sim.context, (4097, 16))
    assert tall.region_change_from(sim.context, tall, (1, 16)).sum_abs.shape == (4097, 1)
    with route("sideways"), pytest.raises(capi.GsError) as e:
        a.region_change_from(sim.context, a, (4, 16))
    assert e.value.code == capi.GS_ERR_INVALID
    for shape in ((0, 16), (7, 0)):
        empty = HipConcentration(sim.context, shape)
        for name in ROUTES:
            with route(name):
                c = empty.region_change_from(sim.context, empty, (4, 16))
            assert c.sum_abs.size == 0 and c.size.size == 0
    for s in (sim, other):
        s.context.close()
