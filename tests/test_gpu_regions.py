"""Regional observables on the device (gs_fields_region_summaries, gs_fields_region_morphology) against their definition
(tests/regions_ref.py): every region cropped from the downloaded plane and handed to the whole-grid restatements.  Sums are
bit-equal, zero extremes compare as summary_ref.same compares them, quads are equal everywhere."""
import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, RegionMorphology, RegionSummaries, Simulation, capi
from grayscott_amd.simulation import (morphology_fields, region_grid, region_morphology_fields, region_summaries_fields,
                                      summarize_fields)
from tests import morph_ref, observe_cases, regions_ref, summary_ref
from tests.helpers import species_from_arrays, stress_fields

pytestmark = pytest.mark.gpu

H = morph_ref.UNIT_ROWS  # the quad kernels' unit height, restated in tests/morph_ref.py
THRESHOLDS = [0.3, -1.5, 0.0, 2.0 ** -130]  # distinct, one of them sub-normal


def assert_summaries(got: RegionSummaries, plane, region, what):
    want = regions_ref.summaries(plane, region)
    assert got.sum.shape == want.shape and got.shape == plane.shape and got.region == regions_ref.shape_of(region), what
    assert np.array_equal(got.size, regions_ref.sizes(plane.shape, region)), what
    for at in np.ndindex(want.shape):
        assert summary_ref.same(got.at(*at), want[at]), f"{what}: region {at}: {got.at(*at)}, not {want[at]}"


def assert_quads(got: RegionMorphology, plane, region, what):
    want = regions_ref.quads(plane, region, got.threshold, got.above)
    assert got.quads.dtype == np.uint64 and got.quads.shape == want.shape, what
    sizes = regions_ref.sizes(plane.shape, region)
    assert np.array_equal(got.cells, sizes), what
    bad = np.argwhere((got.quads != want).any(axis=2))
    assert bad.size == 0, (f"{what}: t {got.threshold} above {got.above}: {len(bad)} regions differ, first {tuple(bad[0])}: "
                           f"{list(map(int, got.quads[tuple(bad[0])]))}, not {list(map(int, want[tuple(bad[0])]))}")


def check_plane(ctx, field, plane, region, thresholds=(0.3,), above=True, what=""):
    field.upload(ctx, plane)
    assert_summaries(field.region_summaries(ctx, region), plane, region, what)
    ms = field.region_morphology(ctx, region, thresholds, above)
    assert len(ms) == len(thresholds)
    for m in ms:
        assert_quads(m, plane, region, what)
    return ms


def planes_for(shape, seed):
    """Planes with sub-normals, NaN, +-inf and signed zeros among ordinary values, of several kinds."""
    yield "planted", morph_ref.planted(shape, 0.3, seed, 0.5, True)
    yield "seams", observe_cases.plane("seams", shape, 0.3, True, seed + 1)
    yield "lane_runs", observe_cases.plane("lane_runs", shape, 0.3, False, seed + 2)
    yield "uniform", stress_fields(shape, seed + 3)[0]


# ---- columns: one region narrower than a wave row, several side by side with a ragged last one (width 1, 3, 4; cols no
# multiple of 4: the pitch padding must be masked), a region exactly 256 wide, regions crossing the 256-column chunk ---------
COLUMN_CASES = [((5, 16), 16), ((5, 40), 16), ((3, 263), 16), ((3, 263), 64), ((3, 263), 256), ((3, 263), 260), ((4, 256), 16),
                ((4, 256), 256), ((3, 257), 256), ((2, 1025), 252), ((2, 1025), 512), ((6, 531), 132)]


@pytest.mark.parametrize("shape,rw", COLUMN_CASES)
def test_columns(built, shape, rw):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    field = HipConcentration(sim.context, shape)
    for rh in (2, shape[0]):
        for kind, plane in planes_for(shape, 7 * rw + shape[1]):
            check_plane(sim.context, field, plane, (rh, rw), THRESHOLDS[:2], kind != "lane_runs", f"{kind} {shape} ({rh}, {rw})")
    sim.context.close()


# ---- rows: a ragged last region row of one row and none, around the quad kernels' unit height ----------------------------
@pytest.mark.parametrize("rh", [1, 2, H - 1, H, H + 1])
def test_rows(built, rh):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    for rows in (2 * rh + 1, 3 * rh):
        shape = (rows, 300)
        field = HipConcentration(sim.context, shape)
        for kind, plane in planes_for(shape, rh):
            check_plane(sim.context, field, plane, (rh, 64), [0.3], True, f"{kind} {shape} rh {rh}")
    sim.context.close()


def test_one_row_of_regions_and_one_region(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    shape = (H + 3, 300)
    field = HipConcentration(sim.context, shape)
    plane = morph_ref.planted(shape, 0.3, 5)
    for rh in (shape[0], shape[0] + 1, 1000, 2 ** 31 - 1):        # rh >= R: one region row
        ms = check_plane(sim.context, field, plane, (rh, 64), [0.3], True, f"rh {rh}")
        assert ms[0].quads.shape == (1, 5, 6)
    # one region covering the whole grid equals the whole-grid calls
    for region in ((shape[0], 300), (64, 512), 2 ** 31 - 4):
        rs = field.region_summaries(sim.context, region)
        rm = field.region_morphology(sim.context, region, THRESHOLDS)
        whole = summarize_fields(sim.context, [field])[0]
        assert rs.sum.shape == (1, 1) and summary_ref.same(rs.at(0, 0), whole) and rs.at(0, 0).size == whole.size
        assert summary_ref.same(whole, summary_ref.summary(plane))
        for m, w in zip(rm, morphology_fields(sim.context, [field], [THRESHOLDS], [True])[0]):
            assert np.array_equal(m.quads[0, 0], w.quads) and np.array_equal(m.at(0, 0).quads, morph_ref.quads(plane, w.threshold, True))
    sim.context.close()


# ---- thresholds and planes -------------------------------------------------------------------------------------------------
def test_thresholds_senses_and_field_lists(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    shape, region = (H + 5, 300), (16, 64)
    inf = float("inf")
    field = HipConcentration(sim.context, shape)
    for above in (True, False):
        plane = morph_ref.planted(shape, 0.3, 11, 0.5, above)
        four = check_plane(sim.context, field, plane, region, THRESHOLDS, above, f"nt 4, above {above}")
        assert [m.threshold for m in four] == [float(np.float32(x)) for x in THRESHOLDS]
        for k, t in enumerate(THRESHOLDS):                    # nt = 4 in one call equals four calls with nt = 1
            one = field.region_morphology(sim.context, region, [t], above)
            assert len(one) == 1 and np.array_equal(one[0].quads, four[k].quads), (above, k)
        for t in (inf, -inf):
            assert_quads(field.region_morphology(sim.context, region, [t], above)[0], plane, region, f"t {t}")
    # 1 to 4 fields in a call, each with its own thresholds and sense
    planes = [morph_ref.planted(shape, THRESHOLDS[k], 40 + k, 0.5, k % 2 == 0) for k in range(4)]
    fields = []
    for p in planes:
        f = HipConcentration(sim.context, shape)
        f.upload(sim.context, p)
        fields.append(f)
    for n in (1, 2, 3, 4):
        got = region_morphology_fields(sim.context, fields[:n], region, [[THRESHOLDS[k], 0.7] for k in range(n)],
                                       [k % 2 == 0 for k in range(n)])
        sums = region_summaries_fields(sim.context, fields[:n], region)
        assert len(got) == n and len(sums) == n
        for k in range(n):
            assert got[k][0].above == (k % 2 == 0)
            assert_quads(got[k][0], planes[k], region, f"field {k} of {n}")
            assert_quads(got[k][1], planes[k], region, f"field {k} of {n}, second threshold")
            assert_summaries(sums[k], planes[k], region, f"field {k} of {n}")
    # an all-set plane: every full region is one filled rectangle
    field.upload(sim.context, np.ones(shape, np.float32))
    m = field.region_morphology(sim.context, region, [0.5])[0]
    assert_quads(m, np.ones(shape, np.float32), region, "all set")
    full = m.cells == 16 * 64
    assert full.sum() == 2 * 4 and np.all(m.area[full] == 16 * 64) and np.all(m.perimeter[full] == 2 * (16 + 64))
    assert np.all(m.euler4 == 1) and np.all(m.euler8 == 1) and np.all(m.area == m.cells) and np.all(m.area_fraction == 1.0)
    sim.context.close()


# ---- slab chains -------------------------------------------------------------------------------------------------------------
def chain_results(args, u0, v0, region):
    sim = Simulation.new(Parameters(), args)
    species = species_from_arrays(sim, u0, v0)
    before = sim.context.stats()
    su, sv = species.region_summaries(region)
    mu, mv = species.region_morphology(region, (0.25, 0.1), (0.5, 0.8))
    assert sim.context.stats() == before
    sim.context.close()
    return su, sv, mu, mv


def test_slab_chains_give_the_same_bits(built):
    shape = (96, 300)
    u0, v0 = stress_fields(shape, 21)
    v0[47:49] = np.float32(0.45)          # set rows on both sides of the two-slab seam, and of the three-slab seams
    v0[31:33] = np.float32(0.45)
    v0[63:65, ::3] = np.float32(np.nan)
    for region, chains in (((16, 64), [HipArgs(devices=[0] * 2), HipArgs(devices=[0] * 3), HipArgs(devices=[0], split=2)]),
                           ((32, 64), [HipArgs(devices=[0] * 3), HipArgs(devices=[0], split=2)])):
        su, sv, mu, mv = chain_results(HipArgs(devices=[0]), u0, v0, region)
        assert_summaries(su, u0, region, "one slab, U")
        assert_summaries(sv, v0, region, "one slab, V")
        for k in range(2):
            assert_quads(mu[k], u0, region, "one slab, U")
            assert_quads(mv[k], v0, region, "one slab, V")
        for args in chains:
            tu, tv, nu, nv = chain_results(args, u0, v0, region)
            for a, b in ((su, tu), (sv, tv)):
                for f in summary_ref.FIELDS:
                    assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (region, args.devices, args.split, f)
            for a, b in zip(mu + mv, nu + nv):
                assert np.array_equal(a.quads, b.quads), (region, args.devices, args.split)
    # two slabs: a seam at row 48, which is no multiple of 32
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * 2))
    species = species_from_arrays(sim, u0, v0)
    for call in (lambda: species.region_summaries((32, 64)), lambda: species.region_morphology((32, 64))):
        with pytest.raises(capi.GsError) as e:
            call()
        assert e.value.code == capi.GS_ERR_UNSUPPORTED
    sim.context.close()


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
            if attach == "map":                         # (every rule has a form for both attachments: none may refuse)
                sim.set_param_map(feed, kill)
            else:
                sim.set_mask(walls)
            sim.perform_steps(species, steps)
            before = (sim.context.stats(), sim.context.info())
            su, sv = species.region_summaries(region)
            mu, mv = species.region_morphology(region, (0.25, 0.1), (0.5, 0.8))
            assert (sim.context.stats(), sim.context.info()) == before
            in_u, in_v, _, _ = species.in_out()
            u, v = in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)
            what = f"boundary {boundary}, math {math}, {attach}"
            assert_summaries(su, u, region, what)
            assert_summaries(sv, v, region, what)
            for k in range(2):
                assert_quads(mu[k], u, region, what)
                assert_quads(mv[k], v, region, what)
            # a following run's bits are those of a run that was never observed
            sim.perform_steps(species, 8)
            in_u, in_v, _, _ = species.in_out()
            seen = (in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context))
            sim.context.close()
            sim = Simulation.new(Parameters(), HipArgs(devices=[0], boundary=boundary, math=math))
            species = sim.make_species(list(shape))
            if attach == "map":
                sim.set_param_map(feed, kill)
            else:
                sim.set_mask(walls)
            sim.perform_steps(species, steps)
            sim.perform_steps(species, 8)
            in_u, in_v, _, _ = species.in_out()
            assert seen[0].tobytes() == in_u.make_scalar_view(sim.context).tobytes(), what
            assert seen[1].tobytes() == in_v.make_scalar_view(sim.context).tobytes(), what
            sim.context.close()


# ---- refusals that need handles ---------------------------------------------------------------------------------------------
def test_refusals_that_need_handles_and_the_empty_plane(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    a, b = HipConcentration(sim.context, (8, 32)), HipConcentration(sim.context, (8, 33))
    foreign = HipConcentration(other.context, (8, 32))
    a.upload(sim.context, stress_fields((8, 32), 1)[0])
    for fields in ([a, b], [a, foreign], [a] * 5):
        for call in (lambda: region_summaries_fields(sim.context, fields, (4, 16)),
                     lambda: region_morphology_fields(sim.context, fields, (4, 16), [[0.5]] * len(fields), [True] * len(fields))):
            with pytest.raises(capi.GsError) as e:
                call()
            assert e.value.code == capi.GS_ERR_INVALID, fields
    for region in ((4, 0), (4, 8), (4, 18), (0, 16), (-1, 16), (4, -16)):
        for call in (lambda: a.region_summaries(sim.context, region), lambda: a.region_morphology(sim.context, region, [0.5])):
            with pytest.raises(capi.GsError) as e:
                call()
            assert e.value.code == capi.GS_ERR_INVALID, region
    for thresholds in ([], [0.1] * 5, [float("nan")]):
        with pytest.raises(capi.GsError) as e:
            a.region_morphology(sim.context, (4, 16), thresholds)
        assert e.value.code == capi.GS_ERR_INVALID, thresholds
    # the region count: exactly GS_REGIONS_MAX regions are accepted, one row more is refused (no large field is made)
    assert region_grid(4096, 16384, (1, 16)) == (4096, 1024)
    with pytest.raises(capi.GsError) as e:
        region_grid(4097, 16384, (1, 16))
    assert e.value.code == capi.GS_ERR_INVALID
    tall = HipConcentration(sim.context, (4097, 16))            # a small real field with the refused row count: 4097 regions, accepted
    assert region_grid(4097, 16, (1, 16)) == (4097, 1)
    assert tall.region_summaries(sim.context, (1, 16)).sum.shape == (4097, 1)
    for shape in ((0, 16), (7, 0)):
        empty = HipConcentration(sim.context, shape)
        s = empty.region_summaries(sim.context, (4, 16))
        m = empty.region_morphology(sim.context, (4, 16), [0.1, 0.2])
        assert s.sum.size == 0 and len(m) == 2 and m[0].quads.size == 0
    for s in (sim, other):
        s.context.close()
