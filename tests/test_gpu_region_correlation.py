"""Regional two-point pair counts on the device (gs_fields_region_correlation) against their definition
(tests/region_corr_ref.py): every region's counts are those of the whole-grid rule on that region's cells alone.  Everything
is bit for bit."""
import functools
import sys

import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, RegionCorrelation, Simulation, capi, hdf5_min
from grayscott_amd.simulation import correlation_fields, region_correlation_fields
from tests import corr_ref, region_corr_ref, regions_ref
from tests.children import ROOT, run_program
from tests.helpers import species_from_arrays, stress_fields

pytestmark = pytest.mark.gpu

H = corr_ref.UNIT_ROWS  # the pair kernels' unit height (kPairRows), restated in tests/corr_ref.py
THRESHOLDS = [0.3, -1.5, 0.0, 2.0 ** -130]  # distinct, one of them sub-normal
SENSES = [True, False, True, False]
SHAPE = (96, 300)
# one word per region (rw <= 64, ragged last column of 44, 12 and 0 columns), a region of 7 rows that leaves a last row of 5,
# four words without halo words (48, 256), and one region over the whole plane in two strips with halo words (100, 320)
REGIONS = [(32, 64), (16, 16), (7, 20), (48, 256), (100, 320)]


@functools.lru_cache(maxsize=None)
def odd_plane(k):
    """Plane k of SHAPE: values in [-2, 2) with NaN, +-inf, sub-normals, signed zeros and cells equal to every threshold."""
    rng = np.random.default_rng(100 + k)
    a = ((stress_fields(SHAPE, 30 + k)[0] - np.float32(0.5)) * np.float32(4.0)).astype(np.float32)
    odd = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-40, 2.0 ** -131, 2.0 ** -129, -2.0 ** -130] + THRESHOLDS, np.float32)
    at = rng.choice(a.size, size=40 * len(odd), replace=False)
    a.flat[at] = np.tile(odd, 40)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want(k, region, t, above):
    """Plane k's counts at the largest lag, once; the counts of a smaller L are its first L + 1 lags."""
    return region_corr_ref.pairs_by_label(odd_plane(k), region, THRESHOLDS[t], above, 64)


def assert_pairs(got: RegionCorrelation, wanted, shape, region, what):
    L = got.max_lag
    wanted = wanted[..., :L + 1]
    assert got.pairs.dtype == np.uint64 and got.pairs.shape == wanted.shape, what
    assert got.region == regions_ref.shape_of(region) and got.shape == tuple(shape), what
    assert np.array_equal(got.cells, regions_ref.sizes(shape, region)), what
    bad = np.argwhere(got.pairs != wanted)
    assert bad.size == 0, (f"{what}: t {got.threshold} above {got.above} L {L}: {len(bad)} counters differ, first "
                           f"(i, j, k, d) = {tuple(bad[0])}: {int(got.pairs[tuple(bad[0])])}, not {int(wanted[tuple(bad[0])])}")


def upload_all(ctx, planes):
    fields = []
    for p in planes:
        f = HipConcentration(ctx, p.shape)
        f.upload(ctx, np.array(p))
        fields.append(f)
    return fields


# ---- odd values and ragged regions; lags, thresholds, senses and field lists ----------------------------------------------------
@pytest.mark.parametrize("region", REGIONS)
def test_odd_values_and_ragged_regions(built, region):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    fields = upload_all(ctx, [odd_plane(k) for k in range(4)])
    # n fields, nt thresholds each, largest lag L; field k set above (even k) or below (odd k) its thresholds
    for n, nt, L in ((4, 4, 64), (1, 1, 1), (2, 2, 5), (3, 3, 64), (1, 4, 5), (4, 1, 64)):
        got = region_correlation_fields(ctx, fields[:n], region, [THRESHOLDS[:nt]] * n, SENSES[:n], L)
        assert len(got) == n and all(len(g) == nt for g in got)
        for k in range(n):
            for t in range(nt):
                assert got[k][t].max_lag == L and got[k][t].above == SENSES[k]
                assert got[k][t].threshold == float(np.float32(THRESHOLDS[t]))
                assert_pairs(got[k][t], want(k, region, t, SENSES[k]), SHAPE, region, f"region {region} n {n} nt {nt} field {k}")
    # the other sense of every field, through the plane's own method
    for k in range(4):
        for c, t in zip(fields[k].region_correlation(ctx, region, THRESHOLDS[:2], 5, not SENSES[k]), range(2)):
            assert_pairs(c, want(k, region, t, not SENSES[k]), SHAPE, region, f"region {region} field {k} other sense")
    if region[0] >= SHAPE[0] and region[1] >= SHAPE[1]:       # one region: the whole-grid call's bits
        one = region_correlation_fields(ctx, fields, region, [THRESHOLDS] * 4, SENSES, 64)
        whole = correlation_fields(ctx, fields, [THRESHOLDS] * 4, SENSES, 64)
        for k in range(4):
            for t in range(4):
                assert one[k][t].pairs.shape == (1, 1, 4, 65) and np.array_equal(one[k][t].pairs[0, 0], whole[k][t].pairs), (k, t)
                assert np.array_equal(whole[k][t].pairs, corr_ref.pairs(odd_plane(k), THRESHOLDS[t], SENSES[k], 64)), (k, t)
    sim.context.close()


# ---- a region's border is a wall: on an all-set plane every counter is the region's own geometry -----------------------------
@pytest.mark.parametrize("region", REGIONS)
def test_region_borders_are_walls(built, region):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    field = HipConcentration(sim.context, SHAPE)
    field.upload(sim.context, np.ones(SHAPE, np.float32))
    for L in (64, 5):
        c = field.region_correlation(sim.context, region, [0.5, 2.0], L)
        wanted = region_corr_ref.totals(SHAPE, region, L)
        excess = c[0].pairs.astype(np.int64) - wanted
        assert not excess.any(), f"region {region} L {L}: pairs leaked or lost at (i, j, k, d) = {tuple(np.argwhere(excess)[0])}"
        assert np.array_equal(c[0].totals(), wanted) and not c[1].pairs.any()                # (nothing is above 2.0)
        assert np.array_equal(c[0].pairs[:, :, 0, 0].astype(np.int64), c[0].cells)
    sim.context.close()


# ---- seams inside a region: two strips (lags carried across words and strips), two row units (the run-in reads the region's
# own rows; the region below begins with nothing above it), and both at once --------------------------------------------------
@pytest.mark.parametrize("shape,region", [((40, 700), (40, 320)), ((2 * H + 76, 80), (H + 88, 80)), ((2 * H + 76, 300), (H + 88, 300))])
def test_seams_inside_a_region(built, shape, region):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    field = HipConcentration(sim.context, shape)
    rng = np.random.default_rng(shape[0])
    plane = (rng.random(shape, dtype=np.float32) < np.float32(0.6)).astype(np.float32)
    plane[::7, ::5] = np.float32(np.nan)
    field.upload(sim.context, plane)
    got = field.region_correlation(sim.context, region, [0.5, -1.0], 64)
    for c, t in zip(got, (0.5, -1.0)):
        assert_pairs(c, region_corr_ref.pairs(plane, region, t, True, 64), shape, region, f"{shape} {region} t {t}")
    sim.context.close()


# ---- slab chains -------------------------------------------------------------------------------------------------------------
def chain_results(args, u0, v0, region, L=64):
    sim = Simulation.new(Parameters(), args)
    species = species_from_arrays(sim, u0, v0)
    before = sim.context.stats()
    cu, cv = species.region_correlation(region, (0.25, 0.1), (0.5, 0.8), L)
    assert sim.context.stats() == before
    sim.context.close()
    return cu + cv


def test_slab_chains_give_the_same_bits(built):
    shape = (96, 300)
    u0, v0 = stress_fields(shape, 21)
    v0[47:49] = np.float32(0.45)          # set rows on both sides of the two-slab seam, and of the three-slab seams
    v0[31:33] = np.float32(0.45)
    v0[63:65, ::3] = np.float32(np.nan)
    for region, chains in (((16, 64), [HipArgs(devices=[0] * 2), HipArgs(devices=[0] * 3), HipArgs(devices=[0], split=2)]),
                           ((32, 320), [HipArgs(devices=[0] * 3), HipArgs(devices=[0], split=3)])):
        one = chain_results(HipArgs(devices=[0]), u0, v0, region)
        for c, (plane, t, above) in zip(one, ((u0, 0.5, False), (u0, 0.8, False), (v0, 0.25, True), (v0, 0.1, True))):
            assert c.above == above
            assert_pairs(c, region_corr_ref.pairs_by_label(plane, region, t, above, 64), shape, region, f"one slab {region} t {t}")
        for args in chains:
            for a, b in zip(one, chain_results(args, u0, v0, region)):
                assert np.array_equal(a.pairs, b.pairs), (region, args.devices, args.split)
    # two slabs: a seam at row 48, which is no multiple of 32 -- refused, and the context goes on working
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * 2))
    species = species_from_arrays(sim, u0, v0)
    with pytest.raises(capi.GsError) as e:
        species.region_correlation((32, 64))
    assert e.value.code == capi.GS_ERR_UNSUPPORTED
    _, cv = species.region_correlation((16, 64), (0.25,), None, 8)
    assert_pairs(cv[0], region_corr_ref.pairs_by_label(v0, (16, 64), 0.25, True, 8), shape, (16, 64), "after the refusal")
    sim.context.close()


# ---- no side effects -----------------------------------------------------------------------------------------------------------
def test_no_side_effects(built):
    shape = (64, 128)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = sim.make_species(list(shape))
    sim.perform_steps(species, 16)
    in_u, in_v, _, _ = species.in_out()
    planes = (in_u.make_scalar_view(sim.context).tobytes(), in_v.make_scalar_view(sim.context).tobytes())
    before = (sim.context.stats(), sim.context.info())
    species.region_correlation((16, 32), (0.25, 0.1), (0.5, 0.8), 16)
    assert (sim.context.stats(), sim.context.info()) == before
    in_u, in_v, _, _ = species.in_out()
    assert (in_u.make_scalar_view(sim.context).tobytes(), in_v.make_scalar_view(sim.context).tobytes()) == planes
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
            if attach == "map":
                sim.set_param_map(feed, kill)
            else:
                sim.set_mask(walls)
            sim.perform_steps(species, steps)
            before = (sim.context.stats(), sim.context.info())
            cu, cv = species.region_correlation(region, (0.25, 0.1), (0.5, 0.8), 16)
            assert (sim.context.stats(), sim.context.info()) == before
            in_u, in_v, _, _ = species.in_out()
            u, v = in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)
            what = f"boundary {boundary}, math {math}, {attach}"
            for k, (tu, tv) in enumerate(((0.5, 0.25), (0.8, 0.1))):         # (wall cells count; pairs never wrap)
                assert_pairs(cu[k], region_corr_ref.pairs_by_label(u, region, tu, False, 16), shape, region, what)
                assert_pairs(cv[k], region_corr_ref.pairs_by_label(v, region, tv, True, 16), shape, region, what)
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
            region_correlation_fields(sim.context, fields, (4, 16), [[0.5]] * len(fields), [True] * len(fields), 4)
        assert e.value.code == capi.GS_ERR_INVALID, fields
    for region, thresholds, lag in (((4, 18), [0.5], 4), ((0, 16), [0.5], 4), ((4, 16), [], 4), ((4, 16), [0.1] * 5, 4),
                                    ((4, 16), [float("nan")], 4), ((4, 16), [0.5], 0), ((4, 16), [0.5], 65)):
        with pytest.raises(capi.GsError) as e:
            a.region_correlation(sim.context, region, thresholds, lag)
        assert e.value.code == capi.GS_ERR_INVALID, (region, thresholds, lag)
    for shape in ((0, 16), (7, 0)):
        empty = HipConcentration(sim.context, shape)
        c = empty.region_correlation(sim.context, (4, 16), [0.1, 0.2], 8)
        assert len(c) == 2 and c[0].pairs.size == 0
    for s in (sim, other):
        s.context.close()


def test_result_cap(built):
    """16 x 8066 regions stay under GS_REGIONS_MAX; with nt = 4 and L = 64 they are 1040 counters each, over
    GS_REGION_PAIRS_MAX = 2^25 per field; with nt = 1 and L = 1 they are 8 each and the call counts."""
    shape, region = (16, 16 * 8066), (1, 16)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    field = HipConcentration(sim.context, shape)
    plane = stress_fields(shape, 3)[0]
    field.upload(sim.context, plane)
    assert 16 * 8066 * 4 * 4 * 65 > capi.GS_REGION_PAIRS_MAX >= 16 * 8066 * 4 * 2 and 16 * 8066 <= 1 << 22
    with pytest.raises(capi.GsError) as e:
        field.region_correlation(sim.context, region, THRESHOLDS, 64)
    assert e.value.code == capi.GS_ERR_INVALID and "counters" in e.value.message
    c = field.region_correlation(sim.context, region, [0.5], 1)[0]
    b = (plane > np.float32(0.5)).reshape(16, 8066, 16)
    assert np.array_equal(c.pairs[:, :, 0, 0], b.sum(axis=2).astype(np.uint64))
    assert np.array_equal(c.pairs[:, :, 0, 1], (b[:, :, 1:] & b[:, :, :-1]).sum(axis=2).astype(np.uint64))
    assert not c.pairs[:, :, 1:, 1].any()                                  # one row: no pair down a column or a diagonal
    sim.context.close()


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_the_driver_records_the_pair_counts(built, tmp_path):
    base = [sys.executable, "-m", "grayscott_amd.simulate", "-r", "64", "-c", "128", "-n", "2", "-e", "16", "--hip-feed-map", "0.01:0.06",
            "--hip-kill-map", "0.04:0.07", "--hip-regions", "16x32", "--hip-regions-every", "1", "--hip-region-threshold-v", "0.25,0.1"]
    region = (16, 32)
    with_flag, without = tmp_path / "with.h5", tmp_path / "without.h5"
    r = run_program(base + ["--hip-region-corr-lags", "8", "-o", str(with_flag)], cwd=ROOT)
    assert r.returncode == 0, r.stderr
    images = hdf5_min.read(str(with_flag))
    z = np.load(tmp_path / "with.regions.npz")
    assert int(z["corr_lags"]) == 8 and "pairs_u" not in z.files
    assert z["pairs_v"].shape == (2, 2, 4, 4, 4, 9) and z["pairs_v"].dtype == np.uint64
    for k, t in enumerate((0.25, 0.1)):                                    # (the images are the V planes)
        assert np.array_equal(z["pairs_v"][-1, k], region_corr_ref.pairs(images[-1], region, t, True, 8)), t
    r = run_program(base + ["-o", str(without)], cwd=ROOT)
    assert r.returncode == 0, r.stderr
    old = np.load(tmp_path / "without.regions.npz")
    keys = {"region", "shape", "steps", "thresholds_v", "thresholds_u", "cells", "quads_v", "feed", "kill"}
    keys |= {f"{f}_{s}" for f in ("sum", "sum_sq", "min", "max", "nonfinite") for s in "uv"}
    assert set(old.files) == keys and set(z.files) == keys | {"pairs_v", "corr_lags"}
    for key in keys:
        assert old[key].tobytes() == z[key].tobytes(), key
