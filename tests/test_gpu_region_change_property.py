"""Seeded random cases of gs_fields_region_compare: any plane shape up to 200 x 600, any admissible region shape, 1..4 pairs,
slab count 1..3, planes of every kind -- order-sensitive magnitudes, planted NaN, infinities, sub-normals and signed zeros,
unmoved blocks, a plane against itself --, each under both forced routes and the library's choice, bit for bit against
tests/region_change_ref.py.  Every case runs: one whose slab seam is no multiple of the region height asserts the refusal and
then runs on one slab."""
import os

import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, Simulation, capi
from grayscott_amd.simulation import region_compare_fields
from tests import change_ref, region_change_ref

pytestmark = pytest.mark.gpu
CASES, GROUPS = 24, 6
ROUTES = ("records", "wave", "")  # "": the library's choice
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-40, 2.0 ** 80, -2.0 ** 80, 1.0], np.float32)


def pair(shape, rng, seed):
    """Two planes of one of four kinds."""
    a, b = change_ref.order_sensitive(shape, seed)
    kind = int(rng.integers(0, 4))
    if kind == 1:                                                           # special values, each plane on its own
        for x in (a, b):
            pos = rng.choice(x.size, size=max(1, x.size // 10), replace=False)
            x.flat[pos] = rng.choice(SPECIAL, size=len(pos))
    elif kind == 2:                                                         # an unmoved block and a non-finite one
        r, c = int(rng.integers(0, shape[0])), int(rng.integers(0, shape[1]))
        b[r:r + 40, c:c + 200] = a[r:r + 40, c:c + 200]
        a[:r // 2, :c // 2] = np.float32(np.nan)
    elif kind == 3:                                                         # a plane against itself
        b = a.copy()
    return a, b


def case(seed):
    rng = np.random.default_rng(12000 + seed)
    rows, cols = int(rng.integers(1, 201)), int(rng.integers(1, 601))
    # region heights around the unroll depth and the band height, up to more than the plane; widths from 16 columns up
    B = int(rng.choice([region_change_ref.UNROLL, region_change_ref.BAND]))
    rh = int(rng.choice([1, 2, B - 1, B, B + 1, 2 * B, 2 * B + 1, int(rng.integers(1, rows + 1)), rows, rows + int(rng.integers(1, 50))]))
    rw = 4 * int(rng.choice([4, 5, int(rng.integers(4, 17)), int(rng.integers(4, 65)), 64, int(rng.integers(64, 140)),
                             int(rng.integers(4, cols // 4 + 5)), cols // 4 + 4]))
    n = int(rng.integers(1, 5))
    slabs = min(int(rng.integers(1, 4)), rows)                              # (one-row slabs occur)
    pairs = [pair((rows, cols), rng, 100 * seed + k) for k in range(n)]
    return pairs, (rh, rw), slabs


def run(pairs, region, slabs):
    """The results of every route, {route: [RegionChange per pair]}."""
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * slabs))
    try:
        fa, fb = [], []
        for a, b in pairs:
            for arr, to in ((a, fa), (b, fb)):
                to.append(HipConcentration(sim.context, arr.shape))
                to[-1].upload(sim.context, arr)
        out = {}
        for route in ROUTES:
            os.environ["GS_HIP_REGION_CHANGE_ROUTE"] = route
            out[route] = region_compare_fields(sim.context, fa, fb, region)
        return out
    finally:
        os.environ.pop("GS_HIP_REGION_CHANGE_ROUTE", None)
        sim.context.close()


@pytest.mark.parametrize("group", range(GROUPS))
def test_random_cases(built, group):
    for seed in range(group, CASES, GROUPS):
        pairs, region, slabs = case(seed)
        what = f"seed {seed}: {len(pairs)} pairs of {pairs[0][0].shape} region {region} slabs {slabs}"
        rows = pairs[0][0].shape[0]
        aligned = all((k * rows // slabs) % region[0] == 0 for k in range(1, slabs))
        if not aligned:
            with pytest.raises(capi.GsError) as e:
                run(pairs, region, slabs)
            assert e.value.code == capi.GS_ERR_UNSUPPORTED, what
            slabs = 1
        got = run(pairs, region, slabs)
        wanted = [region_change_ref.changes(a, b, region) for a, b in pairs]
        for route in ROUTES:
            assert len(got[route]) == len(pairs), what
            for k, (c, want) in enumerate(zip(got[route], wanted)):
                assert c.sum_abs.shape == want.shape, what
                for at in np.ndindex(want.shape):
                    assert change_ref.same(c.at(*at), want[at]), (f"{what}, route {route or 'choice'}, pair {k}, region {at}: "
                                                                 f"{change_ref.as_dict(c.at(*at))}, not {change_ref.as_dict(want[at])}")
