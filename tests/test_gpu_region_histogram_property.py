"""Seeded random cases of gs_fields_region_histogram: any plane shape up to 200 x 700, any admissible region shape, bin count,
range (negative and tiny ones among them), 1..4 fields and slab count 1..3, bit for bit against tests/region_hist_ref.py.
Every case runs: one whose slab seam is no multiple of the region height asserts the refusal and then runs on one slab."""
import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, Simulation, capi
from grayscott_amd.simulation import region_histogram_fields
from tests import hist_ref, region_hist_ref

pytestmark = pytest.mark.gpu
CASES, GROUPS = 24, 6
# every range is legal with every bin count: the width and 4096 / width are normal f32 (include/gs_hip.h)
RANGES = [(0.0, 1.0), (-1.0, 1.0), (-0.5, -0.25), (0.0, 2.0 ** -100), (1e-3, 1.001e-3), (-1e30, 1e30), (0.25, 0.5), (-2.0 ** -100, 2.0 ** -100)]


def case(seed):
    rng = np.random.default_rng(9000 + seed)
    rows, cols = int(rng.integers(1, 201)), int(rng.integers(1, 701))
    # region heights and widths from one cell (16 columns) to more than the plane, small ones as likely as large ones
    rh = int(rng.choice([1, 2, int(rng.integers(1, 17)), int(rng.integers(1, rows + 1)), rows, rows + int(rng.integers(1, 50))]))
    rw = 4 * int(rng.choice([4, 5, int(rng.integers(4, 17)), int(rng.integers(4, 65)), int(rng.integers(4, cols // 4 + 5)), cols // 4 + 4]))
    bins = int(rng.choice([1, 2, 3, 64, 255, 1024, 4096]))
    n = int(rng.integers(1, 5))
    ranges = [RANGES[int(i)] for i in rng.choice(len(RANGES), size=n, replace=False)]
    slabs = min(int(rng.integers(1, 4)), rows)                              # (one-row slabs occur)
    planes = [hist_ref.planted((rows, cols), lo, hi, bins, 100 * seed + k) for k, (lo, hi) in enumerate(ranges)]
    return planes, (rh, rw), bins, ranges, slabs


def run(planes, region, bins, ranges, slabs):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * slabs))
    try:
        fields = []
        for p in planes:
            fields.append(HipConcentration(sim.context, p.shape))
            fields[-1].upload(sim.context, p)
        return region_histogram_fields(sim.context, fields, region, bins, ranges)
    finally:
        sim.context.close()


@pytest.mark.parametrize("group", range(GROUPS))
def test_random_cases(built, group):
    for seed in range(group, CASES, GROUPS):
        planes, region, bins, ranges, slabs = case(seed)
        what = f"seed {seed}: planes {len(planes)} x {planes[0].shape} region {region} bins {bins} ranges {ranges} slabs {slabs}"
        rows = planes[0].shape[0]
        aligned = all((k * rows // slabs) % region[0] == 0 for k in range(1, slabs))
        if not aligned:
            with pytest.raises(capi.GsError) as e:
                run(planes, region, bins, ranges, slabs)
            assert e.value.code == capi.GS_ERR_UNSUPPORTED, what
            slabs = 1
        got = run(planes, region, bins, ranges, slabs)
        assert len(got) == len(planes), what
        for h, plane, (lo, hi) in zip(got, planes, ranges):
            wanted = region_hist_ref.by_label(plane, region, lo, hi, bins)
            c = region_hist_ref.counters_of(h)
            assert c.shape == wanted.shape and h.bins == bins, what
            bad = np.argwhere(c != wanted)
            assert bad.size == 0, (f"{what} [{lo}, {hi}]: {len(bad)} counters differ, first (i, j, slot) = {tuple(bad[0])}: "
                                   f"{int(c[tuple(bad[0])])}, not {int(wanted[tuple(bad[0])])}")
