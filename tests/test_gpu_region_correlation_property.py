"""Seeded random cases of gs_fields_region_correlation: any plane shape up to 200 x 700, any admissible region shape, largest
lag, threshold count, sense and slab count 1..3, bit for bit against tests/region_corr_ref.py.  Every case runs: one whose
slab seam is no multiple of the region height asserts the refusal and then runs on one slab."""
import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, Simulation, capi
from tests import region_corr_ref

pytestmark = pytest.mark.gpu
CASES, GROUPS = 36, 6
ODD = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-40, 3.4028235e38], np.float32)


def case(seed):
    rng = np.random.default_rng(7000 + seed)
    rows, cols = int(rng.integers(1, 201)), int(rng.integers(1, 701))
    # region heights and widths from one cell (16 columns) to more than the plane, small ones as likely as large ones
    rh = int(rng.choice([1, 2, int(rng.integers(1, 17)), int(rng.integers(1, rows + 1)), rows, rows + int(rng.integers(1, 50))]))
    rw = 4 * int(rng.choice([4, 5, int(rng.integers(4, 17)), int(rng.integers(4, 65)), int(rng.integers(4, cols // 4 + 5)), cols // 4 + 4]))
    L = int(rng.choice([1, 2, int(rng.integers(1, 65)), 63, 64]))
    nt = int(rng.integers(1, 5))
    above = bool(rng.integers(0, 2))
    slabs = min(int(rng.integers(1, 4)), rows)                              # (one-row slabs occur)
    plane = (rng.random((rows, cols), dtype=np.float32) * np.float32(2.0) - np.float32(0.5)).astype(np.float32)
    if rng.integers(0, 2):                                                 # patches, so that long lags find pairs
        plane = np.where(np.add.outer(np.arange(rows) // 5, np.arange(cols) // 9) % 3 == 0, plane, np.float32(-1.0)).astype(np.float32)
    at = rng.choice(plane.size, size=min(plane.size, 2 * len(ODD)), replace=False)
    plane.flat[at] = np.resize(ODD, at.size)
    thresholds = [float(x) for x in rng.choice(np.array([0.3, -0.75, 0.0, 2.0 ** -130, 1.2, 0.9], np.float32), size=nt, replace=False)]
    plane.flat[rng.choice(plane.size, size=min(plane.size, 8), replace=False)] = np.float32(thresholds[0])   # cells equal to it
    return plane, (rh, rw), L, thresholds, above, slabs


def run(plane, region, L, thresholds, above, slabs):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * slabs))
    try:
        field = HipConcentration(sim.context, plane.shape)
        field.upload(sim.context, plane)
        return field.region_correlation(sim.context, region, thresholds, L, above)
    finally:
        sim.context.close()


@pytest.mark.parametrize("group", range(GROUPS))
def test_random_cases(built, group):
    for seed in range(group, CASES, GROUPS):
        plane, region, L, thresholds, above, slabs = case(seed)
        what = f"seed {seed}: plane {plane.shape} region {region} L {L} nt {len(thresholds)} above {above} slabs {slabs}"
        rows = plane.shape[0]
        aligned = all((k * rows // slabs) % region[0] == 0 for k in range(1, slabs))
        if not aligned:
            with pytest.raises(capi.GsError) as e:
                run(plane, region, L, thresholds, above, slabs)
            assert e.value.code == capi.GS_ERR_UNSUPPORTED, what
            slabs = 1
        got = run(plane, region, L, thresholds, above, slabs)
        assert len(got) == len(thresholds), what
        for c, t in zip(got, thresholds):
            wanted = region_corr_ref.pairs_by_label(plane, region, t, above, L)
            assert c.pairs.shape == wanted.shape and c.max_lag == L and c.above == above, what
            bad = np.argwhere(c.pairs != wanted)
            assert bad.size == 0, (f"{what} t {t}: {len(bad)} counters differ, first (i, j, k, d) = {tuple(bad[0])}: "
                                   f"{int(c.pairs[tuple(bad[0])])}, not {int(wanted[tuple(bad[0])])}")
