"""Seeded random cases of gs_fields_region_components: any plane shape up to 80 x 600, any admissible region shape, threshold,
sense, connectivity, pattern kind, 1..4 thresholds and slab count 1..3, every counter against tests/region_components_ref.py
and the three invariants of the header against the whole-grid restatement.  Every case runs: one whose slab seam is no
multiple of the region height asserts the refusal and then runs on one slab."""
import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, Simulation, capi
from tests import observe_cases, region_components_ref

pytestmark = pytest.mark.gpu
CASES, GROUPS = 36, 6
THRESHOLDS = [0.25, 0.0, -1.5, 2.0 ** -130, 3.0e38, float("inf"), float("-inf")]
KINDS = ["planted", "serpentine", "comb", "rings", "checkerboard", "staircase", "u_shape", "full", "empty", "one-set", "one-unset",
         "seams", "lane_runs"]


def case(seed):
    rng = np.random.default_rng(7000 + seed)
    rows, cols = int(rng.integers(1, 81)), int(rng.integers(1, 601))
    # region heights and widths from one cell (16 columns) to more than the plane, small ones as likely as large ones
    rh = int(rng.choice([1, 2, int(rng.integers(1, 17)), 16, int(rng.integers(1, rows + 1)), rows + int(rng.integers(0, 50))]))
    rw = 4 * int(rng.choice([4, 5, int(rng.integers(4, 17)), 64, int(rng.integers(4, cols // 4 + 5)), cols // 4 + 4]))
    nt = int(rng.integers(1, 5))
    thresholds = [THRESHOLDS[int(i)] for i in rng.choice(len(THRESHOLDS), size=nt, replace=False)]
    above, connectivity = bool(rng.integers(0, 2)), int(rng.choice([4, 8]))
    kind = KINDS[int(rng.integers(0, len(KINDS)))]
    density = observe_cases.DENSITIES[int(rng.integers(0, len(observe_cases.DENSITIES)))]
    slabs = min(int(rng.integers(1, 4)), rows)                              # (one-row slabs occur)
    plane = observe_cases.plane(kind, (rows, cols), thresholds[0], above, 100 * seed, density, slabs=slabs)
    return plane, (rh, rw), thresholds, above, connectivity, slabs, kind


def run(plane, region, thresholds, above, connectivity, slabs):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * slabs))
    try:
        field = HipConcentration(sim.context, plane.shape)
        field.upload(sim.context, plane)
        return field.region_components(sim.context, region, thresholds, above, connectivity)
    finally:
        sim.context.close()


@pytest.mark.parametrize("group", range(GROUPS))
def test_random_cases(built, group):
    for seed in range(group, CASES, GROUPS):
        plane, region, thresholds, above, connectivity, slabs, kind = case(seed)
        what = (f"seed {seed}: {kind} {plane.shape} region {region} thresholds {thresholds} above {above} connectivity {connectivity} "
                f"slabs {slabs}")
        rows = plane.shape[0]
        aligned = all((k * rows // slabs) % region[0] == 0 for k in range(1, slabs))
        if not aligned:
            with pytest.raises(capi.GsError) as e:
                run(plane, region, thresholds, above, connectivity, slabs)
            assert e.value.code == capi.GS_ERR_UNSUPPORTED, what
            slabs = 1
        got = run(plane, region, thresholds, above, connectivity, slabs)
        assert len(got) == len(thresholds), what
        for c, t in zip(got, thresholds):
            wanted = region_components_ref.counters(plane, region, t, above, connectivity)
            words = c.counters()
            assert words.shape == wanted.shape and c.threshold == float(np.float32(t)), what
            bad = np.argwhere(words != wanted)
            assert bad.size == 0, (f"{what} t {t}: {len(bad)} counters differ, first (i, j, word) = {tuple(bad[0])}: "
                                   f"{int(words[tuple(bad[0])])}, not {int(wanted[tuple(bad[0])])}")
            region_components_ref.invariants(plane, region, t, above, connectivity, words)
