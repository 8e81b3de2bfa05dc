"""The three users of the set rule of grayscott_amd/csrc/gs_plane_scan.h -- bit-quad counts, pair counts, connected
components -- asked about the same planes: the set cells each of them reports are numpy's count by the rule as
include/gs_hip.h words it, at the shapes where the shared four-column load and the shared rule can go wrong."""
import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, Simulation, capi
from grayscott_amd.simulation import quad_measures

pytestmark = pytest.mark.gpu

QUARTER = np.float32(0.25)
SPECIAL = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 2.0 ** -140, QUARTER, np.nextafter(QUARTER, np.float32(1)),
                    np.nextafter(QUARTER, np.float32(-1))], np.float32)
THRESHOLDS = [float("-inf"), 0.0, 0.25, float("inf")]


def cells(shape, seed) -> np.ndarray:
    """Two cells in three from SPECIAL, the others uniform in [-0.5, 1)."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, 3 * len(SPECIAL) // 2, size=shape)
    uniform = (rng.random(shape, dtype=np.float32) * np.float32(1.5) - np.float32(0.5)).astype(np.float32)
    return np.where(pick < len(SPECIAL), SPECIAL[np.minimum(pick, len(SPECIAL) - 1)], uniform).astype(np.float32)


def counted(plane: np.ndarray, t: float, above: bool) -> int:
    """above ? x > t : x < t, NaN never (both comparisons are false for it)."""
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(plane > np.float32(t) if above else plane < np.float32(t)))


def test_morphology_correlation_and_components_agree_on_the_set_cells(built):
    checked = 0
    # one (1, 1) plane; one strip plus one column; a tile row plus one -- in one slab and in two slabs on one GPU
    for devices in ([0], [0, 0]):
        sim = Simulation.new(Parameters(), HipArgs(devices=devices))
        for shape in ((1, 1), (17, 255), (33, 257)):
            if shape[0] < len(devices):  # every slab holds a row: gs_field_create refuses to cut one row in two
                with pytest.raises(capi.GsError) as e:
                    HipConcentration(sim.context, shape)
                assert e.value.code == capi.GS_ERR_INVALID
                continue
            field = HipConcentration(sim.context, shape)
            for seed, above in enumerate((True, False)):
                plane = cells(shape, 100 * shape[1] + seed)
                field.upload(sim.context, plane)
                want = [counted(plane, t, above) for t in THRESHOLDS]
                area = [m.area for m in field.morphology(sim.context, THRESHOLDS, above)]
                comp = [c.set_cells for c in field.components(sim.context, THRESHOLDS, above, 8)]
                print(f"{len(devices)} slab(s) {shape} above {above}: numpy {want} morphology {area} components {comp}")
                assert area == want and comp == want
                for c, n in zip(field.correlation(sim.context, THRESHOLDS, 1, above), want):
                    assert [int(c.pairs[k, 0]) for k in range(4)] == [n] * 4, (shape, above, c.threshold)
                checked += 1
            field.destroy()
        sim.context.close()
    assert checked == 10
    # ensembles, U set below its thresholds and V above: three members of (17, 13) -- a member's 221 cells are no multiple of
    # 4: the ragged loads -- and of (16, 260): the 16-byte loads
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    for shape in ((17, 13), (16, 260)):
        ens = sim.make_ensemble(shape, Parameters(), members=3)
        u, v = cells((3,) + shape, shape[1]), cells((3,) + shape, shape[1] + 1)
        ens.upload(u, v)
        want = np.array([[[counted(p[i], t, s == 1) for t in THRESHOLDS] for s, p in enumerate((u, v))] for i in range(3)])
        area = quad_measures(ens.morphologies(v_thresholds=THRESHOLDS, u_thresholds=THRESHOLDS))[0]
        comp = ens.components(v_thresholds=THRESHOLDS, u_thresholds=THRESHOLDS)[..., 1].astype(np.int64)
        pairs = ens.correlations(v_thresholds=THRESHOLDS, u_thresholds=THRESHOLDS, max_lag=1)[..., 0].astype(np.int64)
        print(f"ensemble {shape}: numpy {want.tolist()}")
        assert np.array_equal(area, want) and np.array_equal(comp, want)
        assert pairs.shape == (3, 2, 4, 4) and np.array_equal(pairs, np.repeat(want[..., None], 4, axis=-1))
        ens.destroy()
    sim.context.close()
