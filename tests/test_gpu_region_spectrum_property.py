"""Seeded random cases of gs_fields_region_spectrum: any plane shape up to 160 x 320, any region height in 1..160, any region
width that is a multiple of 4 in 16..320, a tile for which at least one region holds a tile, either window, NaNs sprinkled
at a rate of 1 in 2000 cells -- bit for bit against tests/region_spectrum_ref.py.  No more than a quarter of the cases have
every tile skipped or no tile at all: the seeds were chosen on the host with the reference, and the test asserts it."""
import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, Simulation
from grayscott_amd.simulation import spectrum_tables
from tests import region_spectrum_ref as ref
from tests import spectrum_ref

pytestmark = pytest.mark.gpu
CASES, BASE = 12, 4100


def case(seed):
    rng = np.random.default_rng(BASE + seed)
    while True:
        rows, cols = int(rng.integers(16, 161)), int(rng.integers(16, 321))
        rh, rw = int(rng.integers(1, 161)), 4 * int(rng.integers(4, 81))
        fits = [T for T in spectrum_ref.TILES if min(rh, rows) >= T and min(rw, cols) >= T]   # region (0, 0) is the largest
        if fits:
            break
    T = int(rng.choice(fits))
    window = int(rng.integers(0, 2))
    plane = rng.standard_normal((rows, cols)).astype(np.float32)
    plane[rng.random((rows, cols)) < 1.0 / 2000.0] = np.nan
    return plane, (rh, rw), T, window


def wanted(seed):
    plane, region, T, window = case(seed)
    h, w = spectrum_tables(T)
    return ref.by_crop(plane, region, T, window, h, w)


def test_the_cases_are_worth_running(built):
    empty = 0
    for seed in range(CASES):
        _, tiles = wanted(seed)
        empty += int(tiles[..., 0].sum() == 0)
    assert 4 * empty <= CASES, empty


@pytest.mark.parametrize("group", range(3))
def test_random_cases(built, group):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    for seed in range(group, CASES, 3):
        plane, region, T, window = case(seed)
        what = f"seed {seed}: plane {plane.shape} region {region} T {T} window {window}"
        f = HipConcentration(sim.context, plane.shape)
        f.upload(sim.context, plane)
        got = f.region_spectrum(sim.context, region, T, window)
        power, tiles = wanted(seed)
        assert got.raw.shape == power.shape, what
        assert np.array_equal(got.tiles_used, tiles[..., 0]) and np.array_equal(got.tiles_skipped, tiles[..., 1]), what
        bad = np.argwhere(got.raw.view(np.uint64) != power.view(np.uint64))
        assert bad.size == 0, f"{what}: {len(bad)} bins differ, first {tuple(bad[0])}"
        f.destroy()
    sim.context.close()
