"""Regional histograms in a multi-process context: gs_fields_region_histogram is collective and gives every rank every
region, equal to the single-process result; a rank seam that is no multiple of the region height is refused on every rank
alike.  All ranks share device 0 through the shared-memory transport double (tests/cpp/shm_transport.cpp, built as
tests/test_gpu_multiprocess.py builds it)."""
import os

import numpy as np
import pytest

from tests.children import rank_session, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
ROWS, COLS, BINS = 96, 300, 100
RANGE_U, RANGE_V = (0.0, 1.0), (-0.125, 0.5)
ALIGNED = {2: [(16, 64), (48, 256)], 3: [(16, 64), (32, 320)]}     # region shapes whose rows every rank seam is a multiple of
UNALIGNED = {2: (32, 64), 3: (24, 64)}                              # ... and one that a seam (48; 32) is not


def _planes():
    from tests.helpers import stress_fields

    u, v = stress_fields((ROWS, COLS), 14)
    v[47:49] = np.float32(0.45)
    v[31:33, ::2] = np.float32(-1.0)
    u[63:65, ::3] = np.float32(np.nan)
    return u, v


def _results(species, region):
    from tests import region_hist_ref

    return [region_hist_ref.counters_of(h) for h in species.region_histogram(region, BINS, RANGE_U, RANGE_V)]


def _worker(rank, world, port, out_dir, transport_lib):
    from grayscott_amd import capi
    from tests.helpers import species_from_arrays

    with rank_session(rank, world, port, transport_lib, ROWS) as (sim, (r0, r1)):
        u0, v0 = _planes()
        species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(ROWS, COLS))
        before = sim.context.stats()
        got = {}
        for k, region in enumerate(ALIGNED[world]):
            for i, a in enumerate(_results(species, region)):
                got[f"r{k}_{i}"] = a
        try:
            species.region_histogram(UNALIGNED[world], BINS, RANGE_U, RANGE_V)
            refused = 0
        except capi.GsError as e:
            refused = e.code
        for i, a in enumerate(_results(species, ALIGNED[world][0])):           # the context goes on working
            assert np.array_equal(a, got[f"r0_{i}"])
        assert sim.context.stats() == before
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), refused=np.array(refused), **got)


@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_gets_every_region(tmp_path, built, shm_transport, world):
    from grayscott_amd import HipArgs, Parameters, Simulation, capi
    from tests import region_hist_ref
    from tests.helpers import free_port, species_from_arrays

    spawn_ranks(_worker, (world, free_port(), str(tmp_path), shm_transport), world)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = _planes()
    species = species_from_arrays(sim, u0, v0)
    for k, region in enumerate(ALIGNED[world]):
        want = _results(species, region)
        assert np.array_equal(want[0], region_hist_ref.by_label(u0, region, RANGE_U[0], RANGE_U[1], BINS))
        assert np.array_equal(want[1], region_hist_ref.by_label(v0, region, RANGE_V[0], RANGE_V[1], BINS))
        for rank in range(world):
            z = np.load(tmp_path / f"rank{rank}.npz")
            assert int(z["refused"]) == capi.GS_ERR_UNSUPPORTED, (rank, z["refused"])
            for i, a in enumerate(want):
                assert z[f"r{k}_{i}"].dtype == a.dtype and z[f"r{k}_{i}"].tobytes() == a.tobytes(), (rank, region, i)
    sim.context.close()
