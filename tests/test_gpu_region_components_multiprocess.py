"""Regional connected components in a multi-process context: gs_fields_region_components is collective and gives every rank
every region, equal to the single-process result; a rank seam that is no multiple of the region height is refused on every
rank alike.  All ranks share device 0 through the shared-memory transport double (tests/cpp/shm_transport.cpp, built as
tests/test_gpu_multiprocess.py builds it)."""
import os

import numpy as np
import pytest

from tests.children import rank_session, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
ROWS, COLS, WORLD = 96, 300, 2
TV, TU = (0.25, 0.1), (0.5, 0.8)
ALIGNED = [((16, 64), 8), ((48, 256), 4)]      # region shapes whose rows the rank seam (row 48) is a multiple of, and a connectivity
UNALIGNED = (32, 64)                           # ... and one that it is not


def _planes():
    from tests.helpers import stress_fields

    u, v = stress_fields((ROWS, COLS), 14)
    v[47:49] = np.float32(0.45)                # a bar across the rank seam, which is a wall: it counts on either side
    v[31:33, ::2] = np.float32(-1.0)
    u[63:65, ::3] = np.float32(np.nan)
    return u, v


def _results(species, region, connectivity):
    cu, cv = species.region_components(region, TV, TU, connectivity=connectivity)
    return [c.counters() for c in cu + cv]


def _worker(rank, world, port, out_dir, transport_lib):
    from grayscott_amd import capi
    from tests.helpers import species_from_arrays

    with rank_session(rank, world, port, transport_lib, ROWS) as (sim, (r0, r1)):
        u0, v0 = _planes()
        species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(ROWS, COLS))
        before = sim.context.stats()
        got = {}
        for k, (region, connectivity) in enumerate(ALIGNED):
            for i, a in enumerate(_results(species, region, connectivity)):
                got[f"r{k}_{i}"] = a
        try:
            species.region_components(UNALIGNED, TV, TU)
            refused = 0
        except capi.GsError as e:
            refused = e.code
        for i, a in enumerate(_results(species, *ALIGNED[0])):                 # the context goes on working
            assert np.array_equal(a, got[f"r0_{i}"])
        assert sim.context.stats() == before
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), refused=np.array(refused), **got)


def test_every_rank_gets_every_region(tmp_path, built, shm_transport):
    from grayscott_amd import HipArgs, Parameters, Simulation, capi
    from tests import region_components_ref
    from tests.helpers import free_port, species_from_arrays

    spawn_ranks(_worker, (WORLD, free_port(), str(tmp_path), shm_transport), WORLD)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = _planes()
    species = species_from_arrays(sim, u0, v0)
    for k, (region, connectivity) in enumerate(ALIGNED):
        want = _results(species, region, connectivity)
        for j in range(2):
            assert np.array_equal(want[j], region_components_ref.counters(u0, region, TU[j], False, connectivity))
            assert np.array_equal(want[2 + j], region_components_ref.counters(v0, region, TV[j], True, connectivity))
        for rank in range(WORLD):
            z = np.load(tmp_path / f"rank{rank}.npz")
            assert int(z["refused"]) == capi.GS_ERR_UNSUPPORTED, (rank, z["refused"])
            for i, a in enumerate(want):
                assert z[f"r{k}_{i}"].dtype == a.dtype and z[f"r{k}_{i}"].tobytes() == a.tobytes(), (rank, region, i)
    sim.context.close()
