"""Connected components in a multi-process context: gs_fields_components is collective and gives every rank the result of
the global grid, equal to the single-process one -- right after the upload, when every ghost row is stale, and after steps.
Every rank's seam rows and counters travel with the call and every rank does the same merge.  All ranks share device 0
through the shared-memory transport double (tests/cpp/shm_transport.cpp, built as tests/test_gpu_multiprocess.py builds it)."""
import os

import numpy as np
import pytest

from tests.children import rank_session, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
TV, TU = (0.25, 0.1), (0.5, 0.8)


def _planes(rows, cols, slabs):
    """V carries a serpentine through the whole plane (set above 0.25 and 0.1); U random cells with set cells (below 0.5)
    planted on both sides of every seam of `slabs` slabs."""
    from tests import components_ref
    from tests.helpers import stress_fields

    u, _ = stress_fields((rows, cols), 4)
    rng = np.random.default_rng(6)
    for i in range(1, slabs):
        seam = i * rows // slabs
        for r in (seam - 1, seam):
            u[r] = np.where(rng.random(cols) < 0.6, np.float32(0.1), np.float32(0.9))
    v = (components_ref.serpentine((rows, cols)) * np.float32(0.45)).astype(np.float32)
    return u, v


def _words(species):
    out = []
    for conn in (8, 4):
        cu, cv = species.components(TV, TU, connectivity=conn)
        out += [np.concatenate([np.array([c.count, c.set_cells, c.largest], np.uint64), c.by_size]) for c in cu + cv]
    return np.stack(out)


def _worker(rank, world, port, rows, cols, steps, out_dir, transport_lib, local_slabs):
    from tests.helpers import species_from_arrays

    with rank_session(rank, world, port, transport_lib, rows, local_slabs) as (sim, (r0, r1)):
        u0, v0 = _planes(rows, cols, world * local_slabs)
        species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(rows, cols))
        before = sim.context.stats()
        fresh = _words(species)                                   # right after the upload: ghost rows stale
        assert sim.context.stats() == before
        sim.perform_steps(species, steps)
        before = sim.context.stats()
        later = _words(species)
        assert sim.context.stats() == before
        np.save(os.path.join(out_dir, f"rank{rank}.npy"), np.concatenate([fresh, later]))


@pytest.mark.parametrize("world,local_slabs,rows,cols,steps", [
    (2, 1, 50, 333, 5),
    (2, 2, 50, 333, 5),
])
def test_every_rank_gets_the_single_process_components(tmp_path, built, shm_transport, world, local_slabs, rows, cols, steps):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from tests import components_ref
    from tests.helpers import free_port, species_from_arrays

    spawn_ranks(_worker, (world, free_port(), rows, cols, steps, str(tmp_path), shm_transport, local_slabs), world)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = _planes(rows, cols, world * local_slabs)
    species = species_from_arrays(sim, u0, v0)
    fresh = _words(species)
    for j, conn in enumerate((8, 4)):
        for k in range(2):
            assert np.array_equal(fresh[4 * j + k], components_ref.counters(u0, TU[k], False, conn))
            assert np.array_equal(fresh[4 * j + 2 + k], components_ref.counters(v0, TV[k], True, conn))
    assert fresh[2, 0] == 1 and fresh[6, 0] == 1              # the serpentine is one component, under 8 and under 4
    sim.perform_steps(species, steps)
    later = _words(species)
    in_u, in_v, _, _ = species.in_out()
    u, v = in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)
    for j, conn in enumerate((8, 4)):
        for k in range(2):
            assert np.array_equal(later[4 * j + k], components_ref.counters(u, TU[k], False, conn))
            assert np.array_equal(later[4 * j + 2 + k], components_ref.counters(v, TV[k], True, conn))
    sim.context.close()
    for rank in range(world):
        rec = np.load(tmp_path / f"rank{rank}.npy")
        assert rec.dtype == np.uint64 and rec.shape == (16, 35)
        assert np.array_equal(rec[:8], fresh), (rank, rec[:8], fresh)
        assert np.array_equal(rec[8:], later), (rank, rec[8:], later)
