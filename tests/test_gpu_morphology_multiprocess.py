"""Bit-quad counts in a multi-process context: gs_fields_morphology is collective and gives every rank the counts of the
global grid, equal to the single-process ones -- right after the upload, when every ghost row is stale, and after steps.
The quads across the rank seam need the last row of the rank above: it travels with the call.  All ranks share device 0
through the shared-memory transport double (tests/cpp/shm_transport.cpp, built as tests/test_gpu_multiprocess.py builds it)."""
import os

import numpy as np
import pytest

from tests.children import rank_session, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
TV, TU = (0.25, 0.1), (0.5, 0.8)


def _planes(rows, cols, slabs):
    """U and V with set cells (U below 0.5, V above 0.25) planted on both sides of every seam of `slabs` slabs."""
    from tests.helpers import stress_fields

    u, v = stress_fields((rows, cols), 4)
    rng = np.random.default_rng(6)
    for i in range(1, slabs):
        seam = i * rows // slabs
        for r in (seam - 1, seam):
            on = rng.random(cols) < 0.6
            u[r] = np.where(on, np.float32(0.1), np.float32(0.9))
            v[r] = np.where(on, np.float32(0.45), np.float32(0.01))
    return u, v


def _quads(species):
    mu, mv = species.morphology(TV, TU)
    return np.stack([m.quads for m in mu + mv])


def _worker(rank, world, port, rows, cols, steps, out_dir, transport_lib, local_slabs):
    from tests.helpers import species_from_arrays

    with rank_session(rank, world, port, transport_lib, rows, local_slabs) as (sim, (r0, r1)):
        u0, v0 = _planes(rows, cols, world * local_slabs)
        species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(rows, cols))
        before = sim.context.stats()
        fresh = _quads(species)                                   # right after the upload: ghost rows stale
        assert sim.context.stats() == before
        sim.perform_steps(species, steps)
        before = sim.context.stats()
        later = _quads(species)
        assert sim.context.stats() == before
        alone = species.in_out()[1].morphology(sim.context, [TV[0]])[0].quads   # one plane alone: another collective call
        np.save(os.path.join(out_dir, f"rank{rank}.npy"), np.concatenate([fresh, later, alone[None]]))


@pytest.mark.parametrize("world,local_slabs,rows,cols,steps", [
    (2, 1, 50, 333, 5),
    (2, 2, 50, 333, 5),
])
def test_every_rank_gets_the_single_process_morphology(tmp_path, built, shm_transport, world, local_slabs, rows, cols, steps):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from tests import morph_ref
    from tests.helpers import free_port, species_from_arrays

    spawn_ranks(_worker, (world, free_port(), rows, cols, steps, str(tmp_path), shm_transport, local_slabs), world)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = _planes(rows, cols, world * local_slabs)
    species = species_from_arrays(sim, u0, v0)
    fresh = _quads(species)
    for k in range(2):
        assert np.array_equal(fresh[k], morph_ref.quads(u0, TU[k], False)) and np.array_equal(fresh[2 + k], morph_ref.quads(v0, TV[k], True))
    sim.perform_steps(species, steps)
    later = _quads(species)
    in_u, in_v, _, _ = species.in_out()
    u, v = in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)
    for k in range(2):
        assert np.array_equal(later[k], morph_ref.quads(u, TU[k], False)) and np.array_equal(later[2 + k], morph_ref.quads(v, TV[k], True))
    sim.context.close()
    for rank in range(world):
        rec = np.load(tmp_path / f"rank{rank}.npy")
        assert rec.dtype == np.uint64 and rec.shape == (9, 6) and np.all(rec.sum(axis=1) == (rows + 1) * (cols + 1))
        assert np.array_equal(rec[:4], fresh), (rank, rec[:4], fresh)
        assert np.array_equal(rec[4:8], later), (rank, rec[4:8], later)
        assert np.array_equal(rec[8], later[2]), rank
