"""Histograms in a multi-process context: gs_fields_histogram is collective and gives every rank the counts of the global
grid, equal to the single-process ones.  All ranks share device 0 through the shared-memory transport double
(tests/cpp/shm_transport.cpp, built as tests/test_gpu_multiprocess.py builds it)."""
import os

import numpy as np
import pytest

from tests.children import rank_session, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
BINS, U_RANGE, V_RANGE = 1000, (0.0, 1.0), (0.0, 0.5)


def _counters(h):
    return np.concatenate([h.counts, np.array([h.below, h.above, h.nan], np.uint64)])


def _worker(rank, world, port, rows, cols, steps, out_dir, transport_lib, local_slabs):
    from tests.helpers import species_from_arrays, stress_fields

    with rank_session(rank, world, port, transport_lib, rows, local_slabs) as (sim, (r0, r1)):
        u0, v0 = stress_fields((rows, cols), 4)
        species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(rows, cols))
        sim.perform_steps(species, steps)
        u, v = species.histogram(BINS, U_RANGE, V_RANGE)
        in_u = species.in_out()[0]
        again = in_u.histogram(sim.context, BINS, U_RANGE)   # one plane alone: a second collective call
        np.save(os.path.join(out_dir, f"rank{rank}.npy"), np.stack([_counters(h) for h in (u, v, again)]))


@pytest.mark.parametrize("world,local_slabs,rows,cols,steps", [
    (2, 1, 96, 300, 22),
    (3, 1, 1030, 777, 17),
    (2, 2, 301, 200, 9),
])
def test_every_rank_gets_the_single_process_histogram(tmp_path, built, shm_transport, world, local_slabs, rows, cols, steps):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from tests import hist_ref
    from tests.helpers import free_port, species_from_arrays, stress_fields

    spawn_ranks(_worker, (world, free_port(), rows, cols, steps, str(tmp_path), shm_transport, local_slabs), world)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = stress_fields((rows, cols), 4)
    species = species_from_arrays(sim, u0, v0)
    sim.perform_steps(species, steps)
    u, v = species.histogram(BINS, U_RANGE, V_RANGE)
    in_u, in_v, _, _ = species.in_out()
    assert np.array_equal(_counters(u), hist_ref.histogram(in_u.make_scalar_view(sim.context), *U_RANGE, BINS))
    assert np.array_equal(_counters(v), hist_ref.histogram(in_v.make_scalar_view(sim.context), *V_RANGE, BINS))
    sim.context.close()
    for rank in range(world):
        rec = np.load(tmp_path / f"rank{rank}.npy")
        assert rec.dtype == np.uint64 and int(rec[0].sum()) == rows * cols
        assert np.array_equal(rec[0], _counters(u)), rank
        assert np.array_equal(rec[1], _counters(v)), rank
        assert np.array_equal(rec[2], rec[0]), rank
