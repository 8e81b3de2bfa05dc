"""Summaries in a multi-process context: gs_fields_summarize is collective and gives every rank the summary of the global
grid, bit for bit the single-process one.  All ranks share device 0 through the shared-memory transport double
(tests/cpp/shm_transport.cpp, built as tests/test_gpu_multiprocess.py builds it), whose messages hold at most 1 MiB: one
grid's row records exceed that per rank, so the all-gather goes in chunks."""
import os

import numpy as np
import pytest

from tests.children import rank_session, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, rows, cols, steps, out_dir, transport_lib, local_slabs):
    from grayscott_amd.simulation import SUMMARY_DTYPE
    from tests.helpers import species_from_arrays, stress_fields

    with rank_session(rank, world, port, transport_lib, rows, local_slabs) as (sim, (r0, r1)):
        u0, v0 = stress_fields((rows, cols), 4)
        species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(rows, cols))
        sim.perform_steps(species, steps)
        u, v = species.summary()
        in_u = species.in_out()[0]
        again = in_u.summary(sim.context)             # one plane alone: a second collective call
        rec = np.zeros(3, SUMMARY_DTYPE)
        for i, s in enumerate((u, v, again)):
            rec[i] = (s.sum, s.sum_sq, s.min, s.max, s.nonfinite)
        np.save(os.path.join(out_dir, f"rank{rank}.npy"), rec)


@pytest.mark.parametrize("world,local_slabs,rows,cols,steps", [
    (2, 1, 96, 300, 22),
    (3, 1, 1030, 777, 17),
    (2, 2, 301, 200, 9),
    (2, 1, 40000, 70, 5),       # 20000 rows per rank: 1.28 MB of records each, sent as two messages
])
def test_every_rank_gets_the_single_process_summary(tmp_path, built, shm_transport, world, local_slabs, rows, cols, steps):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from tests import summary_ref
    from tests.helpers import free_port, species_from_arrays, stress_fields

    spawn_ranks(_worker, (world, free_port(), rows, cols, steps, str(tmp_path), shm_transport, local_slabs), world)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = stress_fields((rows, cols), 4)
    species = species_from_arrays(sim, u0, v0)
    sim.perform_steps(species, steps)
    u, v = species.summary()
    in_u, in_v, _, _ = species.in_out()
    assert summary_ref.same(u, summary_ref.summary(in_u.make_scalar_view(sim.context)))
    assert summary_ref.same(v, summary_ref.summary(in_v.make_scalar_view(sim.context)))
    sim.context.close()
    for rank in range(world):
        rec = np.load(tmp_path / f"rank{rank}.npy")
        assert summary_ref.same(rec[0], u), (rank, rec[0], u)
        assert summary_ref.same(rec[1], v), (rank, rec[1], v)
        assert rec[2].tobytes() == rec[0].tobytes(), rank
