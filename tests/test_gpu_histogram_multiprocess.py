"""Histograms in a multi-process context: gs_fields_histogram is collective and gives every rank the counts of the global
grid, equal to the single-process ones.  All ranks share device 0 through the shared-memory transport double
(tests/cpp/shm_transport.cpp, built as tests/test_gpu_multiprocess.py builds it)."""
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS, U_RANGE, V_RANGE = 1000, (0.0, 1.0), (0.0, 0.5)


@pytest.fixture(scope="module")
def shm_transport(built):
    from tests.helpers import build_shm_transport

    return build_shm_transport()


def _counters(h):
    return np.concatenate([h.counts, np.array([h.below, h.above, h.nan], np.uint64)])


def _worker(rank, world, port, rows, cols, steps, out_dir, transport_lib, local_slabs):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from grayscott_amd import Parameters, Simulation
    from tests.helpers import join_ranks, species_from_arrays, stress_fields

    args, (r0, r1) = join_ranks(rank, world, port, transport_lib, rows, local_slabs)
    sim = Simulation.new(Parameters(), args)
    u0, v0 = stress_fields((rows, cols), 4)
    species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(rows, cols))
    sim.perform_steps(species, steps)
    u, v = species.histogram(BINS, U_RANGE, V_RANGE)
    in_u = species.in_out()[0]
    again = in_u.histogram(sim.context, BINS, U_RANGE)   # one plane alone: a second collective call
    np.save(os.path.join(out_dir, f"rank{rank}.npy"), np.stack([_counters(h) for h in (u, v, again)]))
    dist.barrier()
    sim.context.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,local_slabs,rows,cols,steps", [
    (2, 1, 96, 300, 22),
    (3, 1, 1030, 777, 17),
    (2, 2, 301, 200, 9),
])
def test_every_rank_gets_the_single_process_histogram(tmp_path, built, shm_transport, world, local_slabs, rows, cols, steps):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from tests import hist_ref
    from tests.helpers import free_port, species_from_arrays, stress_fields

    mp.spawn(_worker, args=(world, free_port(), rows, cols, steps, str(tmp_path), shm_transport, local_slabs),
             nprocs=world, join=True)
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
