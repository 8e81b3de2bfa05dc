"""Comparisons and snapshots in a multi-process context: gs_fields_compare is collective and gives every rank the result of
the global grid, bit for bit the single-process one; gs_fields_copy copies every process's own rows, and a restore
followed by steps gives the single-process planes.  All ranks share device 0 through the shared-memory transport double
(tests/cpp/shm_transport.cpp, built as tests/test_gpu_multiprocess.py builds it); the rows do not divide evenly."""
import os

import numpy as np
import pytest

from tests.children import rank_session, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
BEFORE, BETWEEN, AFTER = 6, 13, 8      # steps before the snapshot, between snapshot and comparison, after the restore


def _scenario(sim, species, rec):
    """Snapshot, steps, comparison (twice: U and V together, then V alone), restore, steps.  Fills rec[0:3]."""
    sim.perform_steps(species, BEFORE)
    snap = species.snapshot()
    sim.perform_steps(species, BETWEEN)
    u, v = species.change_since(snap)
    again = species.in_out()[1].change_from(sim.context, snap.v)     # one pair alone: a second collective call
    for i, c in enumerate((u, v, again)):
        rec[i] = (c.sum_abs, c.sum_sq, c.max_abs, c.differing, c.nonfinite)
    species.restore(snap)
    sim.perform_steps(species, AFTER)
    in_u, in_v, _, _ = species.in_out()
    return in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)


def _worker(rank, world, port, rows, cols, out_dir, transport_lib, local_slabs):
    from grayscott_amd.simulation import CHANGE_DTYPE
    from tests.helpers import species_from_arrays, stress_fields

    with rank_session(rank, world, port, transport_lib, rows, local_slabs) as (sim, (r0, r1)):
        u0, v0 = stress_fields((rows, cols), 4)
        species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(rows, cols))
        rec = np.zeros(3, CHANGE_DTYPE)
        u, v = _scenario(sim, species, rec)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), rec=rec, u=u, v=v, rows=np.array([r0, r1]))


@pytest.mark.parametrize("world,local_slabs", [(2, 1), (2, 2), (3, 1)])
def test_every_rank_gets_the_single_process_change(tmp_path, built, shm_transport, world, local_slabs):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from grayscott_amd.simulation import CHANGE_DTYPE
    from tests import change_ref
    from tests.helpers import free_port, species_from_arrays, stress_fields

    rows, cols = 203, 333
    spawn_ranks(_worker, (world, free_port(), rows, cols, str(tmp_path), shm_transport, local_slabs), world)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = stress_fields((rows, cols), 4)
    species = species_from_arrays(sim, u0, v0)
    want = np.zeros(3, CHANGE_DTYPE)
    u, v = _scenario(sim, species, want)
    sim.context.close()
    # the single-process result is the restatement's
    from tests.helpers import gpu_run

    before = gpu_run(u0, v0, BEFORE)
    after = gpu_run(u0, v0, BEFORE + BETWEEN)
    assert change_ref.same(want[0], change_ref.change(after[0], before[0]))
    assert change_ref.same(want[1], change_ref.change(after[1], before[1]))
    assert want[2].tobytes() == want[1].tobytes() and want[0]["differing"] > 0
    covered = 0
    for rank in range(world):
        z = np.load(tmp_path / f"rank{rank}.npz")
        assert z["rec"].tobytes() == want.tobytes(), (rank, z["rec"], want)
        r0, r1 = z["rows"]
        assert z["u"].tobytes() == u[r0:r1].tobytes() and z["v"].tobytes() == v[r0:r1].tobytes(), rank
        covered += r1 - r0
    assert covered == rows
