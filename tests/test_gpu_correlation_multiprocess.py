"""Two-point pair counts in a multi-process context: gs_fields_correlation is collective and gives every rank the counts of
the global grid, equal to the single-process ones -- right after the upload, when every ghost row is stale, and after steps.
The pairs across a rank seam need the last L rows of the rank above: they travel with the call.  A slab shorter than L is
refused on every rank.  All ranks share device 0 through the shared-memory transport double (tests/cpp/shm_transport.cpp,
built as tests/test_gpu_multiprocess.py builds it)."""
import os

import numpy as np
import pytest

from tests.children import rank_session, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
TV, TU = (0.25, 0.1), (0.5, 0.8)


def _planes(rows, cols):
    """U and V with cells set at density 1/2 (U below 0.5 and 0.8, V above 0.25 and 0.1): set cells at every lag across
    every seam."""
    rng = np.random.default_rng(6)
    u = np.where(rng.random((rows, cols)) < 0.5, np.float32(0.1), np.float32(0.9)).astype(np.float32)
    v = np.where(rng.random((rows, cols)) < 0.5, np.float32(0.45), np.float32(0.01)).astype(np.float32)
    return u, v


def _pairs(species, lag):
    cu, cv = species.correlation(TV, TU, max_lag=lag)
    return np.stack([c.pairs for c in cu + cv])


def _worker(rank, world, port, rows, cols, steps, lag, too_long, out_dir, transport_lib, local_slabs):
    from grayscott_amd import capi
    from tests.helpers import species_from_arrays

    with rank_session(rank, world, port, transport_lib, rows, local_slabs) as (sim, (r0, r1)):
        u0, v0 = _planes(rows, cols)
        species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(rows, cols))
        before = sim.context.stats()
        fresh = _pairs(species, lag)                              # right after the upload: ghost rows stale
        assert sim.context.stats() == before
        try:                                                      # a slab shorter than the lag: refused here as on every rank
            _pairs(species, too_long)
            refused = 0
        except capi.GsError as e:
            refused = e.code
        sim.perform_steps(species, steps)
        before = sim.context.stats()
        later = _pairs(species, lag)
        assert sim.context.stats() == before
        alone = species.in_out()[1].correlation(sim.context, [TV[0]], lag)[0].pairs   # one plane alone: another collective call
        np.save(os.path.join(out_dir, f"rank{rank}.npy"), np.concatenate([fresh, later, alone[None]]))
        np.save(os.path.join(out_dir, f"refused{rank}.npy"), np.array([refused]))


@pytest.mark.parametrize("world,local_slabs,rows,cols,steps,lag,too_long", [
    (2, 1, 50, 333, 5, 16, 26),       # slabs of 25 rows
    (3, 1, 50, 333, 5, 16, 17),       # slabs of 16, 17, 17 rows: the first is the short one
    (2, 2, 50, 333, 5, 12, 13),       # four slabs of 12, 13, 12, 13 rows, two per rank
])
def test_every_rank_gets_the_single_process_correlation(tmp_path, built, shm_transport, world, local_slabs, rows, cols, steps,
                                                         lag, too_long):
    from grayscott_amd import HipArgs, Parameters, Simulation, capi
    from tests import corr_ref
    from tests.helpers import free_port, species_from_arrays

    spawn_ranks(_worker, (world, free_port(), rows, cols, steps, lag, too_long, str(tmp_path), shm_transport, local_slabs), world)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = _planes(rows, cols)
    species = species_from_arrays(sim, u0, v0)
    fresh = _pairs(species, lag)
    for k in range(2):
        assert np.array_equal(fresh[k], corr_ref.pairs(u0, TU[k], False, lag))
        assert np.array_equal(fresh[2 + k], corr_ref.pairs(v0, TV[k], True, lag))
    sim.perform_steps(species, steps)
    later = _pairs(species, lag)
    in_u, in_v, _, _ = species.in_out()
    u, v = in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)
    for k in range(2):
        assert np.array_equal(later[k], corr_ref.pairs(u, TU[k], False, lag))
        assert np.array_equal(later[2 + k], corr_ref.pairs(v, TV[k], True, lag))
    sim.context.close()
    for rank in range(world):
        rec = np.load(tmp_path / f"rank{rank}.npy")
        assert rec.dtype == np.uint64 and rec.shape == (9, 4, lag + 1)
        assert np.array_equal(rec[:4], fresh), (rank, rec[:4], fresh)
        assert np.array_equal(rec[4:8], later), (rank, rec[4:8], later)
        assert np.array_equal(rec[8], later[2]), rank
        assert int(np.load(tmp_path / f"refused{rank}.npy")[0]) == capi.GS_ERR_UNSUPPORTED, rank
