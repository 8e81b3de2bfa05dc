"""Reduced result images in a multi-process context: each rank receives its own output rows, [row0 / f, ceil(row1 / f)),
and they are the matching rows of the single-process image, bit for bit; a (rows, world, f) triple in which some rank's
slab begins off a multiple of f is refused on every rank.  All ranks share device 0 through the shared-memory transport
double (tests/cpp/shm_transport.cpp, built as tests/test_gpu_multiprocess.py builds it)."""
import os

import numpy as np
import pytest

from tests.children import rank_session, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
FACTORS = (2, 3, 4, 5, 8, 16, 64)


def _worker(rank, world, port, rows, cols, steps, out_dir, transport_lib, local_slabs):
    from grayscott_amd import capi
    from grayscott_amd.simulation import pinned_empty
    from tests import reduce_ref
    from tests.helpers import species_from_arrays, stress_fields

    with rank_session(rank, world, port, transport_lib, rows, local_slabs) as (sim, (r0, r1)):
        S = world * local_slabs
        u0, v0 = stress_fields((rows, cols), 4)
        species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(rows, cols))
        sim.perform_steps(species, steps)
        in_v = species.in_out()[1]
        out = {}
        for f in FACTORS:
            if not reduce_ref.slab_rule(rows, S, f):
                codes = []
                for call in (lambda: in_v.reduced_shape(f), lambda: species.make_result_view(reduce=f)):
                    try:
                        call()
                        codes.append(0)
                    except capi.GsError as e:
                        codes.append(e.code)
                out[f"refused{f}"] = np.array(codes)
                continue
            lo, hi = reduce_ref.local_rows(rows, S, rank * local_slabs, local_slabs, f)
            assert in_v.reduced_shape(f) == (hi - lo, -(-cols // f)), (rank, f, in_v.reduced_shape(f))
            out[f"blocking{f}"] = species.make_result_view(reduce=f)
            image = pinned_empty((hi - lo, -(-cols // f)))
            species.write_result_view_after(image, reduce=f)
            sim.context.download_wait()
            out[f"overlapped{f}"] = np.array(image)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)


@pytest.mark.parametrize("world,local_slabs,rows,cols,steps", [
    (2, 1, 96, 300, 22),        # slabs begin at 0 and 48: 5 and 64 are refused
    (3, 1, 1030, 777, 17),      # 0, 343, 686: every factor of the list is refused, on every rank
    (3, 1, 960, 517, 17),       # 0, 320, 640: everything up to 64 goes
    (2, 2, 304, 200, 9),        # four slabs of 76 rows: 2 and 4 go
])
def test_each_rank_gets_its_rows_of_the_single_process_image(tmp_path, built, shm_transport, world, local_slabs, rows, cols, steps):
    from grayscott_amd import HipArgs, Parameters, Simulation, capi
    from tests import reduce_ref
    from tests.helpers import free_port, species_from_arrays, stress_fields

    spawn_ranks(_worker, (world, free_port(), rows, cols, steps, str(tmp_path), shm_transport, local_slabs), world)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = stress_fields((rows, cols), 4)
    species = species_from_arrays(sim, u0, v0)
    sim.perform_steps(species, steps)
    plane = species.make_result_view()
    S = world * local_slabs
    admitted = 0
    for f in FACTORS:
        whole = species.make_result_view(reduce=f)                 # one slab: every factor goes
        assert reduce_ref.same_bits(whole, reduce_ref.reduce(plane, f)), f
        for rank in range(world):
            z = np.load(tmp_path / f"rank{rank}.npz")
            if not reduce_ref.slab_rule(rows, S, f):
                assert list(z[f"refused{f}"]) == [capi.GS_ERR_UNSUPPORTED] * 2, (rank, f, z[f"refused{f}"])
                continue
            lo, hi = reduce_ref.local_rows(rows, S, rank * local_slabs, local_slabs, f)
            for form in ("blocking", "overlapped"):
                assert reduce_ref.same_bits(z[f"{form}{f}"], whole[lo:hi]), (rank, f, form)
            admitted += 1
    sim.context.close()
    assert (admitted > 0) == any(reduce_ref.slab_rule(rows, S, f) for f in FACTORS)
