"""Domain masks in a two-process run (gs_ctx_set_mask is collective: each process uploads its own rows, the link words
of a slab's edge rows need the other process's mask rows): both ranks share device 0 through the shared-memory
transport double, and the gathered result is bit for bit the masked reference of tests/mask_ref.py."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from grayscott_amd import capi

from . import mask_ref as R
from .helpers import assert_bits_equal, stress_fields
from tests.children import ROOT, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, rows, cols, steps, out_dir, transport_lib, boundary):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", GS_RCCL_LIBRARY=transport_lib)
    import torch.distributed as dist

    from grayscott_amd import HipArgs, Parameters, Simulation
    from grayscott_amd import dist as gsd
    from tests import mask_ref
    from tests.helpers import species_from_arrays, stress_fields

    info = gsd.bootstrap(backend="gloo", device="cpu")
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], rank=info.rank, world=info.world,
                                               unique_id=info.unique_id, boundary=boundary))
    r0, r1 = gsd.slab_range(rows, world, rank)
    u0, v0 = stress_fields((rows, cols), 32)
    mask = mask_ref.maze((rows, cols), np.random.default_rng(33))
    species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(rows, cols))
    sim.set_mask(mask)
    sim.perform_steps(species, steps)
    for _ in range(3):
        sim.perform_step(species)
    in_u, in_v, _, _ = species.in_out()
    u = gsd.gather_rows(in_u.make_scalar_view(sim.context), rank, world)
    v = gsd.gather_rows(in_v.make_scalar_view(sim.context), rank, world)
    if rank == 0:
        np.save(os.path.join(out_dir, "u.npy"), u)
        np.save(os.path.join(out_dir, "v.npy"), v)
        open(os.path.join(out_dir, "name"), "w").write(sim.context.info()[0])
    dist.barrier()
    sim.context.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("boundary", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_NEUMANN])
def test_two_processes_over_the_shm_transport(tmp_path, built, shm_transport, boundary):  # noqa: F811
    from tests.helpers import free_port

    rows, cols, steps = 301, 517, 14     # the seam at row 150 crosses a wall line (rows 0, 4, ..., 148, 152)
    spawn_ranks(_worker, (2, free_port(), rows, cols, steps, str(tmp_path), shm_transport, boundary), 2)
    u0, v0 = stress_fields((rows, cols), 32)
    mask = R.maze((rows, cols), np.random.default_rng(33))
    ref = R.run(u0, v0, steps + 3, mask, boundary=boundary)
    name = open(tmp_path / "name").read()
    assert name.split("@")[0].endswith("/neumann/mask" if boundary == capi.GS_BOUNDARY_NEUMANN else "/mask"), name
    assert_bits_equal(np.load(tmp_path / "u.npy"), ref[0], f"U 2 processes ({name})")
    assert_bits_equal(np.load(tmp_path / "v.npy"), ref[1], f"V 2 processes ({name})")
