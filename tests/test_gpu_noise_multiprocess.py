"""The noise term over two processes (gs_ctx_set_noise is collective; every process passes the same struct): each rank
draws at its slab's GLOBAL rows, ghost rows at the neighbour's, so every word equals the single-slab restatement of
tests/noise_ref.py.  Two ranks over the shm transport through the child-process kit of tests/children.py."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from grayscott_amd import capi

from . import noise_ref as N
from .helpers import assert_bits_equal
from tests.children import ROOT, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
NOISE = dict(sigma_u=0.02, sigma_v=0.01, seed=0xFEEDFACE12345678, step=2 ** 32 - 3)  # the step index crosses 2^32 in the run


def _worker(rank, world, port, rows, cols, steps, out_dir, transport_lib, boundary):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", GS_RCCL_LIBRARY=transport_lib)
    import torch.distributed as dist

    from grayscott_amd import HipArgs, Parameters, Simulation
    from grayscott_amd import dist as gsd
    from tests.helpers import species_from_arrays, stress_fields
    from tests.test_gpu_noise_multiprocess import NOISE

    info = gsd.bootstrap(backend="gloo", device="cpu")
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], rank=info.rank, world=info.world,
                                               unique_id=info.unique_id, boundary=boundary))
    r0, r1 = gsd.slab_range(rows, world, rank)
    u0, v0 = stress_fields((rows, cols), 22)
    species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(rows, cols))
    sim.set_noise(**NOISE)
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
        open(os.path.join(out_dir, "step"), "w").write(str(sim.noise()["step"]))
    dist.barrier()
    sim.context.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("boundary", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_NEUMANN])
def test_two_processes_over_the_shm_transport(tmp_path, built, shm_transport, boundary):  # noqa: F811
    from tests.helpers import free_port, stress_fields

    rows, cols, steps = 300, 517, 14
    spawn_ranks(_worker, (2, free_port(), rows, cols, steps, str(tmp_path), shm_transport, boundary), 2)
    u0, v0 = stress_fields((rows, cols), 22)
    ref = N.run(u0, v0, steps + 3, NOISE, rule=boundary)
    name = open(tmp_path / "name").read()
    assert name.split("@")[0].endswith("/noise"), name
    assert int(open(tmp_path / "step").read()) == NOISE["step"] + steps + 3
    assert_bits_equal(np.load(tmp_path / "u.npy"), ref[0], f"U of 2 processes ({name})")
    assert_bits_equal(np.load(tmp_path / "v.npy"), ref[1], f"V of 2 processes ({name})")
