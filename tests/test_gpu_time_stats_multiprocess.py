"""Time statistics in a multi-process context: no rank exchanges anything, every process keeps the accumulators of its own
rows, and they are bit for bit the single-process ones.  Both ranks share device 0 through the shared-memory transport double
(tests/cpp/shm_transport.cpp, built as tests/test_gpu_multiprocess.py builds it); the rows do not divide evenly.  The ranks run
under a watchdog."""
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, COLS = 64, 300
BEFORE, EVERY, SAMPLES = 11, 7, 4
WATCHDOG_S = 120.0       # the ranks need a few seconds; one that hangs in the transport double must not hang the suite
RAW = ("sum", "squares", "min", "max", "set_count", "first_stamp")
RESULTS = ("mean", "variance", "min", "max", "occupancy", "arrival")


@pytest.fixture(scope="module")
def shm_transport(built):
    from tests.helpers import build_shm_transport

    return build_shm_transport()


def _scenario(sim, species):
    """Four samples of a stepping Species; {name: this process's rows} of every raw accumulator and result plane of U and V."""
    ctx = sim.context
    stats = species.time_stats(("sum", "squares", "extremes", "crossings"), v_threshold=0.25, u_threshold=0.5, above=(False, True))
    sim.perform_steps(species, BEFORE)
    for k in range(SAMPLES):
        if k:
            sim.perform_steps(species, EVERY)
        stats.accumulate(BEFORE + k * EVERY)
    out = {"samples": np.array([stats.samples])}
    for sp in ("u", "v"):
        for name in RAW:
            out[f"raw_{name}_{sp}"] = stats.raw(name, sp)
        for name in RESULTS:
            plane = getattr(stats, name)(sp)
            out[f"{name}_{sp}"] = plane.make_scalar_view(ctx)
            plane.destroy()
    stats.close()
    return out


def _worker(rank, world, port, out_dir, transport_lib):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from grayscott_amd import Parameters, Simulation
    from tests.helpers import join_ranks, species_from_arrays, stress_fields

    args, (r0, r1) = join_ranks(rank, world, port, transport_lib, ROWS, 1)
    sim = Simulation.new(Parameters(), args)
    u0, v0 = stress_fields((ROWS, COLS), 4)
    species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(ROWS, COLS))
    out = _scenario(sim, species)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), rows=np.array([r0, r1]), **out)
    dist.barrier()
    sim.context.close()
    dist.destroy_process_group()


def _spawn_bounded(fn, args, world):
    """``mp.spawn`` with a watchdog: the ranks are joined until WATCHDOG_S have passed; then whatever still runs is killed and
    the test fails.  (A rank that fails makes ``join`` raise, as with ``join=True``.)"""
    import time

    ctx = mp.spawn(fn, args=args, nprocs=world, join=False)
    deadline = time.monotonic() + WATCHDOG_S
    try:
        while not ctx.join(timeout=1.0):
            if time.monotonic() > deadline:
                raise AssertionError(f"the ranks did not finish within {WATCHDOG_S:.0f} s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
        for p in ctx.processes:
            p.join(5.0)


def test_every_rank_keeps_the_single_process_bits_of_its_rows(tmp_path, built, shm_transport):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from tests import time_stats_ref as ref
    from tests.helpers import free_port, species_from_arrays, stress_fields

    world = 2
    _spawn_bounded(_worker, (world, free_port(), str(tmp_path), shm_transport), world)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = stress_fields((ROWS, COLS), 4)
    want = _scenario(sim, species_from_arrays(sim, u0, v0))
    sim.context.close()
    assert int(want["samples"][0]) == SAMPLES and want["variance_v"].max() > 0
    covered = 0
    for rank in range(world):
        z = np.load(tmp_path / f"rank{rank}.npz")
        r0, r1 = z["rows"]
        assert int(z["samples"][0]) == SAMPLES
        for name, a in want.items():
            if name != "samples":
                assert z[name].shape == (r1 - r0, COLS), (rank, name, z[name].shape)
                assert ref.same_bits(z[name], a[r0:r1]), (rank, name, ref.describe(z[name], a[r0:r1]))
        covered += r1 - r0
    assert covered == ROWS
