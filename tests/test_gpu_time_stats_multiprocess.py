"""Time statistics in a multi-process context: no rank exchanges anything, every process keeps the accumulators of its own
rows, and they are bit for bit the single-process ones.  Both ranks share device 0 through the shared-memory transport double
(tests/cpp/shm_transport.cpp, built as tests/test_gpu_multiprocess.py builds it); the rows do not divide evenly."""
import os

import numpy as np
import pytest

from tests.children import rank_session, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
ROWS, COLS = 64, 300
BEFORE, EVERY, SAMPLES = 11, 7, 4
RAW = ("sum", "squares", "min", "max", "set_count", "first_stamp")
RESULTS = ("mean", "variance", "min", "max", "occupancy", "arrival")


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
    from tests.helpers import species_from_arrays, stress_fields

    with rank_session(rank, world, port, transport_lib, ROWS) as (sim, (r0, r1)):
        u0, v0 = stress_fields((ROWS, COLS), 4)
        species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(ROWS, COLS))
        out = _scenario(sim, species)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), rows=np.array([r0, r1]), **out)


def test_every_rank_keeps_the_single_process_bits_of_its_rows(tmp_path, built, shm_transport):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from tests import time_stats_ref as ref
    from tests.helpers import free_port, species_from_arrays, stress_fields

    world = 2
    spawn_ranks(_worker, (world, free_port(), str(tmp_path), shm_transport), world)
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
