"""TimeStats of the C++ mirror (include/grayscott_hip.hpp) over the C ABI.

CPU: the program compiles with plain g++ against gs_hip.h, links libgs_hip.so and fails loudly without a GPU.  GPU: its
planes -- a Species' and an ensemble's -- equal the Python binding's bit for bit."""
import os

import numpy as np
import pytest

from tests.children import build_program, run_program

BEFORE, EVERY, SAMPLES = 24, 8, 5


@pytest.fixture(scope="module")
def exe(built, tmp_path_factory):
    out = build_program("time_stats_mirror", tmp_path_factory.mktemp("cpp"))
    return str(out)


def test_cpp_time_stats_mirror_builds_and_fails_loudly_without_gpu(exe, tmp_path):
    assert os.access(exe, os.X_OK)
    if not os.path.exists("/dev/kfd"):
        r = run_program([exe, "8", "16", "2", "2", "2", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(24, 30), (64, 300)])
def test_cpp_time_stats_match_the_python_binding(exe, tmp_path, rows, cols):
    from grayscott_amd import HipArgs, Parameters, Simulation

    out = tmp_path / "o.bin"
    r = run_program([exe, str(rows), str(cols), str(BEFORE), str(EVERY), str(SAMPLES), str(out)])
    assert r.returncode == 0, r.stderr
    data = open(out, "rb").read()
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    want = []

    def sampled(source, stats, steps):
        steps(BEFORE)
        for k in range(SAMPLES):
            if k:
                steps(EVERY)
            stats.accumulate(BEFORE + k * EVERY)

    species = sim.make_species((rows, cols))
    stats = species.time_stats(("sum", "squares", "extremes", "crossings"), v_threshold=0.25, u_threshold=0.5, above=(False, True))
    sampled(species, stats, lambda n: sim.perform_steps(species, n))
    for name in ("mean", "variance", "min", "max", "occupancy", "arrival"):
        want.append(getattr(stats, name)("v").make_scalar_view(ctx))
    want.append(stats.mean("u").make_scalar_view(ctx))
    want += [stats.raw("sum", "v"), stats.raw("first_stamp", "v"), np.array([stats.samples], np.uint64)]
    assert stats.samples == SAMPLES and want[1].max() > 0 and (want[5] >= 0).any()
    stats.close()
    params = [Parameters(feed_rate=float(np.float32(0.014) + np.float32(0.004) * np.float32(i))) for i in range(3)]
    ens = sim.make_ensemble((rows, cols), params)
    stats = ens.time_stats(("sum", "squares", "extremes", "crossings"), v_threshold=0.25, u_threshold=0.5, above=(False, True))
    sampled(ens, stats, ens.perform_steps)
    want += [stats.mean("v"), stats.variance("v"), stats.max("v"), stats.arrival("v"), stats.occupancy("u")]
    assert want[-5].shape == (3, rows, cols) and not np.array_equal(want[-5][0], want[-5][2])
    stats.close()
    ctx.close()
    blob = b"".join(np.ascontiguousarray(a).tobytes() for a in want)
    assert len(data) == len(blob)
    at = 0
    for i, a in enumerate(want):
        assert data[at:at + a.nbytes] == np.ascontiguousarray(a).tobytes(), f"block {i} differs"
        at += a.nbytes
