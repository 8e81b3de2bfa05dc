"""The drivers' time statistics on the GPU: ``simulate --hip-time-stats-every`` and ``sweep --time-stats-every`` write the planes
the restatement (tests/time_stats_ref.py) forms from the same states, and leave the images they write as they are."""
import numpy as np
import pytest

from tests import time_stats_ref as ref

pytestmark = pytest.mark.gpu


def restated(states, steps, threshold):
    """{key: plane} as the drivers name them, from [(u, v)] sampled at ``steps``."""
    accs = {"u": ref.Accumulators(states[0][0].shape, ref.ALL, None), "v": ref.Accumulators(states[0][1].shape, ref.ALL, threshold, True)}
    for (u, v), step in zip(states, steps):
        accs["u"].accumulate(u, step)
        accs["v"].accumulate(v, step)
    out = {}
    for sp in ("u", "v"):
        for key, name in (("mean", "mean"), ("var", "variance"), ("min", "min"), ("max", "max")):
            out[f"{key}_{sp}"] = accs[sp].result(name)
    out["occupancy_v"], out["arrival_v"] = accs["v"].result("occupancy"), accs["v"].result("arrival")
    return out


def test_simulate_writes_the_restated_planes(built, tmp_path):
    from grayscott_amd import simulate
    from tests.helpers import gpu_run
    import oracle

    base = ["-n", "3", "-e", "8", "-r", "64", "-c", "300"]
    plain, with_stats = str(tmp_path / "plain.npy"), str(tmp_path / "stats.npy")
    simulate.run(simulate.parse(base + ["-o", plain]))
    simulate.run(simulate.parse(base + ["-o", with_stats, "--hip-time-stats-every", "4", "--hip-time-stats-from", "6",
                                        "--hip-time-stats-threshold-v", "0.25"]))
    assert np.load(plain).tobytes() == np.load(with_stats).tobytes()
    steps = list(range(6, 25, 4))
    u0, v0 = oracle.init_species(64, 300)
    states = [gpu_run(u0, v0, s)[:2] for s in steps]
    want = restated(states, steps, 0.25)
    with np.load(simulate.time_stats_path(with_stats)) as z:
        assert int(z["samples"]) == len(steps) and list(z["steps"]) == steps and list(z["rows"]) == [0, 64]
        for key, plane in want.items():
            assert ref.same_bits(z[key], plane), (key, ref.describe(z[key], plane))
        assert z["var_v"].max() > 0 and (z["arrival_v"] >= 0).any()


def test_both_drivers_sample_the_initial_state_from_step_0(built, tmp_path):
    """``--*-from 0``: step 0 is a sample like any other, in both drivers."""
    from grayscott_amd import simulate, sweep
    from tests.helpers import gpu_run
    import oracle

    out = str(tmp_path / "zero.npy")
    simulate.run(simulate.parse(["-n", "2", "-e", "5", "-r", "64", "-c", "300", "-o", out, "--hip-time-stats-every", "4",
                                 "--hip-time-stats-from", "0", "--hip-time-stats-threshold-v", "0.25"]))
    steps = [0, 4, 8]
    u0, v0 = oracle.init_species(64, 300)
    want = restated([(u0, v0)] + [gpu_run(u0, v0, s)[:2] for s in steps[1:]], steps, 0.25)
    with np.load(simulate.time_stats_path(out)) as z:
        assert list(z["steps"]) == steps and z["steps"][0] == 0 and int(z["samples"]) == 3
        for key, plane in want.items():
            assert ref.same_bits(z[key], plane), (key, ref.describe(z[key], plane))
        # the seed is V = 1 > 0.25: where it lies the front "arrived" at step 0
        assert np.array_equal(z["arrival_v"] == 0, v0 > np.float32(0.25)) and (z["arrival_v"] == 0).any()
    out = str(tmp_path / "zero.h5")
    sweep.run(sweep.parse(["--feed", "0.014:0.03:2", "--kill", "0.054:0.054:1", "-r", "24", "-c", "30", "-s", "9", "-o", out,
                           "--time-stats-every", "4", "--time-stats-from", "0", "--time-stats-threshold-v", "0.25"]))
    with np.load(sweep.time_stats_path(out)) as z:
        assert list(z["steps"]) == steps and int(z["samples"]) == 3 and (z["arrival_v"] == 0).any()
        assert np.array_equal(z["max_u"][:, 0, 0], np.ones(2, np.float32))      # U = 1 outside the seed at step 0


def test_sweep_writes_the_restated_planes_and_scalars(built, tmp_path):
    from grayscott_amd import HipArgs, Parameters, Simulation, sweep

    argv = ["--feed", "0.014:0.03:2", "--kill", "0.054:0.054:1", "-r", "24", "-c", "30", "-s", "22", "--time-stats-every", "5",
            "--time-stats-threshold-v", "0.25"]
    out = str(tmp_path / "run.h5")
    args = sweep.parse(argv + ["-o", out])
    sweep.run(args)
    steps = [5, 10, 15, 20]
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ens = sim.make_ensemble((24, 30), sweep.member_params(args))
    states, done = [], 0
    for s in steps:
        ens.perform_steps(s - done)
        done = s
        states.append((ens.u_views(), ens.result_views()))
    ens.perform_steps(22 - done)
    final = ens.result_views()
    ens.destroy()
    sim.context.close()
    want = restated(states, steps, 0.25)
    with np.load(sweep.time_stats_path(out)) as z:
        assert int(z["samples"]) == 4 and list(z["steps"]) == steps
        for key, plane in want.items():
            assert ref.same_bits(z[key], plane), (key, ref.describe(z[key], plane))
        assert np.array_equal(z["var_v_mean"], want["var_v"].mean(axis=(1, 2), dtype=np.float64))
        assert np.array_equal(z["var_v_max"], want["var_v"].max(axis=(1, 2)).astype(np.float64)) and z["var_v_max"].min() > 0
        assert np.array_equal(z["mean_v_mean"], want["mean_v"].mean(axis=(1, 2), dtype=np.float64))
    # the run went on to its last step, and --no-fields leaves the planes out
    from grayscott_amd import hdf5_min

    assert np.asarray(hdf5_min.read(out)).tobytes() == final.tobytes()
    out2 = str(tmp_path / "lean.h5")
    sweep.run(sweep.parse(argv + ["-o", out2, "--no-fields"]))
    with np.load(sweep.time_stats_path(out2)) as z:
        assert "var_v" not in z.files and np.array_equal(z["var_v_max"], want["var_v"].max(axis=(1, 2)).astype(np.float64))
