"""bench.py --dump-outputs end to end: the files are the planes of the timed Species (and of the developed pattern) after
the step counts the line reports -- the right slot, U before V, the sample's cells where the index says -- checked against
an independent replay with the single-step kernel (itself pinned to the CPU oracle in test_gpu_parity.py).  The replay
stands in for the oracle because bench.py's untimed warm-up alone is ~6e10 cell-steps on any grid below 2^24 cells."""
import json
import os
import sys

import numpy as np
import pytest

from tests.children import ROOT, run_program

pytestmark = pytest.mark.gpu


def _bench(args, timeout=600):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GS_RCCL_LIBRARY"):
        e.pop(k, None)
    r = run_program([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=e, limit=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def _replayed(sim, u0, v0, shape, steps):
    """(U, V) after `steps` single-step launches from Species::new (u0 None) or from (u0, v0)."""
    from benchkit.legs import upload_species

    sp = sim.make_species(list(shape), place_candidates=0) if u0 is None else upload_species(sim, u0, v0, 0)
    sim.perform_steps(sp, steps)
    in_u, in_v, _, _ = sp.in_out()
    out = in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)
    for c in sp.u._pair + sp.v._pair:
        c.destroy()
    return out


def test_dump_outputs_are_the_timed_planes(built, tmp_path):
    import bench
    from benchkit.legs import developed_start
    from grayscott_amd import HipArgs, Parameters, Simulation, capi

    out = str(tmp_path / "dump")
    common = ["--gpus", "1", "--steps", "8", "--warmup", "4", "--repeats", "1", "--no-verify", "--no-cpu-baseline",
              "--dump-outputs", out]
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], kernel=capi.GS_KERNEL_STREAM))
    try:
        # 4096 x 2048 with the developed pattern: four planes above 64 MB -> a sample of cells; then 1024 x 2048 without
        # it into the same directory -> two whole planes, and nothing of the first dump left beside them
        for grid, extra in (("4096x2048", []), ("1024x2048", ["--no-extra"])):
            line = _bench(["--grid", grid] + extra + common)
            rows, cols = line["config"]["grid"]
            d = line["dump_outputs"]
            sampled = grid == "4096x2048"
            want = ["u.npy", "v.npy"] + (["index.npy", "developed_u.npy", "developed_v.npy"] if sampled else [])
            assert sorted(d["files"]) == sorted(want) and sorted(os.listdir(out)) == sorted(want), (d, os.listdir(out))
            assert d["steps"] == line["untimed_steps_before_first_region"] + line["steps"] * line["repeats"], d
            assert sum(os.path.getsize(os.path.join(out, f)) for f in want) <= 64 * 10 ** 6
            idx = None
            if sampled:
                idx = np.load(os.path.join(out, "index.npy"))
                assert idx.dtype == np.float64 and d["sampled_cells"] == idx.size
                idx = idx.astype(np.int64)
                assert idx.tobytes() == bench.dump_index(rows, cols, 4).tobytes()      # the fixed, seeded sample
            else:
                assert d["sampled_cells"] is None

            cases = [("", None, None, d["steps"])]
            if sampled:
                u0, v0 = developed_start(rows, cols)
                cases.append(("developed_", u0, v0, d["developed_steps"]))
            for prefix, u0, v0, steps in cases:
                ref_u, ref_v = _replayed(sim, u0, v0, (rows, cols), steps)
                if idx is not None:
                    ref_u, ref_v = ref_u.reshape(-1)[idx], ref_v.reshape(-1)[idx]
                got_u, got_v = np.load(os.path.join(out, prefix + "u.npy")), np.load(os.path.join(out, prefix + "v.npy"))
                assert got_u.dtype == got_v.dtype == np.float32 and got_u.shape == got_v.shape == ref_u.shape
                assert got_u.tobytes() == ref_u.tobytes(), (grid, prefix + "u")
                assert got_v.tobytes() == ref_v.tobytes(), (grid, prefix + "v")
    finally:
        sim.context.close()
