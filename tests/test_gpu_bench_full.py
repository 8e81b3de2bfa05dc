"""bench.py's plain run against its --full run on one GPU: the plain line carries the headline and none of the legs that
--full adds, the --full line carries them and its replay says "equal", and both runs dump the same planes (the timed
steps and their inputs do not depend on --full)."""
import json
import os
import sys

import numpy as np
import pytest

from tests.children import ROOT, run_program

pytestmark = pytest.mark.gpu

FULL_ONLY = ("verified", "single_step", "developed_pattern", "value_developed_pattern", "cpu_baseline",
             "energy_pJ_per_cell_step", "ranks", "peer_chain")


def _bench(args, timeout=600):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GS_RCCL_LIBRARY"):
        e.pop(k, None)
    r = run_program([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=e, limit=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_has_the_headline_only_and_dumps_what_full_dumps(built, tmp_path):
    common = ["--gpus", "1", "--steps", "8", "--warmup", "4", "--repeats", "3", "--grid", "4096x2048", "--no-cpu-baseline"]
    plain = _bench(common + ["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(common + ["--full", "--dump-outputs", str(tmp_path / "full")])

    for line in (plain, full):
        assert line["value"] > 0 and line["steps"] == 8 and line["warmup"] == 4 and line["repeats"] == 3
        assert abs(line["ms_per_step"] - 4096 * 2048 / (line["value"] * 1e6) * 1e3) < 1e-6 * line["ms_per_step"]
        assert line["roofline"]["launches"] > 0 and line["config"]["grid"] == [4096, 2048]
    assert not [k for k in FULL_ONLY if k in plain], plain.keys()
    assert set(plain["stage_seconds"]) == {"import", "init", "setup", "timed", "dump", "developed"}, plain["stage_seconds"]

    assert full["verified"]["equal"] is True and full["verified"]["developed_pattern"]["equal"] is True, full["verified"]
    assert full["single_step"]["kernel"].startswith("stream") and full["developed_pattern"]["repeats"] == 3
    assert "cpu_baseline" not in full            # (--no-cpu-baseline)

    # the same steps on the same inputs: the same files, the same bits
    dp, df = plain["dump_outputs"], full["dump_outputs"]
    assert dp["tuning_steps"] == df["tuning_steps"], (dp, df)
    assert dp["steps"] == df["steps"] and dp["developed_steps"] == df["developed_steps"], (dp, df)
    assert sorted(dp["files"]) == sorted(df["files"]) == sorted(["u.npy", "v.npy", "index.npy", "developed_u.npy",
                                                                  "developed_v.npy"])
    for name in dp["files"]:
        a, b = np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
