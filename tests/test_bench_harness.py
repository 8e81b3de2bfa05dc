"""bench.py's harness around the timed regions, without a GPU: the per-rank watchdog (a stage that exceeds its
bound prints one JSON line and the process exits non-zero), the fault hook the GPU tests use to force such a
stall, and the launcher path of `python bench.py --gpus N` (a torchrun CHILD, started before this process touches
a GPU; never an exec)."""
import json
import os
import sys

from tests.children import ROOT, run_program


def _python(code, env=None, timeout=120):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return run_program([sys.executable, "-c", code], cwd=ROOT, env=e, limit=timeout)


def test_watchdog_ends_a_stage_that_exceeds_its_bound():
    r = _python("import time, bench\nwd = bench.Watchdog(rank=3)\n"
                "with wd.stage('quick', 30):\n    pass\n"
                "with wd.stage('comm-init', 0.5):\n    time.sleep(30)\nprint('not reached')\n")
    assert r.returncode == 3, (r.returncode, r.stdout, r.stderr)
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["rank"] == 3 and line["stage"] == "comm-init" and "error" in line and line["bound_s"] == 0.5
    assert "not reached" not in r.stdout


def test_watchdog_leaves_a_stage_that_ends_in_time_alone():
    r = _python("import time, bench\nwd = bench.Watchdog(rank=0)\n"
                "with wd.stage('a', 1.0):\n    time.sleep(0.2)\ntime.sleep(1.5)\nprint('done')\n")
    assert r.returncode == 0 and r.stdout.strip() == "done", (r.returncode, r.stdout, r.stderr)


def test_fault_hook_stalls_the_named_rank_and_stage_only():
    code = ("import bench\nwd = bench.Watchdog(rank=1)\n"
            "with wd.stage('init', 2):\n    pass\nprint('init passed', flush=True)\n"
            "with wd.stage('timed', 2):\n    pass\nprint('timed passed')\n")
    r = _python(code, env={"GS_BENCH_FAULT": "stall:1:timed", "GS_BENCH_WATCHDOG_S": "1"})
    assert r.returncode == 3 and "init passed" in r.stdout and "timed passed" not in r.stdout
    assert json.loads(r.stdout.strip().splitlines()[-1])["stage"] == "timed"
    r = _python(code, env={"GS_BENCH_FAULT": "stall:0:timed", "GS_BENCH_WATCHDOG_S": "1"})
    assert r.returncode == 0 and "timed passed" in r.stdout


def test_gpus_n_without_torchrun_starts_a_torchrun_child():
    """No GPU here: every child rank reaches bench.py's own "no GPU visible" exit, which proves that the parent
    started torch.distributed.run with N ranks and relayed its failure as a non-zero exit code."""
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    r = run_program([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "0"],
                    cwd=ROOT, env=e, limit=600)
    assert r.returncode != 0
    assert r.stderr.count("no GPU visible") >= 2, r.stderr[-2000:]


def test_dump_outputs_sample_is_fixed_and_within_budget():
    """--dump-outputs: whole planes while they fit 64 MB, else the same seeded sample of cells for every run of a grid."""
    import bench

    assert bench.dump_index(1080, 1920, 4) is None and bench.dump_index(2000, 2000, 4) is not None
    a, b = bench.dump_index(16384, 16384, 4), bench.dump_index(16384, 16384, 4)
    assert a.tobytes() == b.tobytes() and a.size > (1 << 20)
    assert (a[1:] > a[:-1]).all() and a[0] >= 0 and a[-1] < 16384 * 16384
    assert 4 * a.size * 4 + a.size * 8 <= bench.DUMP_MAX_BYTES <= 64 * 10 ** 6


def test_dump_outputs_is_refused_for_several_gpus():
    r = _python("import sys, bench\nsys.argv = ['bench.py', '--gpus', '2', '--dump-outputs', 'out']\nsys.exit(bench.main())\n")
    assert r.returncode == 2 and "--dump-outputs" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(os.path.join(ROOT, "out"))


def test_full_is_off_by_default():
    """A plain run times the headline only; every other leg waits for --full."""
    r = _python("import sys, bench\nsys.argv = ['bench.py', '--gpus', '1', '--steps', '4', '--warmup', '0']\n"
                "print(bench.parse_args().full)\nsys.argv.append('--full')\nprint(bench.parse_args().full)\n")
    assert r.returncode == 0 and r.stdout.split() == ["False", "True"], (r.returncode, r.stdout, r.stderr)
