"""What active sets cost and save (``gs_members_set_active``): ensembles with all, half and one eighth of their members active.

Three measurements, each a median of 5 timed with device events (``HipContext.timer_start`` / ``timer_stop``):

  active   for every row (members x grid), in 256-step calls in ONE process: all members active (the unlisted kernels), then
           every second and every eighth member active (the listed forms) -- time per call, time per active member-step,
           and both as ratios to the all-active run; then all reactivated (the unlisted kernels again), as a check that the
           first figure still stands.
  against  the all-active row of this tree and of another checkout (``--against ROOT``, e.g. the parent commit, built),
           in alternating fresh processes: the difference between the trees beside the run-to-run spread of either.
  mirror   what a run pays for members retired since the last one: 256 of 512 members of 64 x 128 retired, the first 2-step
           call after the retirement (it uploads the list and launches gs_members_mirror_k) against the same call with
           nothing to mirror, and a device-to-device copy of the same bytes (``Ensemble.copy_from`` of 256 members:
           two hipMemcpyAsync).

    python tools/ensemble_active_rate.py [--rows 512x64x128,64x256x512] [--against ROOT] [--json out.jsonl]

Every measurement runs in a child process of its own under ``timeout``; the tool stops at the first one that fails.
Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [(512, 64, 128), (64, 256, 512)]
STEPS, CALLS = 256, 5
CHILD_TIMEOUT = 240  # seconds per child: a measurement takes a few


def timed_calls(ctx, ens, steps, calls=CALLS):
    ens.perform_steps(steps)  # warm-up (and, after a retirement, the mirror launch)
    times = []
    for _ in range(calls):
        ctx.timer_start()
        ens.prepare_steps(steps)
        times.append(ctx.timer_stop())
    ctx.sync()
    return times


def child_active(members, rows, cols, all_only=False):
    import numpy as np

    from ensemble_rate import member_params
    from grayscott_amd import HipArgs, Simulation

    params = member_params(members)
    sim = Simulation.new(params[0], HipArgs(devices=[0]))
    ctx = sim.context
    ens = sim.make_ensemble((rows, cols), params)
    out = {"members": members, "rows": rows, "cols": cols, "steps_per_call": STEPS, "runs": []}
    for label, every in (("all", 1),) if all_only else (("all", 1), ("half", 2), ("eighth", 8), ("all again", 1)):
        if not all_only:
            mask = np.zeros(members, np.bool_)
            mask[::every] = True
            ens.set_active(mask)
        active = members if all_only else ens.active_count()
        times = timed_calls(ctx, ens, STEPS)
        ms = statistics.median(times)
        out["runs"].append({"label": label, "active": active, "kernel": ctx.info()[0], "ms": ms, "ms_all": times,
                            "ns_per_active_member_step": ms * 1e6 / (active * STEPS)})
    ens.destroy()
    ctx.close()
    return out


def child_mirror():
    import numpy as np

    from ensemble_rate import member_params
    from grayscott_amd import HipArgs, Simulation

    members, rows, cols = 512, 64, 128
    sim = Simulation.new(member_params(members)[0], HipArgs(devices=[0]))
    ctx = sim.context
    ens = sim.make_ensemble((rows, cols), member_params(members))
    snap = ens.snapshot()
    mask = np.ones(members, np.bool_)
    mask[1::2] = False
    ens.set_active(mask)
    ens.perform_steps(2)  # warm-up of the listed kernels and of the mirror kernel
    with_mirror, without, copies = [], [], []
    for _ in range(CALLS):
        ens.set_active(np.ones(members, np.bool_))
        ens.set_active(mask)  # retired again: 256 members to mirror
        ctx.timer_start()
        ens.prepare_steps(2)
        with_mirror.append(ctx.timer_stop())
        ctx.timer_start()
        ens.prepare_steps(2)
        without.append(ctx.timer_stop())
        ctx.timer_start()
        snap.copy_from(ens, 0, 256)
        copies.append(ctx.timer_stop())
    out = {"members": members, "rows": rows, "cols": cols, "mirrored": 256, "bytes": 256 * rows * cols * 4 * 2, "kernel": ctx.info()[0],
           "ms_with_mirror": statistics.median(with_mirror), "ms_without": statistics.median(without),
           "ms_copy_same_bytes": statistics.median(copies), "ms_with_mirror_all": with_mirror, "ms_without_all": without,
           "ms_copy_all": copies}
    out["ms_mirror"] = out["ms_with_mirror"] - out["ms_without"]
    ens.destroy()
    snap.destroy()
    ctx.close()
    return out


def run_child(root, argv):
    """One measurement in a fresh process on the tree at ``root`` under its own time limit -> its JSON record."""
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child"] + argv
    env = dict(os.environ, GS_ACTIVE_RATE_ROOT=root)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=root)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"{' '.join(argv)} on {root}: exit status {r.returncode}; stopping")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", default=None, help="comma-separated MEMBERSxROWSxCOLS (default: 512x64x128,64x256x512)")
    ap.add_argument("--against", default=None, metavar="ROOT", help="another built checkout to time the all-active rows on")
    ap.add_argument("--pairs", type=int, default=3, help="process pairs per row of the comparison with --against")
    ap.add_argument("--no-mirror", action="store_true", help="skip the mirror measurement")
    ap.add_argument("--json", default=None, help="append one JSON line per measurement to this file")
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.child:
        root = os.environ.get("GS_ACTIVE_RATE_ROOT", ROOT)
        sys.path[:0] = [root, os.path.join(root, "tools")]
        kind = args.child[0]
        if kind == "mirror":
            res = child_mirror()
        else:
            res = child_active(*(int(x) for x in args.child[1:4]), all_only=kind == "all")
        print(json.dumps(res))
        return 0
    rows = ROWS if not args.rows else [tuple(int(x) for x in r.split("x")) for r in args.rows.split(",")]

    def keep(res):
        if args.json:
            with open(args.json, "a") as f:
                f.write(json.dumps(res) + "\n")
        return res

    print("| members x grid | active | kernel | ms per call | vs all | ns per active member-step | vs all |")
    print("|---|---|---|---|---|---|---|")
    for m, r, c in rows:
        res = keep(run_child(ROOT, ["active", str(m), str(r), str(c)]))
        base = res["runs"][0]
        for x in res["runs"]:
            print(f"| {m} x {r}x{c} | {x['label']}: {x['active']} | {x['kernel']} | {x['ms']:.3f} | {x['ms'] / base['ms']:.3f} | "
                  f"{x['ns_per_active_member_step']:.2f} | {x['ns_per_active_member_step'] / base['ns_per_active_member_step']:.3f} |",
                  flush=True)
    if args.against:
        print("\n| members x grid | tree | ms per call, all active (median of 5 per process) | median | spread |")
        print("|---|---|---|---|---|")
        for m, r, c in rows:
            got = {"this": [], "other": []}
            for _ in range(args.pairs):
                for name, root in (("this", ROOT), ("other", os.path.abspath(args.against))):
                    res = keep(dict(run_child(root, ["all", str(m), str(r), str(c)]), tree=name))
                    got[name].append(res["runs"][0]["ms"])
            for name in ("this", "other"):
                v = got[name]
                print(f"| {m} x {r}x{c} | {name} | {', '.join(f'{x:.3f}' for x in v)} | {statistics.median(v):.3f} | "
                      f"{(max(v) - min(v)) / statistics.median(v) * 100:.2f} % |", flush=True)
            d = statistics.median(got["this"]) / statistics.median(got["other"]) - 1
            print(f"| {m} x {r}x{c} | this / other - 1 | | {d * 100:+.2f} % | |", flush=True)
    if not args.no_mirror:
        res = keep(run_child(ROOT, ["mirror"]))
        print(f"\nmirror: {res['mirrored']} members of {res['rows']}x{res['cols']} ({res['bytes'] / 2**20:.0f} MiB): the 2-step call after the "
              f"retirement {res['ms_with_mirror']:.3f} ms, the same call with nothing to mirror {res['ms_without']:.3f} ms -> "
              f"{res['ms_mirror']:.3f} ms for the list upload and the mirror launch; a device-to-device copy of the same bytes "
              f"{res['ms_copy_same_bytes']:.3f} ms ({res['kernel']})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
