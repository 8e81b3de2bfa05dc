"""Rates of ensembles against the same members run one after another (``gs_ensemble_run`` vs ``gs_run``).

For every row (members x grid), in 256-step calls:
  * the aggregate rate of the ensemble: the sum over members of cells x steps / s, from device events around each call
    (median of 5 calls, after one warm-up call);
  * the rate of the same members run one after another through gs_run in the same process: a sample of up to
    ``--sample`` members (the ones at evenly spaced indices), each a Species with its own parameters, timed back to back
    in one window per call (median of 5, warmed up) -- the sequential rate does not depend on how many members follow;
  * the speed-up, the kernel gs_ctx_info names, and a bit-check: a sampled member of the ensemble against its lone run
    after the same calls.

    python tools/ensemble_rate.py [--rows 4096x8x16,64x256x512] [--json out.jsonl] [--no-sequential]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = [(4096, 8, 16), (512, 64, 128), (256, 128, 256), (64, 256, 512), (16, 512, 1024), (4, 1024, 2048)]
STEPS, CALLS = 256, 5


def member_params(n):
    """A (feed, kill) sweep around the defaults; every member keeps the default stencil and dt (the .op kernels)."""
    from grayscott_amd import Parameters

    side = max(1, int(round(n ** 0.5)))
    return [Parameters(feed_rate=0.010 + 0.030 * (i % side) / side, kill_rate=0.045 + 0.020 * (i // side) / max(1, (n + side - 1) // side))
            for i in range(n)]


def measure(members, rows, cols, sample, sequential=True):
    import numpy as np

    from grayscott_amd import HipArgs, Simulation

    params = member_params(members)
    sim = Simulation.new(params[0], HipArgs(devices=[0]))
    ctx = sim.context
    ens = sim.make_ensemble((rows, cols), params)
    ens.perform_steps(STEPS)  # warm-up
    times = []
    for _ in range(CALLS):
        ctx.timer_start()
        ens.prepare_steps(STEPS)
        times.append(ctx.timer_stop())
    ctx.sync()
    kernel = ctx.info()[0]
    cells = rows * cols
    out = {"members": members, "rows": rows, "cols": cols, "steps_per_call": STEPS, "kernel": kernel,
           "ensemble_ms": statistics.median(times), "ensemble_ms_all": times}
    out["ensemble_rate"] = members * cells * STEPS / (out["ensemble_ms"] * 1e3)  # Mcells x steps / s
    if sequential:
        idx = sorted({int(round(i * (members - 1) / max(1, min(sample, members) - 1))) for i in range(min(sample, members))})
        solo = [sim.make_species((rows, cols)) for _ in idx]
        seq_times, solo_kernel = [], None
        for call in range(CALLS + 1):  # the first call of every member is its warm-up
            ctx.timer_start()
            for j, i in enumerate(idx):
                ctx.set_params(params[i])
                sim.prepare_steps(solo[j], STEPS)
            ms = ctx.timer_stop()
            if call:
                seq_times.append(ms)
            solo_kernel = ctx.info()[0]
        ctx.sync()
        out["sequential_members_timed"] = len(idx)
        out["sequential_kernel"] = solo_kernel
        out["sequential_ms_per_member"] = statistics.median(seq_times) / len(idx)
        out["sequential_rate"] = cells * STEPS / (out["sequential_ms_per_member"] * 1e3)
        out["speedup"] = out["ensemble_rate"] / out["sequential_rate"]
        # bit-check: the middle sampled member, after the same 1 + CALLS calls on both sides
        j = len(idx) // 2
        got = ens.result_views(idx[j], 1)[0]
        ref = solo[j].make_result_view()
        out["bitcheck_member"] = idx[j]
        out["bitcheck"] = bool(got.tobytes() == ref.tobytes())
        out["bitcheck_max_abs_diff"] = float(np.max(np.abs(got.astype(np.float64) - ref)))
        for s in solo:
            for c in s.in_out():
                c.destroy()
    ens.destroy()
    ctx.close()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", default=None, help="comma-separated MEMBERSxROWSxCOLS (default: the six rows of the table)")
    ap.add_argument("--sample", type=int, default=32, help="members timed one after another for the sequential rate")
    ap.add_argument("--no-sequential", action="store_true", help="time the ensembles only (profiling runs)")
    ap.add_argument("--json", default=None, help="append one JSON line per row to this file")
    args = ap.parse_args(argv)
    rows = ROWS if not args.rows else [tuple(int(x) for x in r.split("x")) for r in args.rows.split(",")]
    print("| members x grid | kernel | ensemble Mcells*steps/s | sequential Mcells*steps/s | speed-up | bit-check |")
    print("|---|---|---|---|---|---|")
    ok = True
    for members, r, c in rows:
        res = measure(members, r, c, args.sample, not args.no_sequential)
        if args.json:
            with open(args.json, "a") as f:
                f.write(json.dumps(res) + "\n")
        if args.no_sequential:
            print(f"| {members} x {r}x{c} | {res['kernel']} | {res['ensemble_rate']:.0f} | - | - | - |", flush=True)
            continue
        ok = ok and res["bitcheck"]
        print(f"| {members} x {r}x{c} | {res['kernel']} | {res['ensemble_rate']:.0f} | {res['sequential_rate']:.0f} "
              f"({res['sequential_kernel']}) | {res['speedup']:.1f}x | member {res['bitcheck_member']}: "
              f"{'identical' if res['bitcheck'] else 'DIFFERS'} |", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
