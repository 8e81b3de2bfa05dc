"""Time of a summary (gs_fields_summarize, gs_members_summarize) against a single-step pass, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and for an ensemble of 512 members of 64 x 128: the state after a
few warm-up steps is summarized ``--calls`` times, each call timed twice -- device events around it on the context's
compute stream (the row kernel and the copy of its records: what the chip spends) and the host clock around the whole
blocking call (wait, launch, record copy, host fold) -- and a single-step pass (gs_step on the streaming kernel; one
gs_ensemble_run step for the ensemble) is timed with device events the same number of times.  Medians are reported,
with the plane-read rate of the summary (U and V: 8 bytes per cell) against its device time.

    python tools/summary_rate.py [--calls 20] [--json FILE] [--md profiles/summary.md]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(16384, 16384), (4096, 4096), (1080, 1920)]
ENSEMBLE = (512, 64, 128)  # members, rows, cols


def _median_ms(fn, calls):
    return statistics.median(fn() for _ in range(calls))


def time_species(rows, cols, calls):
    from grayscott_amd import HipArgs, Parameters, Simulation

    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    species = sim.make_species((rows, cols))
    sim.perform_steps(species, 16)
    species.summary()  # first launch: code object load

    def device_summary():
        ctx.timer_start()
        species.summary()
        return ctx.timer_stop()

    def host_summary():
        t0 = time.perf_counter()
        species.summary()
        return (time.perf_counter() - t0) * 1e3

    def step():
        ctx.sync()
        ctx.timer_start()
        sim.perform_step(species)
        ms = ctx.timer_stop()
        ctx.sync()
        return ms

    step()
    out = {"grid": f"{rows}x{cols}", "cells": rows * cols, "summary_device_ms": _median_ms(device_summary, calls),
           "summary_host_ms": _median_ms(host_summary, calls), "step_ms": _median_ms(step, calls),
           "step_kernel": ctx.info()[0]}
    ctx.close()
    return out


def time_ensemble(members, rows, cols, calls):
    from grayscott_amd import HipArgs, Parameters, Simulation

    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    ens = sim.make_ensemble((rows, cols), Parameters(), members=members)
    ens.perform_steps(16)
    ens.summaries()

    def device_summary():
        ctx.timer_start()
        ens.summaries()
        return ctx.timer_stop()

    def host_summary():
        t0 = time.perf_counter()
        ens.summaries()
        return (time.perf_counter() - t0) * 1e3

    def step():
        ctx.sync()
        ctx.timer_start()
        ens.prepare_steps(1)
        ms = ctx.timer_stop()
        ctx.sync()
        return ms

    step()
    out = {"grid": f"{members} x {rows}x{cols}", "cells": members * rows * cols,
           "summary_device_ms": _median_ms(device_summary, calls), "summary_host_ms": _median_ms(host_summary, calls),
           "step_ms": _median_ms(step, calls), "step_kernel": ctx.info()[0]}
    ens.destroy()
    ctx.close()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--json", default=None, help="also write the rows as a JSON list")
    ap.add_argument("--md", default=None, help="also write the table as markdown")
    args = ap.parse_args(argv)
    import torch  # noqa: F401  (the process's HIP runtime is torch's, as in bench.py and the tests)

    rows = [time_species(r, c, args.calls) for r, c in GRIDS] + [time_ensemble(*ENSEMBLE, args.calls)]
    for r in rows:
        r["read_tb_per_s"] = 8.0 * r["cells"] / (r["summary_device_ms"] * 1e-3) / 1e12
        r["summary_over_step"] = r["summary_device_ms"] / r["step_ms"]
        print(json.dumps(r))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    lines = ["| grid | summary, device (ms) | summary, host call (ms) | plane reads (TB/s) | single step (ms) | kernel of the step |"
             " summary / step |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['grid']} | {r['summary_device_ms']:.3f} | {r['summary_host_ms']:.3f} | {r['read_tb_per_s']:.2f} | "
                     f"{r['step_ms']:.3f} | {r['step_kernel']} | {r['summary_over_step']:.2f} |")
    print("\n".join(lines))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
