"""Time of a summary (gs_fields_summarize, gs_members_summarize) against a single-step pass, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and for an ensemble of 512 members of 64 x 128: the state after a
few warm-up steps is summarized ``--calls`` times, each call timed twice -- device events around it on the context's
compute stream (the row kernel and the copy of its records: what the chip spends) and the host clock around the whole
blocking call (wait, launch, record copy, host fold) -- and a single-step pass (gs_step on the streaming kernel; one
gs_ensemble_run step for the ensemble) is timed with device events the same number of times.  Medians are reported,
with the plane-read rate of the summary (U and V: 8 bytes per cell) against its device time.

    python tools/summary_rate.py [--calls 20] [--grids 16384x16384,4096x4096,1080x1920] [--no-ensemble] [--json FILE] [--md profiles/summary.md]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402
from ratekit import ENSEMBLE  # noqa: E402

HEADER = ["| grid | summary, device (ms) | summary, host call (ms) | plane reads (TB/s) | single step (ms) | kernel of the step |"
          " summary / step |", "|---|---|---|---|---|---|---|"]


def _time(ctx, grid, cells, summary, step, calls):
    """The three figures one after another, ``calls`` calls each: the summary by device events, by the host clock, then a
    single-step pass between syncs."""
    summary()  # first launch: code object load

    def step_ms():
        ctx.sync()
        ms = ratekit.device_ms(ctx, step)
        ctx.sync()
        return ms

    step_ms()
    return {"grid": grid, "cells": cells,
            "summary_device_ms": statistics.median(ratekit.device_ms(ctx, summary) for _ in range(calls)),
            "summary_host_ms": statistics.median(ratekit.wall_ms(summary) for _ in range(calls)),
            "step_ms": statistics.median(step_ms() for _ in range(calls)), "step_kernel": ctx.info()[0]}


def time_species(rows, cols, calls):
    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        sim.perform_steps(species, 16)
        return _time(ctx, f"{rows}x{cols}", rows * cols, species.summary, lambda: sim.perform_step(species), calls)


def time_ensemble(members, rows, cols, calls):
    with ratekit.ensemble_subject(members, rows, cols) as (sim, ctx, ens):
        ens.perform_steps(16)
        return _time(ctx, f"{members} x {rows}x{cols}", members * rows * cols, ens.summaries, lambda: ens.prepare_steps(1), calls)


def main(argv=None) -> int:
    args = ratekit.observable_args(__doc__, argv, calls=20)
    report = ratekit.Report(args.json, args.md)
    rows = [time_species(r, c, args.calls) for r, c in ratekit.parse_grids(args.grids)]
    rows += [] if args.no_ensemble else [time_ensemble(*ENSEMBLE, args.calls)]
    for r in rows:
        r["read_tb_per_s"] = 8.0 * r["cells"] / (r["summary_device_ms"] * 1e-3) / 1e12
        r["summary_over_step"] = r["summary_device_ms"] / r["step_ms"]
        report.row(r)
    report.table(*HEADER, *(f"| {r['grid']} | {r['summary_device_ms']:.3f} | {r['summary_host_ms']:.3f} | {r['read_tb_per_s']:.2f} | "
                            f"{r['step_ms']:.3f} | {r['step_kernel']} | {r['summary_over_step']:.2f} |" for r in rows))
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
