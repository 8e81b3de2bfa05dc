"""Time of a morphology call (gs_fields_morphology, gs_members_morphology) against a summary of the same planes, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and each of three inputs -- ``new`` (Species::new untouched),
``developed`` (uniform random planes after steps: a pattern) and ``random`` (uniform random values: half the cells set) --
the bit-quad counts of U and V with one threshold each (nt = 1) and with four (nt = 4) and their summary are timed in turn:
device events around the blocking call on the context's compute stream, ``--calls`` times each after a warm-up call, medians
reported.  The yardstick is the summary -- the established cost of reading the two planes once with a wave per row --, so the
table gives the ratios morphology / summary.  The same for an ensemble of 512 members of 64 x 128 (gs_members_morphology
against gs_members_summarize).

    python tools/morphology_rate.py [--calls 9] [--grids 16384x16384,4096x4096,1080x1920] [--no-ensemble] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402
from ratekit import ENSEMBLE, KINDS  # noqa: E402

TV, TU = (0.25, 0.1, 0.05, 0.4), (0.5, 0.8, 0.3, 0.95)
HEADER = ["| grid | input | nt = 1 (ms) | nt = 4 (ms) | summary (ms) | nt = 1 / summary | nt = 4 / summary | plane reads, nt = 1 (TB/s) |",
          "|---|---|---|---|---|---|---|---|"]


def time_species(rows, cols, kind, calls):
    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        ratekit.fill(sim, species, kind)
        _, mv = species.morphology(TV[:1], TU[:1])
        m = ratekit.medians(ctx, {"nt1_ms": lambda: species.morphology(TV[:1], TU[:1]), "nt4_ms": lambda: species.morphology(TV, TU),
                                  "summary_ms": species.summary}, calls)
        return {"grid": f"{rows}x{cols}", "input": kind, "cells": rows * cols, **m,
                "v_area_fraction": mv[0].area_fraction, "v_euler8": mv[0].euler8}


def time_ensemble(members, rows, cols, calls):
    with ratekit.ensemble_subject(members, rows, cols) as (sim, ctx, ens):
        ens.perform_steps(16)
        m = ratekit.medians(ctx, {"nt1_ms": lambda: ens.morphologies(v_thresholds=TV[:1], u_thresholds=TU[:1]),
                                  "nt4_ms": lambda: ens.morphologies(v_thresholds=TV, u_thresholds=TU),
                                  "summary_ms": ens.summaries}, calls)
        return {"grid": f"{members} x {rows}x{cols}", "input": "new + 16 steps", "cells": members * rows * cols, **m}


def main(argv=None) -> int:
    args = ratekit.observable_args(__doc__, argv, calls=9)
    report = ratekit.Report(args.json, args.md)
    for r, c in ratekit.parse_grids(args.grids):
        for kind in KINDS:
            report.row(time_species(r, c, kind, args.calls))
    if not args.no_ensemble:
        report.row(time_ensemble(*ENSEMBLE, args.calls))
    rows = report.rows
    for r in rows:
        r["nt1_over_summary"] = r["nt1_ms"] / r["summary_ms"]
        r["nt4_over_summary"] = r["nt4_ms"] / r["summary_ms"]
        r["nt1_read_tb_per_s"] = 8.0 * r["cells"] / (r["nt1_ms"] * 1e-3) / 1e12
    report.table(*HEADER, *(f"| {r['grid']} | {r['input']} | {r['nt1_ms']:.3f} | {r['nt4_ms']:.3f} | {r['summary_ms']:.3f} | "
                            f"{r['nt1_over_summary']:.2f} | {r['nt4_over_summary']:.2f} | {r['nt1_read_tb_per_s']:.2f} |" for r in rows))
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
