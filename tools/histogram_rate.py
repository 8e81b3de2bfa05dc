"""Time of a histogram (gs_fields_histogram, gs_members_histogram) against a summary of the same planes, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and each of three distributions -- ``new`` (Species::new untouched:
one-valued), ``developed`` (uniform random planes after steps: a pattern) and ``random`` (uniform random values over every
bin) -- the histogram of U and V (256 bins unless ``--bins``) and their summary are timed alternately: device events
around the blocking call on the context's compute stream, ``--calls`` times each after a warm-up call, medians reported.
The yardstick is the summary -- the established cost of reading the two planes once with a wave per row --, so the table
gives the ratio histogram / summary per row and the ratio of the one-valued to the random input per grid.  The same for an
ensemble of 512 members of 64 x 128 (gs_members_histogram against gs_members_summarize).

    python tools/histogram_rate.py [--calls 9] [--bins 256] [--grids 16384x16384,4096x4096,1080x1920] [--no-ensemble] [--json FILE] [--md FILE]

GS_HIP_LIBRARY=<a variant built with tools/ab_build.py> times another build of the kernel (the two forms of count() that
profiles/histogram.md measured are retired: grayscott_amd/csrc/gs_experiments.h names the last commit that builds them).
Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402
from ratekit import ENSEMBLE, KINDS  # noqa: E402

HEADER = ["| grid | input | bins | histogram (ms) | summary (ms) | histogram / summary | plane reads (TB/s) | / random input |",
          "|---|---|---|---|---|---|---|---|"]


def time_species(rows, cols, kind, bins, calls):
    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        ratekit.fill(sim, species, kind)
        hu, hv = species.histogram(bins)
        m = ratekit.medians(ctx, {"histogram_ms": lambda: species.histogram(bins), "summary_ms": species.summary}, calls)
        return {"grid": f"{rows}x{cols}", "input": kind, "cells": rows * cols, "bins": bins, **m,
                "filled_bins_u": int(np.count_nonzero(hu.counts)), "filled_bins_v": int(np.count_nonzero(hv.counts)),
                "largest_share_u": float(hu.counts.max()) / (rows * cols)}


def time_ensemble(members, rows, cols, bins, calls):
    with ratekit.ensemble_subject(members, rows, cols) as (sim, ctx, ens):
        ens.perform_steps(16)
        m = ratekit.medians(ctx, {"histogram_ms": lambda: ens.histograms(bins=bins), "summary_ms": ens.summaries}, calls)
        return {"grid": f"{members} x {rows}x{cols}", "input": "new + 16 steps", "cells": members * rows * cols, "bins": bins, **m}


def main(argv=None) -> int:
    args = ratekit.observable_args(__doc__, argv, calls=9, add=lambda ap: ap.add_argument("--bins", type=int, default=256))
    report = ratekit.Report(args.json, args.md)
    for r, c in ratekit.parse_grids(args.grids):
        for kind in KINDS:
            report.row(time_species(r, c, kind, args.bins, args.calls))
    if not args.no_ensemble:
        report.row(time_ensemble(*ENSEMBLE, args.bins, args.calls))
    rows = report.rows
    random_ms = {r["grid"]: r["histogram_ms"] for r in rows if r["input"] == "random"}
    for r in rows:
        r["histogram_over_summary"] = r["histogram_ms"] / r["summary_ms"]
        r["read_tb_per_s"] = 8.0 * r["cells"] / (r["histogram_ms"] * 1e-3) / 1e12
        r["over_random"] = r["histogram_ms"] / random_ms[r["grid"]] if r["grid"] in random_ms else None
    report.table(*HEADER, *(
        f"| {r['grid']} | {r['input']} | {r['bins']} | {r['histogram_ms']:.3f} | {r['summary_ms']:.3f} | "
        f"{r['histogram_over_summary']:.2f} | {r['read_tb_per_s']:.2f} | "
        f"{'' if r['over_random'] is None else format(r['over_random'], '.2f')} |" for r in rows))
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
