"""Time of a correlation call (gs_fields_correlation, gs_members_correlation) against a summary and a morphology call on the
same planes, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and each of three inputs -- ``new`` (Species::new untouched),
``developed`` (uniform random planes after steps: a pattern) and ``random`` (uniform random values: half the cells set) --
the pair counts of U and V with one threshold each at L = 16, 32 and 64, with four thresholds at L = 32, their summary and
their morphology with one threshold are timed in turn: device events around the blocking call on the context's compute
stream, ``--calls`` times each after a warm-up call, medians reported.  The yardsticks are the summary and the morphology
call, so the table gives the ratios to both.  The same for an ensemble of 512 members of 64 x 128.

    python tools/correlation_rate.py [--calls 9] [--grids 16384x16384,4096x4096,1080x1920] [--no-ensemble] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402
from ratekit import ENSEMBLE, KINDS  # noqa: E402

TV, TU = (0.25, 0.1, 0.05, 0.4), (0.5, 0.8, 0.3, 0.95)
HEADER = ["| grid | input | L = 16 (ms) | L = 32 (ms) | L = 64 (ms) | nt = 4, L = 32 (ms) | summary (ms) | morphology (ms) | "
          "L = 32 / summary | L = 32 / morphology | L = 64 / morphology | plane reads, L = 32 (TB/s) |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]


def time_species(rows, cols, kind, calls):
    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        ratekit.fill(sim, species, kind)
        fns = {"l16_ms": lambda: species.correlation(TV[:1], TU[:1], max_lag=16),
               "l32_ms": lambda: species.correlation(TV[:1], TU[:1], max_lag=32),
               "l64_ms": lambda: species.correlation(TV[:1], TU[:1], max_lag=64),
               "nt4_l32_ms": lambda: species.correlation(TV, TU, max_lag=32),
               "summary_ms": species.summary, "morphology_ms": lambda: species.morphology(TV[:1], TU[:1])}
        out = {"grid": f"{rows}x{cols}", "input": kind, "cells": rows * cols, **ratekit.medians(ctx, fns, calls)}
        _, cv = species.correlation(TV[:1], TU[:1], max_lag=32)
        out["v_fraction"] = cv[0].fraction
        out["v_first_minimum_rows"] = cv[0].first_minimum(0)
        return out


def time_ensemble(members, rows, cols, calls):
    with ratekit.ensemble_subject(members, rows, cols) as (sim, ctx, ens):
        ens.perform_steps(16)
        one = {"v_thresholds": TV[:1], "u_thresholds": TU[:1]}
        fns = {"l16_ms": lambda: ens.correlations(max_lag=16, **one), "l32_ms": lambda: ens.correlations(max_lag=32, **one),
               "l64_ms": lambda: ens.correlations(max_lag=64, **one),
               "nt4_l32_ms": lambda: ens.correlations(v_thresholds=TV, u_thresholds=TU, max_lag=32),
               "summary_ms": ens.summaries, "morphology_ms": lambda: ens.morphologies(**one)}
        return {"grid": f"{members} x {rows}x{cols}", "input": "new + 16 steps", "cells": members * rows * cols,
                **ratekit.medians(ctx, fns, calls)}


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
        r["l32_over_summary"] = r["l32_ms"] / r["summary_ms"]
        r["l32_over_morphology"] = r["l32_ms"] / r["morphology_ms"]
        r["l64_over_morphology"] = r["l64_ms"] / r["morphology_ms"]
        r["l32_read_tb_per_s"] = 8.0 * r["cells"] / (r["l32_ms"] * 1e-3) / 1e12
    report.table(*HEADER, *(
        f"| {r['grid']} | {r['input']} | {r['l16_ms']:.3f} | {r['l32_ms']:.3f} | {r['l64_ms']:.3f} | "
        f"{r['nt4_l32_ms']:.3f} | {r['summary_ms']:.3f} | {r['morphology_ms']:.3f} | {r['l32_over_summary']:.2f} | "
        f"{r['l32_over_morphology']:.2f} | {r['l64_over_morphology']:.2f} | {r['l32_read_tb_per_s']:.2f} |" for r in rows))
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
