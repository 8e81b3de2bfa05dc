"""Time of the regional observables (gs_fields_region_summaries, gs_fields_region_morphology) against their whole-grid twins, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920), every region shape (64x64, 256x256, 1024x1024) and each of two inputs --
``new`` (Species::new untouched) and ``random`` (uniform random values) -- the summaries of every region of U and V are timed
beside ``gs_fields_summarize`` of the same planes, and the regions' bit-quad counts with one threshold (nt = 1) and with four
(nt = 4) beside ``gs_fields_morphology``: device events around the blocking call on the context's compute stream, ``--calls``
times each in turn after a warm-up call, medians reported.  The yardstick is the whole-grid call beside it -- both read each
plane once --, so the table gives the ratios regional / whole-grid.  The host route -- the download of both planes plus the numpy
restatement of the region means, variances, extremes and set-cell counts -- is timed once per row (wall clock).

    python tools/regions_rate.py [--calls 9] [--grids 16384x16384,4096x4096,1080x1920] [--regions 64x64,256x256,1024x1024]
                                 [--no-host] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402

KINDS = ("new", "random")
REGIONS = "64x64,256x256,1024x1024"
TV, TU = (0.25, 0.1, 0.05, 0.4), (0.5, 0.8, 0.3, 0.95)
HEADER = ["| grid | region | input | region summaries (ms) | summary (ms) | ratio | region quads nt = 1 (ms) | quads nt = 1 (ms) | ratio "
          "| region quads nt = 4 (ms) | quads nt = 4 (ms) | ratio | host route (ms) |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]


def host_route(ctx, species, region):
    """Download of both planes and the numpy restatement: per region mean, variance, min, max, non-finite and set-cell counts."""
    import numpy as np

    rh, rw = region
    in_u, in_v, _, _ = species.in_out()
    out = []
    for plane, t, above in ((in_u.make_scalar_view(ctx), TU[0], False), (in_v.make_scalar_view(ctx), TV[0], True)):
        rows, cols = plane.shape
        re, ce = np.arange(0, rows, rh), np.arange(0, cols, rw)
        a = plane.astype(np.float64)

        def blocks(x, op):
            return op.reduceat(op.reduceat(x, re, axis=0), ce, axis=1)

        cells = np.minimum(rh, rows - re)[:, None] * np.minimum(rw, cols - ce)[None, :]
        mean = blocks(a, np.add) / cells
        out.append((mean, blocks(a * a, np.add) / cells - mean * mean, blocks(plane, np.minimum), blocks(plane, np.maximum),
                    blocks((~np.isfinite(plane)).astype(np.int64), np.add),
                    blocks(((plane > t) if above else (plane < t)).astype(np.int64), np.add)))
    return out


def time_species(rows, cols, regions, kind, calls, host):
    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        ratekit.fill(sim, species, kind)
        for region in regions:
            m = ratekit.medians(ctx, {"region_summary_ms": lambda: species.region_summaries(region),
                                      "summary_ms": species.summary,
                                      "region_quads1_ms": lambda: species.region_morphology(region, TV[:1], TU[:1]),
                                      "quads1_ms": lambda: species.morphology(TV[:1], TU[:1]),
                                      "region_quads4_ms": lambda: species.region_morphology(region, TV, TU),
                                      "quads4_ms": lambda: species.morphology(TV, TU)}, calls)
            rec = {"grid": f"{rows}x{cols}", "region": f"{region[0]}x{region[1]}", "input": kind, "cells": rows * cols, **m}
            rec["host_ms"] = ratekit.wall_ms(lambda: host_route(ctx, species, region)) if host else None
            yield rec


def main(argv=None) -> int:
    def add(ap):
        ap.add_argument("--regions", default=REGIONS, help="comma-separated RHxRW region shapes")
        ap.add_argument("--no-host", action="store_true", help="leave the host route out")

    args = ratekit.observable_args(__doc__, argv, calls=9, add=add)
    report = ratekit.Report(args.json, args.md)
    regions = ratekit.parse_grids(args.regions)
    for r, c in ratekit.parse_grids(args.grids):
        for kind in KINDS:
            for rec in time_species(r, c, regions, kind, args.calls, not args.no_host):
                report.row(rec)
    for r in report.rows:
        r["summary_ratio"] = r["region_summary_ms"] / r["summary_ms"]
        r["quads1_ratio"] = r["region_quads1_ms"] / r["quads1_ms"]
        r["quads4_ratio"] = r["region_quads4_ms"] / r["quads4_ms"]
    report.table(*HEADER, *(f"| {r['grid']} | {r['region']} | {r['input']} | {r['region_summary_ms']:.3f} | {r['summary_ms']:.3f} | "
                            f"{r['summary_ratio']:.2f} | {r['region_quads1_ms']:.3f} | {r['quads1_ms']:.3f} | {r['quads1_ratio']:.2f} | "
                            f"{r['region_quads4_ms']:.3f} | {r['quads4_ms']:.3f} | {r['quads4_ratio']:.2f} | "
                            + (f"{r['host_ms']:.1f}" if r["host_ms"] is not None else "-") + " |" for r in report.rows))
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
