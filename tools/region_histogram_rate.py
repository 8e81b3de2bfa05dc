"""Time of the regional histograms (gs_fields_region_histogram) against the whole-grid histogram, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920), every region shape (64x64, 256x256, 1024x1024), every bin count (64, 256, 4096)
and each of two inputs -- ``new`` (Species::new untouched) and ``random`` (uniform random values) -- the histograms of every
region of U and V are timed beside ``gs_fields_histogram`` of the same planes with the same bins, and beside the regions'
summaries (``gs_fields_region_summaries``): device events around the blocking call on the context's compute stream,
``--calls`` times each in turn after a warm-up call, medians reported.  The regional call is timed twice: as
``Species.region_histogram`` makes it, into a result array that is allocated anew in every call and taken apart into a
``RegionHistogram``, and as the library's call alone into a result that is allocated and touched once and then reused
(``reused``) -- host pages that are first touched under the device-to-host copy cost more than the launch.  The yardstick is the
whole-grid call beside it, so the table gives the ratios regional / whole-grid, of both forms.  A regional call whose result
is over GS_REGION_HIST_MAX counters per field is refused by the library: its cells hold ``-``.  The host route -- the download
of both planes plus numpy's counts of every crop of U and V -- is timed once per row (wall clock) on grids of at most
``--host-cells`` cells.

    python tools/region_histogram_rate.py [--calls 5] [--grids 16384x16384,4096x4096,1080x1920] [--regions 64x64,256x256,1024x1024]
                                          [--bins 64,256,4096] [--no-host] [--host-cells N] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402

KINDS = ("new", "random")
REGIONS = "64x64,256x256,1024x1024"
BINS = "64,256,4096"
RANGES = ((0.0, 1.0), (0.0, 1.0))
HEADER = ["| grid | region | bins | input | region histogram (ms) | reused (ms) | histogram (ms) | ratio | region summaries (ms) | host route (ms) |",
          "|---|---|---|---|---|---|---|---|---|---|"]


def library_call(ctx, species, region, bins):
    """The library's call alone on U and V, into a result that is allocated and touched here, once."""
    import ctypes

    import numpy as np

    from grayscott_amd import capi
    from grayscott_amd.simulation import _f32_pairs, _handle_array, region_grid

    in_u, in_v, _, _ = species.in_out()
    fields = [in_u, in_v]
    rows, cols = in_u.shape()
    lo, hi = _f32_pairs(RANGES)
    out = np.empty((2,) + region_grid(rows, cols, region) + (bins + 3,), np.uint64)
    out.fill(0)
    handles, to = _handle_array(fields), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    return lambda: capi.check(ctx._lib.gs_fields_region_histogram(ctx.handle, handles, 2, region[0], region[1], lo, hi, bins, to)), out


def host_route(ctx, species, region, bins):
    """Download of both planes and numpy's counts of every crop of U and V (numpy.histogram: f64 edges, not the library's
    rule -- the time is what is asked for here, not the bits)."""
    import numpy as np

    rh, rw = region
    in_u, in_v, _, _ = species.in_out()
    out = []
    for plane, rng in zip((in_u.make_scalar_view(ctx), in_v.make_scalar_view(ctx)), RANGES):
        rows, cols = plane.shape
        counts = np.zeros((-(-rows // rh), -(-cols // rw), bins), np.int64)
        for i in range(counts.shape[0]):
            for j in range(counts.shape[1]):
                counts[i, j] = np.histogram(plane[i * rh:(i + 1) * rh, j * rw:(j + 1) * rw], bins=bins, range=rng)[0]
        out.append(counts)
    return out


def time_species(rows, cols, regions, bin_counts, kind, calls, host):
    from grayscott_amd import capi

    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        ratekit.fill(sim, species, kind)
        for region in regions:
            for bins in bin_counts:
                fns = {"hist_ms": lambda: species.histogram(bins, *RANGES),
                       "region_summaries_ms": lambda: species.region_summaries(region)}
                try:  # (a result over the cap is refused before any device work)
                    species.region_histogram(region, bins, *RANGES)
                    fns["region_hist_ms"] = lambda: species.region_histogram(region, bins, *RANGES)
                    fns["region_hist_reused_ms"], _ = library_call(ctx, species, region, bins)
                except capi.GsError as e:
                    if e.code != capi.GS_ERR_INVALID:
                        raise
                m = ratekit.medians(ctx, fns, calls)
                rec = {"grid": f"{rows}x{cols}", "region": f"{region[0]}x{region[1]}", "bins": bins, "input": kind, "cells": rows * cols,
                       "region_hist_ms": None, "region_hist_reused_ms": None, **m}
                rec["host_ms"] = ratekit.wall_ms(lambda: host_route(ctx, species, region, bins)) if host else None
                yield rec


def main(argv=None) -> int:
    def add(ap):
        ap.add_argument("--regions", default=REGIONS, help="comma-separated RHxRW region shapes")
        ap.add_argument("--bins", default=BINS, help="comma-separated bin counts")
        ap.add_argument("--no-host", action="store_true", help="leave the host route out")
        ap.add_argument("--host-cells", type=int, default=1 << 24, help="the host route is timed on grids of at most this many cells")

    args = ratekit.observable_args(__doc__, argv, calls=5, add=add)
    report = ratekit.Report(args.json, args.md)
    regions, bin_counts = ratekit.parse_grids(args.regions), [int(x) for x in args.bins.split(",") if x]
    for r, c in ratekit.parse_grids(args.grids):
        for kind in KINDS:
            for rec in time_species(r, c, regions, bin_counts, kind, args.calls, not args.no_host and r * c <= args.host_cells):
                report.row(rec)

    def ms(x):
        return f"{x:.3f}" if x is not None else "-"

    for r in report.rows:
        for key in ("region_hist_ms", "region_hist_reused_ms"):
            r[key.replace("_ms", "_ratio")] = r[key] / r["hist_ms"] if r[key] is not None else None
    report.table(*HEADER, *(f"| {r['grid']} | {r['region']} | {r['bins']} | {r['input']} | {ms(r['region_hist_ms'])} | "
                            f"{ms(r['region_hist_reused_ms'])} | {r['hist_ms']:.3f} | "
                            + (f"{r['region_hist_ratio']:.2f} / {r['region_hist_reused_ratio']:.2f}" if r["region_hist_ratio"] is not None else "-")
                            + f" | {r['region_summaries_ms']:.3f} | " + (f"{r['host_ms']:.1f}" if r["host_ms"] is not None else "-") + " |"
                            for r in report.rows))
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
