"""Time of the regional state comparison (gs_fields_region_compare) against the whole-grid comparison, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and every region shape (64x64, 256x256, 1024x1024) the change of every
region of U and V against a snapshot taken four steps earlier (random planes) is timed: the library's call alone into a result
that is allocated and touched once and then reused, with each route forced (GS_HIP_REGION_CHANGE_ROUTE = ``records``, ``wave``)
and with the library's own choice, and the Python call ``Species.region_changes_since``, which allocates its result anew and
takes it apart into ``RegionChange`` objects.  Beside them, on the same planes: ``gs_fields_compare`` of the same two pairs --
the yardstick: it reads the same bytes -- and ``gs_fields_region_summaries`` of two planes, the regional twin whose kernel
gives a wave a whole region.  Device events around the blocking call on the context's compute stream, ``--calls`` times each
in turn after a warm-up call, medians reported; the table gives the ratios of the library's choice to both baselines.  The
host route -- the download of V and of the snapshot's V plus the restatement of the rule (tests/change_ref.py) on every crop --
is timed once per row (wall clock) on grids of at most ``--host-cells`` cells.

    python tools/region_change_rate.py [--calls 5] [--grids 16384x16384,4096x4096,1080x1920] [--regions 64x64,256x256,1024x1024]
                                       [--no-host] [--host-cells N] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ratekit  # noqa: E402

REGIONS = "64x64,256x256,1024x1024"
ROUTES = (("records", "change_records_ms"), ("wave", "change_wave_ms"), ("", "change_ms"))  # "": the library's choice
VARIABLE = "GS_HIP_REGION_CHANGE_ROUTE"
HEADER = ["| grid | region | records (ms) | wave (ms) | choice (ms) | Python call (ms) | compare (ms) | choice / compare | "
          "region summaries (ms) | choice / summaries | host route (ms) |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]


def library_call(ctx, species, snap, region):
    """The library's call alone on (U, V) against the snapshot, into a result that is allocated and touched here, once:
    ``call(route)`` makes it with the route switch set to ``route``."""
    import ctypes

    import numpy as np

    from grayscott_amd import capi
    from grayscott_amd.simulation import CHANGE_DTYPE, _handle_array, region_grid

    in_u, in_v, _, _ = species.in_out()
    rows, cols = in_u.shape()
    out = np.empty((2,) + region_grid(rows, cols, region), CHANGE_DTYPE)
    out.fill(0)
    a, b, to = _handle_array([in_u, in_v]), _handle_array([snap.u, snap.v]), out.ctypes.data_as(ctypes.POINTER(capi.GsChange))

    def call(route):
        os.environ[VARIABLE] = route
        capi.check(ctx._lib.gs_fields_region_compare(ctx.handle, a, b, 2, region[0], region[1], to))

    return call, out


def host_route(ctx, species, snap, region):
    """Two downloads -- V and the snapshot's V -- and the rule's restatement on every crop."""
    sys.path.insert(0, os.path.dirname(HERE))
    try:
        from tests import change_ref
    finally:
        sys.path.pop(0)
    rh, rw = region
    now, then = species.in_out()[1].make_scalar_view(ctx), snap.v.make_scalar_view(ctx)
    rows, cols = now.shape
    return [[change_ref.change(now[i:i + rh, j:j + rw], then[i:i + rh, j:j + rw]) for j in range(0, cols, rw)]
            for i in range(0, rows, rh)]


def time_species(rows, cols, regions, calls, host):
    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        ratekit.fill(sim, species, "random")
        snap = species.snapshot()
        try:
            sim.perform_steps(species, 4)
            ctx.sync()
            for region in regions:
                call, out = library_call(ctx, species, snap, region)
                fns = {key: (lambda route=route: call(route)) for route, key in ROUTES}
                os.environ[VARIABLE] = ""
                fns["python_ms"] = lambda: (os.environ.__setitem__(VARIABLE, ""), species.region_changes_since(snap, region))
                fns["compare_ms"] = lambda: species.change_since(snap)
                fns["region_summaries_ms"] = lambda: species.region_summaries(region)
                m = ratekit.medians(ctx, fns, calls)
                whole = species.change_since(snap)
                rec = {"grid": f"{rows}x{cols}", "region": f"{region[0]}x{region[1]}", "cells": rows * cols,
                       "regions": int(out[0].size), **m}
                # what was timed is the comparison: the regions' counts add up to the whole grid's
                rec["checked"] = bool(int(out["differing"][1].sum()) == whole[1].differing and whole[1].differing > 0)
                rec["host_ms"] = ratekit.wall_ms(lambda: host_route(ctx, species, snap, region)) if host else None
                yield rec
        finally:
            os.environ.pop(VARIABLE, None)
            snap.close()


def main(argv=None) -> int:
    def add(ap):
        ap.add_argument("--regions", default=REGIONS, help="comma-separated RHxRW region shapes")
        ap.add_argument("--no-host", action="store_true", help="leave the host route out")
        ap.add_argument("--host-cells", type=int, default=1 << 24, help="the host route is timed on grids of at most this many cells")

    args = ratekit.observable_args(__doc__, argv, calls=5, add=add)
    report = ratekit.Report(args.json, args.md)
    regions = ratekit.parse_grids(args.regions)
    for r, c in ratekit.parse_grids(args.grids):
        for rec in time_species(r, c, regions, args.calls, not args.no_host and r * c <= args.host_cells):
            report.row(rec)
    for r in report.rows:
        r["compare_ratio"] = r["change_ms"] / r["compare_ms"]
        r["summaries_ratio"] = r["change_ms"] / r["region_summaries_ms"]
    report.table(*HEADER, *(f"| {r['grid']} | {r['region']} | {r['change_records_ms']:.3f} | {r['change_wave_ms']:.3f} | "
                            f"{r['change_ms']:.3f} | {r['python_ms']:.3f} | {r['compare_ms']:.3f} | {r['compare_ratio']:.2f} | "
                            f"{r['region_summaries_ms']:.3f} | {r['summaries_ratio']:.2f} | "
                            + (f"{r['host_ms']:.1f}" if r["host_ms"] is not None else "-") + " |" for r in report.rows))
    report.finish()
    return 0 if all(r["checked"] for r in report.rows) else 1


if __name__ == "__main__":
    sys.exit(main())
