"""Time of the regional two-point correlations (gs_fields_region_correlation) against the whole-grid call, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920), every region shape (256x256, 1024x1024, 64x64), every largest lag
(16, 32, 64) and each of two inputs -- ``new`` (Species::new untouched) and ``random`` (uniform random values) -- the pair
counts of every region of U and V with one threshold (nt = 1) and with four (nt = 4) are timed beside ``gs_fields_correlation``
of the same planes, lags and thresholds, and beside the regions' bit-quad counts (``gs_fields_region_morphology``, nt = 1):
device events around the blocking call on the context's compute stream, ``--calls`` times each in turn after a warm-up call,
medians reported.  The regional call is timed twice: as ``Species.region_correlation`` makes it, into a result array that
is allocated anew in every call, and as the library's call alone into a result that is allocated and touched once and then
reused (``reused``) -- host pages that are first touched under the device-to-host copy cost more than the launch.  The
yardstick is the whole-grid call beside it, so the table gives the ratios regional / whole-grid, of both forms.  A regional call whose result is over GS_REGION_PAIRS_MAX counters per field is refused by the library: its cells hold ``-``.
The host route -- the download of both planes plus the numpy pair counts of every crop of V at one threshold -- is timed once
per row (wall clock) on grids of at most ``--host-cells`` cells.

    python tools/region_correlation_rate.py [--calls 5] [--grids 16384x16384,4096x4096,1080x1920]
                                            [--regions 256x256,1024x1024,64x64] [--lags 16,32,64] [--no-host]
                                            [--host-cells N] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402

KINDS = ("new", "random")
REGIONS = "256x256,1024x1024,64x64"
LAGS = "16,32,64"
TV, TU = (0.25, 0.1, 0.05, 0.4), (0.5, 0.8, 0.3, 0.95)
STEPS = ((0, 1), (1, 0), (1, 1), (1, -1))
HEADER = ["| grid | region | L | input | region pairs nt = 1 (ms) | reused (ms) | pairs nt = 1 (ms) | ratio | region pairs nt = 4 (ms) | reused (ms) "
          "| pairs nt = 4 (ms) | ratio | region quads nt = 1 (ms) | host route (ms) |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]


def library_call(ctx, species, region, nt, max_lag):
    """The library's call alone on U and V, into a result that is allocated and touched here, once."""
    import ctypes

    import numpy as np

    from grayscott_amd import capi
    from grayscott_amd.simulation import _field_thresholds, _handle_array, region_grid

    in_u, in_v, _, _ = species.in_out()
    fields = [in_u, in_v]
    n, nt, thr, sense = _field_thresholds(fields, [TU[:nt], TV[:nt]], [False, True])
    rows, cols = in_u.shape()
    out = np.empty((n,) + region_grid(rows, cols, region) + (nt, 4, max_lag + 1), np.uint64)
    out.fill(0)
    handles, to = _handle_array(fields), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    return lambda: capi.check(ctx._lib.gs_fields_region_correlation(ctx.handle, handles, n, region[0], region[1], thr, sense, nt,
                                                                    max_lag, to)), out


def host_route(ctx, species, region, max_lag):
    """Download of both planes and the numpy pair counts of every crop of V set above TV[0]."""
    import numpy as np

    rh, rw = region
    in_u, in_v, _, _ = species.in_out()
    in_u.make_scalar_view(ctx)
    b = in_v.make_scalar_view(ctx) > np.float32(TV[0])
    rows, cols = b.shape
    out = np.zeros((-(-rows // rh), -(-cols // rw), 4, max_lag + 1), np.uint64)
    for i in range(out.shape[0]):
        for j in range(out.shape[1]):
            crop = b[i * rh:(i + 1) * rh, j * rw:(j + 1) * rw]
            h, w = crop.shape
            for k, (dr, dc) in enumerate(STEPS):
                for d in range(max_lag + 1):
                    if d * dr >= h or d * abs(dc) >= w:
                        break
                    upper, lower = crop[:h - d * dr], crop[d * dr:]
                    if dc > 0:
                        upper, lower = upper[:, :w - d], lower[:, d:]
                    elif dc < 0:
                        upper, lower = upper[:, d:], lower[:, :w - d]
                    out[i, j, k, d] = np.count_nonzero(upper & lower)
    return out


def time_species(rows, cols, regions, lags, kind, calls, host):
    from grayscott_amd import capi

    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        ratekit.fill(sim, species, kind)
        for region in regions:
            for L in lags:
                fns = {"pairs1_ms": lambda: species.correlation(TV[:1], TU[:1], L),
                       "pairs4_ms": lambda: species.correlation(TV, TU, L),
                       "region_quads1_ms": lambda: species.region_morphology(region, TV[:1], TU[:1])}
                for name, nt in (("region_pairs1_ms", 1), ("region_pairs4_ms", 4)):
                    try:  # (a result over the cap is refused before any device work)
                        species.region_correlation(region, TV[:nt], TU[:nt], L)
                        fns[name] = lambda nt=nt: species.region_correlation(region, TV[:nt], TU[:nt], L)
                        fns[name.replace("_ms", "_reused_ms")], _ = library_call(ctx, species, region, nt, L)
                    except capi.GsError as e:
                        if e.code != capi.GS_ERR_INVALID:
                            raise
                m = ratekit.medians(ctx, fns, calls)
                rec = {"grid": f"{rows}x{cols}", "region": f"{region[0]}x{region[1]}", "lags": L, "input": kind, "cells": rows * cols,
                       "region_pairs1_ms": None, "region_pairs4_ms": None, "region_pairs1_reused_ms": None,
                       "region_pairs4_reused_ms": None, **m}
                rec["host_ms"] = ratekit.wall_ms(lambda: host_route(ctx, species, region, L)) if host else None
                yield rec


def main(argv=None) -> int:
    def add(ap):
        ap.add_argument("--regions", default=REGIONS, help="comma-separated RHxRW region shapes")
        ap.add_argument("--lags", default=LAGS, help="comma-separated largest lags")
        ap.add_argument("--no-host", action="store_true", help="leave the host route out")
        ap.add_argument("--host-cells", type=int, default=1 << 22, help="the host route is timed on grids of at most this many cells")

    args = ratekit.observable_args(__doc__, argv, calls=5, add=add)
    report = ratekit.Report(args.json, args.md)
    regions, lags = ratekit.parse_grids(args.regions), [int(x) for x in args.lags.split(",") if x]
    for r, c in ratekit.parse_grids(args.grids):
        for kind in KINDS:
            for rec in time_species(r, c, regions, lags, kind, args.calls, not args.no_host and r * c <= args.host_cells):
                report.row(rec)

    def ms(x):
        return f"{x:.3f}" if x is not None else "-"

    def ratios(r, nt):  # of the call as Python makes it / of the library's call alone
        a, b = r[f"pairs{nt}_ratio"], r[f"pairs{nt}_reused_ratio"]
        return f"{a:.2f} / {b:.2f}" if a is not None else "-"

    for r in report.rows:
        for nt in (1, 4):
            got = r[f"region_pairs{nt}_ms"]
            r[f"pairs{nt}_ratio"] = got / r[f"pairs{nt}_ms"] if got is not None else None
            reused = r[f"region_pairs{nt}_reused_ms"]
            r[f"pairs{nt}_reused_ratio"] = reused / r[f"pairs{nt}_ms"] if reused is not None else None
    report.table(*HEADER, *(f"| {r['grid']} | {r['region']} | {r['lags']} | {r['input']} | {ms(r['region_pairs1_ms'])} | {ms(r['region_pairs1_reused_ms'])} | "
                            f"{r['pairs1_ms']:.3f} | " + ratios(r, 1)
                            + f" | {ms(r['region_pairs4_ms'])} | {ms(r['region_pairs4_reused_ms'])} | {r['pairs4_ms']:.3f} | " + ratios(r, 4)
                            + f" | {r['region_quads1_ms']:.3f} | " + (f"{r['host_ms']:.1f}" if r["host_ms"] is not None else "-") + " |"
                            for r in report.rows))
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
