"""Time of the regional power spectra (gs_fields_region_spectrum) against the whole-grid spectrum, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) in the state ``developed`` (64 steps from uniform random values), every
region shape (64x64, 256x256, 1024x1024) and every tile size (16, 64, 128) with the periodic Hann window, the spectra of every
region of U and V are timed beside ``gs_fields_spectrum`` of the same planes with the same tile, and beside the regions'
summaries (``gs_fields_region_summaries``): device events around the blocking call on the context's compute stream,
``--calls`` times each in turn after a warm-up call, medians reported.  The regional call is timed twice: as
``Species.region_spectrum`` makes it, into result arrays that are allocated anew in every call and taken apart into a
``RegionSpectrum``, and as the library's call alone into a result that is allocated and touched once and then reused
(``reused``).  The yardstick is the whole-grid call beside it, so the table gives the ratios regional / whole-grid, of both
forms.  A regional call that the library refuses -- a result over GS_REGION_SPECTRUM_MAX words per field, or segment records
over GS_REGION_SPECTRUM_RECORDS_MAX words -- has cells that hold ``-``.  The host route -- the download of both planes plus
``numpy.fft.rfft2`` of every whole tile of every crop of U and V, mean removed and windowed -- is timed once per row (wall
clock) on grids of at most ``--host-cells`` cells.

    python tools/region_spectrum_rate.py [--calls 5] [--grids 16384x16384,4096x4096,1080x1920] [--regions 64x64,256x256,1024x1024]
                                         [--tiles 16,64,128] [--no-host] [--host-cells N] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402

REGIONS = "64x64,256x256,1024x1024"
TILES = "16,64,128"
WINDOW = "hann"
HEADER = ["| grid | region | T | region spectrum (ms) | reused (ms) | spectrum (ms) | ratio | region summaries (ms) | host route (ms) |",
          "|---|---|---|---|---|---|---|---|---|"]


def library_call(ctx, species, region, T):
    """The library's call alone on U and V, into a result that is allocated and touched here, once."""
    import ctypes

    import numpy as np

    from grayscott_amd import capi
    from grayscott_amd.simulation import _handle_array, region_grid

    in_u, in_v, _, _ = species.in_out()
    rows, cols = in_u.shape()
    grid = region_grid(rows, cols, region)
    power = np.empty((2,) + grid + (T, T // 2 + 1), np.float64)
    tiles = np.empty((2,) + grid + (2,), np.uint64)
    power.fill(0)
    tiles.fill(0)
    handles = _handle_array([in_u, in_v])
    to_power, to_tiles = power.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), tiles.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    return lambda: capi.check(ctx._lib.gs_fields_region_spectrum(ctx.handle, handles, 2, region[0], region[1], T, 1, to_power,
                                                                 to_tiles)), (power, tiles)


def host_route(ctx, species, region, T):
    """Download of both planes and numpy's rfft2 of every whole tile of every crop of U and V, mean removed and windowed, f64
    (not the library's rule -- the time is what is asked for here, not the bits)."""
    import numpy as np

    rh, rw = region
    in_u, in_v, _, _ = species.in_out()
    h = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(T) / T)
    out = []
    for plane in (in_u.make_scalar_view(ctx), in_v.make_scalar_view(ctx)):
        rows, cols = plane.shape
        power = np.zeros((-(-rows // rh), -(-cols // rw), T, T // 2 + 1))
        for i in range(power.shape[0]):
            for j in range(power.shape[1]):
                crop = plane[i * rh:(i + 1) * rh, j * rw:(j + 1) * rw]
                nb, nt = crop.shape[0] // T, crop.shape[1] // T
                if nb == 0 or nt == 0:
                    continue
                t = crop[:nb * T, :nt * T].reshape(nb, T, nt, T).transpose(0, 2, 1, 3).astype(np.float64)
                t -= t.mean(axis=(2, 3), keepdims=True)
                t *= h[:, None] * h[None, :]
                power[i, j] = (np.abs(np.fft.rfft2(t, axes=(2, 3))) ** 2).sum(axis=(0, 1))
        out.append(power)
    return out


def time_species(rows, cols, regions, tiles, calls, host):
    from grayscott_amd import capi

    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        ratekit.fill(sim, species, "developed")
        for region in regions:
            for T in tiles:
                fns = {"spectrum_ms": lambda: species.spectrum(T, WINDOW),
                       "region_summaries_ms": lambda: species.region_summaries(region)}
                try:  # (a result or record memory over its cap is refused before any device work)
                    species.region_spectrum(region, T, WINDOW)
                    fns["region_spectrum_ms"] = lambda: species.region_spectrum(region, T, WINDOW)
                    fns["region_spectrum_reused_ms"], _ = library_call(ctx, species, region, T)
                except capi.GsError as e:
                    if e.code != capi.GS_ERR_INVALID:
                        raise
                m = ratekit.medians(ctx, fns, calls)
                rec = {"grid": f"{rows}x{cols}", "region": f"{region[0]}x{region[1]}", "tile": T, "window": WINDOW, "cells": rows * cols,
                       "region_spectrum_ms": None, "region_spectrum_reused_ms": None, **m}
                rec["host_ms"] = ratekit.wall_ms(lambda: host_route(ctx, species, region, T)) if host else None
                yield rec


def main(argv=None) -> int:
    def add(ap):
        ap.add_argument("--regions", default=REGIONS, help="comma-separated RHxRW region shapes")
        ap.add_argument("--tiles", default=TILES, help="comma-separated tile sizes (16, 32, 64, 128)")
        ap.add_argument("--no-host", action="store_true", help="leave the host route out")
        ap.add_argument("--host-cells", type=int, default=1 << 24, help="the host route is timed on grids of at most this many cells")

    args = ratekit.observable_args(__doc__, argv, calls=5, add=add)
    report = ratekit.Report(args.json, args.md)
    regions, tiles = ratekit.parse_grids(args.regions), [int(x) for x in args.tiles.split(",") if x]
    for r, c in ratekit.parse_grids(args.grids):
        for rec in time_species(r, c, regions, tiles, args.calls, not args.no_host and r * c <= args.host_cells):
            report.row(rec)

    def ms(x):
        return f"{x:.3f}" if x is not None else "-"

    for r in report.rows:
        for key in ("region_spectrum_ms", "region_spectrum_reused_ms"):
            r[key.replace("_ms", "_ratio")] = r[key] / r["spectrum_ms"] if r[key] is not None else None
    report.table(*HEADER, *(f"| {r['grid']} | {r['region']} | {r['tile']} | {ms(r['region_spectrum_ms'])} | "
                            f"{ms(r['region_spectrum_reused_ms'])} | {r['spectrum_ms']:.3f} | "
                            + (f"{r['region_spectrum_ratio']:.2f} / {r['region_spectrum_reused_ratio']:.2f}"
                               if r["region_spectrum_ratio"] is not None else "-")
                            + f" | {r['region_summaries_ms']:.3f} | " + (f"{r['host_ms']:.1f}" if r["host_ms"] is not None else "-") + " |"
                            for r in report.rows))
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
