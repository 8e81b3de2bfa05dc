"""Time of the on-device power spectra (gs_fields_spectrum, gs_members_spectrum) against the summaries, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) in the state ``developed`` (64 steps from uniform random values) and
for an ensemble of 512 members of 64 x 128, the spectra of U and V with tiles of 16, 64 and 128 cells a side, with the
periodic Hann window and without a window, are timed beside ``gs_fields_summarize`` (``gs_members_summarize``) of the same
planes -- the cheapest observable that reads every cell once: device events around the blocking call on the context's compute
stream, ``--calls`` times each in turn after a warm-up call, medians reported, and the ratio spectrum / summary.  The host
route -- the download of both planes plus ``numpy.fft.rfft2`` of every whole tile of both, mean removed and windowed -- is
timed once per row (wall clock) on grids of at most ``--host-cells`` cells; the download alone is timed beside it.

    python tools/spectrum_rate.py [--calls 5] [--grids 16384x16384,4096x4096,1080x1920] [--tiles 16,64,128] [--no-ensemble]
                                  [--no-host] [--host-cells N] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402

TILES = "16,64,128"
WINDOWS = ("hann", "none")
HEADER = ["| planes | T | window | spectrum (ms) | summary (ms) | ratio | download (ms) | host route (ms) |",
          "|---|---|---|---|---|---|---|---|"]


def host_spectrum(planes, T, window):
    """numpy's route on downloaded planes [n, rows, cols]: rfft2 of every whole tile, mean removed and windowed, f64."""
    import numpy as np

    n, rows, cols = planes.shape
    nb, nt = rows // T, cols // T
    if nb == 0 or nt == 0:
        return np.zeros((n, T, T // 2 + 1))
    tiles = planes[:, :nb * T, :nt * T].reshape(n, nb, T, nt, T).transpose(0, 1, 3, 2, 4).astype(np.float64)
    tiles -= tiles.mean(axis=(3, 4), keepdims=True)
    if window == "hann":
        h = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(T) / T)
        tiles *= h[:, None] * h[None, :]
    return (np.abs(np.fft.rfft2(tiles, axes=(3, 4))) ** 2).sum(axis=(1, 2))


def rows_of(label, cells, ctx, spectrum, summary, download, tiles, calls, host):
    import numpy as np

    fns = {"summary_ms": summary}
    for T in tiles:
        for window in WINDOWS:
            fns[f"{T}_{window}"] = lambda T=T, window=window: spectrum(T, window)
    m = ratekit.medians(ctx, fns, calls)
    planes, download_ms = None, None
    if host:
        download_ms = ratekit.wall_ms(download)
        planes = np.stack(download())
    for T in tiles:
        for window in WINDOWS:
            rec = {"planes": label, "cells": cells, "tile": T, "window": window, "spectrum_ms": m[f"{T}_{window}"],
                   "summary_ms": m["summary_ms"], "ratio": m[f"{T}_{window}"] / m["summary_ms"], "download_ms": download_ms,
                   "host_ms": None}
            if host:
                rec["host_ms"] = download_ms + ratekit.wall_ms(lambda: host_spectrum(planes, T, window))
            yield rec


def main(argv=None) -> int:
    def add(ap):
        ap.add_argument("--tiles", default=TILES, help="comma-separated tile sizes (16, 32, 64, 128)")
        ap.add_argument("--no-host", action="store_true", help="leave the host route out")
        ap.add_argument("--host-cells", type=int, default=1 << 24, help="the host route is timed on grids of at most this many cells")

    args = ratekit.observable_args(__doc__, argv, calls=5, add=add)
    report = ratekit.Report(args.json, args.md)
    tiles = [int(x) for x in args.tiles.split(",") if x]
    for r, c in ratekit.parse_grids(args.grids):
        with ratekit.species_subject(r, c) as (sim, ctx, species):
            ratekit.fill(sim, species, "developed")
            in_u, in_v, _, _ = species.in_out()
            for rec in rows_of(f"{r}x{c} U, V", 2 * r * c, ctx, species.spectrum, species.summary,
                               lambda: (in_u.make_scalar_view(ctx), in_v.make_scalar_view(ctx)), tiles, args.calls,
                               not args.no_host and r * c <= args.host_cells):
                report.row(rec)
    if not args.no_ensemble:
        members, r, c = ratekit.ENSEMBLE
        with ratekit.ensemble_subject(members, r, c) as (sim, ctx, ens):
            ens.perform_steps(64)

            def download():  # every member's U, then every member's V: [2 members, rows, cols]
                import numpy as np

                return np.concatenate((ens.u_views(), ens.result_views()))

            for rec in rows_of(f"{members} members of {r}x{c}", 2 * members * r * c, ctx,
                               lambda T, window: ens.spectra(tile=T, window=window), ens.summaries, download,
                               [T for T in tiles if T <= min(r, c)], args.calls, not args.no_host):
                report.row(rec)

    def ms(x, digits=3):
        return f"{x:.{digits}f}" if x is not None else "-"

    report.table(*HEADER, *(f"| {x['planes']} | {x['tile']} | {x['window']} | {ms(x['spectrum_ms'])} | {ms(x['summary_ms'])} | "
                            f"{x['ratio']:.2f} | {ms(x['download_ms'], 1)} | {ms(x['host_ms'], 1)} |" for x in report.rows))
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
