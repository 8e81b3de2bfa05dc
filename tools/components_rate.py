"""Time of a components call (gs_fields_components, gs_members_components) against two things beside it, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and each of three inputs -- ``new`` (Species::new untouched),
``developed`` (uniform random planes after steps: a spot pattern) and ``random`` (cells set with probability 0.59, the
4-connected percolation regime: the worst case for union-find) -- the connected components of V at ONE threshold are timed
under connectivity 8 and under 4, in turn with

* ``gs_fields_morphology`` with one threshold on the same plane: the one-pass floor of reading the plane;
* a download of the plane plus ``scipy.ndimage.label`` and a ``bincount`` of the sizes, where scipy is present: what a user
  does without the call (``--label-calls`` times, default 1: it takes seconds at 16384^2).

The calls block and the components call allocates and frees its label memory inside, so every figure is the wall time of the
call (``time.perf_counter`` around it, after a warm-up call; medians of ``--calls``); the time between device events on the
compute stream is given beside it for the two device calls.  The same for an ensemble of 512 members of 64 x 128
(gs_members_components against gs_members_morphology; the download is of both species of all members).

    python tools/components_rate.py [--calls 9] [--label-calls 1] [--grids 16384x16384,4096x4096,1080x1920] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402
from ratekit import ENSEMBLE, KINDS  # noqa: E402

TV, TU = 0.25, 0.5
DENSITY = 0.59
HEADER = ["| grid | input | components | components, 8 (ms) | components, 4 (ms) | morphology (ms) | 8 / morphology | "
          "download + label (ms) | label / components |",
          "|---|---|---|---|---|---|---|---|---|"]


def scipy_ndimage(label_calls):
    """scipy.ndimage where it is present and the download + label route is to be timed."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    return ndimage if label_calls > 0 else None


def fill(sim, species, kind):
    """ratekit.fill, but ``random`` is V = 0.5 on cells drawn with probability DENSITY and 0 on the others."""
    if kind != "random":
        return ratekit.fill(sim, species, kind)
    rng = np.random.default_rng(3)
    v = np.where(rng.random(tuple(species.shape()), dtype=np.float32) < np.float32(DENSITY), np.float32(0.5), np.float32(0.0))
    species.in_out()[1].upload(sim.context, v.astype(np.float32))


def _host_label(ndimage, plane, threshold, structure):
    labels, n = ndimage.label(plane > np.float32(threshold), structure)
    sizes = np.bincount(labels.ravel())[1:]
    return n, int(sizes.max()) if n else 0


def _columns(m):
    return {"components8_ms": m["c8"][0], "components4_ms": m["c4"][0], "morphology_ms": m["morph"][0],
            "components8_event_ms": m["c8"][1], "components4_event_ms": m["c4"][1], "morphology_event_ms": m["morph"][1]}


def time_species(rows, cols, kind, calls, label_calls):
    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        fill(sim, species, kind)
        _, in_v, _, _ = species.in_out()
        c8 = in_v.components(ctx, [TV], True, 8)[0]
        m = ratekit.medians(ctx, {"c8": lambda: in_v.components(ctx, [TV], True, 8), "c4": lambda: in_v.components(ctx, [TV], True, 4),
                                  "morph": lambda: in_v.morphology(ctx, [TV])}, calls, both=True)
        out = {"grid": f"{rows}x{cols}", "input": kind, "cells": rows * cols, **_columns(m), "components": c8.count,
               "largest_fraction": c8.largest_fraction, "label_memory_bytes": 8 * rows * cols, "download_label_ms": None}
        ndimage = scipy_ndimage(label_calls)
        if ndimage is not None:
            eight = ndimage.generate_binary_structure(2, 2)
            got = []
            out["download_label_ms"] = statistics.median(
                ratekit.wall_ms(lambda: got.append(_host_label(ndimage, in_v.make_scalar_view(ctx), TV, eight)))
                for _ in range(label_calls))
            if got[-1] != (c8.count, c8.largest):
                raise RuntimeError(f"{out['grid']} {kind}: the device counts {(c8.count, c8.largest)}, scipy {got[-1]}")
        return out


def time_ensemble(members, rows, cols, calls, label_calls):
    with ratekit.ensemble_subject(members, rows, cols) as (sim, ctx, ens):
        ens.perform_steps(16)
        m = ratekit.medians(ctx, {"c8": lambda: ens.components(v_thresholds=[TV], u_thresholds=[TU], connectivity=8),
                                  "c4": lambda: ens.components(v_thresholds=[TV], u_thresholds=[TU], connectivity=4),
                                  "morph": lambda: ens.morphologies(v_thresholds=[TV], u_thresholds=[TU])}, calls, both=True)
        out = {"grid": f"{members} x {rows}x{cols}", "input": "new + 16 steps, U and V", "cells": 2 * members * rows * cols,
               **_columns(m), "components": None, "largest_fraction": None, "label_memory_bytes": 8 * members * rows * cols,
               "download_label_ms": None}
        ndimage = scipy_ndimage(label_calls)
        if ndimage is not None:
            eight = ndimage.generate_binary_structure(2, 2)

            def host():
                u, v = ens.u_views(), ens.result_views()
                for i in range(members):
                    _host_label(ndimage, -u[i], -TU, eight)
                    _host_label(ndimage, v[i], TV, eight)

            out["download_label_ms"] = statistics.median(ratekit.wall_ms(host) for _ in range(label_calls))
        return out


def main(argv=None) -> int:
    args = ratekit.observable_args(__doc__, argv, calls=9, add=lambda ap: ap.add_argument(
        "--label-calls", type=int, default=1, help="timed runs of the download + scipy.ndimage.label (0: none)"))
    report = ratekit.Report(args.json, args.md)
    for r, c in ratekit.parse_grids(args.grids):
        for kind in KINDS:
            report.row(time_species(r, c, kind, args.calls, args.label_calls))
    if not args.no_ensemble:
        report.row(time_ensemble(*ENSEMBLE, args.calls, args.label_calls))
    rows = report.rows
    for r in rows:
        r["components8_over_morphology"] = r["components8_ms"] / r["morphology_ms"]
        r["label_over_components8"] = r["download_label_ms"] / r["components8_ms"] if r["download_label_ms"] else None
    report.table(*HEADER)
    for r in rows:
        label = f"{r['download_label_ms']:.1f}" if r["download_label_ms"] else "-"
        ratio = f"{r['label_over_components8']:.1f}" if r["label_over_components8"] else "-"
        report.table(f"| {r['grid']} | {r['input']} | {r['components'] if r['components'] is not None else '-'} | "
                     f"{r['components8_ms']:.3f} | {r['components4_ms']:.3f} | {r['morphology_ms']:.3f} | "
                     f"{r['components8_over_morphology']:.1f} | {label} | {ratio} |")
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
