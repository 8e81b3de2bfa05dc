"""Time of a component list call (gs_field_component_list, gs_members_component_list) against two things beside it, in one
process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and each of four inputs -- ``new`` (Species::new untouched),
``developed`` (a lattice of seed squares, one every 48 cells, after 1500 steps: spots of V > 0.25 all over the plane), ``full`` (every cell set: one component, the
worst contention of the gather's atomics) and ``random`` (cells set with probability 0.59: millions of records) -- the
component list of V at ONE threshold under connectivity 8 is timed in turn with

* ``gs_fields_components`` with the same arguments: the labelling both share, so the difference is what the records cost;
* a download of the plane plus ``scipy.ndimage.label``, ``find_objects`` and two ``sum_labels``, where scipy is present: what
  a user does without the call (``--label-calls`` times, default 1: it takes seconds at 16384^2).

The calls block and allocate and free their label and record memory inside, so every figure is the wall time of the call
(``time.perf_counter`` around it, after a warm-up call; medians of ``--calls``); the time between device events on the compute
stream is given beside it.  The list call's wall time includes copying the records into a numpy array.  The same for an
ensemble of 512 members of 64 x 128 (gs_members_component_list of V against gs_members_components).

    python tools/component_list_rate.py [--calls 9] [--label-calls 1] [--grids 16384x16384,4096x4096,1080x1920] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402
from ratekit import ENSEMBLE  # noqa: E402
from components_rate import fill, scipy_ndimage  # noqa: E402  (the same inputs)

KINDS = ("new", "developed", "full", "random")
TV = 0.25
HEADER = ["| grid | input | records | largest (cells) | list (ms) | list, min_size 5 (ms) | components (ms) | list / components | "
          "download + label + measure (ms) | host / list |",
          "|---|---|---|---|---|---|---|---|---|---|"]


def _develop(sim, species, rows, cols):
    """Species::new's square (U = 0.5, V = 0.25 on 8 x 8 cells) every 48 cells in both directions, then 1500 steps: the squares
    become spots, more than one per seed, whose cores stay above 0.25 (held to the CPU oracle on 192 x 192)."""
    in_rows = (np.arange(rows) % 48 >= 20) & (np.arange(rows) % 48 < 28)
    in_cols = (np.arange(cols) % 48 >= 20) & (np.arange(cols) % 48 < 28)
    seed = np.outer(in_rows, in_cols)
    in_u, in_v, _, _ = species.in_out()
    in_u.upload(sim.context, np.where(seed, np.float32(0.5), np.float32(1.0)).astype(np.float32))
    in_v.upload(sim.context, np.where(seed, np.float32(0.25), np.float32(0.0)).astype(np.float32))
    sim.perform_steps(species, 1500)


def _host_list(ndimage, plane, threshold, structure):
    labels, n = ndimage.label(plane > np.float32(threshold), structure)
    if n == 0:
        return 0, 0
    index = np.arange(1, n + 1)
    ndimage.find_objects(labels)
    r, c = np.indices(plane.shape, sparse=True)
    sizes = np.bincount(labels.ravel())[1:]
    ndimage.sum_labels(np.broadcast_to(r, plane.shape), labels, index)
    ndimage.sum_labels(np.broadcast_to(c, plane.shape), labels, index)
    return n, int(sizes.max())


def _columns(m):
    return {"list_ms": m["list"][0], "list_min5_ms": m["list5"][0], "components_ms": m["comp"][0], "list_event_ms": m["list"][1],
            "list_min5_event_ms": m["list5"][1], "components_event_ms": m["comp"][1], "download_label_ms": None}


def time_species(rows, cols, kind, calls, label_calls):
    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        if kind == "full":
            species.in_out()[1].upload(ctx, np.full((rows, cols), 0.5, np.float32))
        elif kind == "developed":
            _develop(sim, species, rows, cols)
        else:
            fill(sim, species, kind)
        _, in_v, _, _ = species.in_out()
        got = in_v.component_list(ctx, TV, True, 8)
        largest = int(got.sizes.max()) if got.count else 0
        m = ratekit.medians(ctx, {"list": lambda: in_v.component_list(ctx, TV, True, 8),
                                  "list5": lambda: in_v.component_list(ctx, TV, True, 8, 5),
                                  "comp": lambda: in_v.components(ctx, [TV], True, 8)}, calls, both=True)
        out = {"grid": f"{rows}x{cols}", "input": kind, "cells": rows * cols, "records": got.count, "largest": largest, **_columns(m)}
        ndimage = scipy_ndimage(label_calls)
        if ndimage is not None:
            eight = ndimage.generate_binary_structure(2, 2)
            host = []
            out["download_label_ms"] = statistics.median(
                ratekit.wall_ms(lambda: host.append(_host_list(ndimage, in_v.make_scalar_view(ctx), TV, eight)))
                for _ in range(label_calls))
            if host[-1] != (got.count, largest):
                raise RuntimeError(f"{out['grid']} {kind}: the device lists {(got.count, largest)}, scipy {host[-1]}")
        return out


def time_ensemble(members, rows, cols, calls, label_calls):
    with ratekit.ensemble_subject(members, rows, cols) as (sim, ctx, ens):
        ens.perform_steps(16)
        lists = ens.component_lists(threshold=TV)
        m = ratekit.medians(ctx, {"list": lambda: ens.component_lists(threshold=TV),
                                  "list5": lambda: ens.component_lists(threshold=TV, min_size=5),
                                  "comp": lambda: ens.components(v_thresholds=[TV], u_thresholds=[0.5])}, calls, both=True)
        out = {"grid": f"{members} x {rows}x{cols}", "input": "new + 16 steps, V (components: U and V)",
               "cells": members * rows * cols, "records": sum(c.count for c in lists),
               "largest": max([int(c.sizes.max()) for c in lists if c.count] or [0]), **_columns(m)}
        ndimage = scipy_ndimage(label_calls)
        if ndimage is not None:
            eight = ndimage.generate_binary_structure(2, 2)

            def host():
                v = ens.result_views()
                for i in range(members):
                    _host_list(ndimage, v[i], TV, eight)

            out["download_label_ms"] = statistics.median(ratekit.wall_ms(host) for _ in range(label_calls))
        return out


def _flags(ap):
    ap.add_argument("--label-calls", type=int, default=1, help="timed runs of the download + scipy route (0: none)")
    ap.add_argument("--kinds", default=",".join(KINDS))


def main(argv=None) -> int:
    args = ratekit.observable_args(__doc__, argv, calls=9, add=_flags)
    report = ratekit.Report(args.json, args.md)
    for r, c in ratekit.parse_grids(args.grids):
        for kind in filter(None, args.kinds.split(",")):
            report.row(time_species(r, c, kind, args.calls, args.label_calls))
    if not args.no_ensemble:
        report.row(time_ensemble(*ENSEMBLE, args.calls, args.label_calls))
    report.table(*HEADER)
    for r in report.rows:
        label = f"{r['download_label_ms']:.1f}" if r["download_label_ms"] else "-"
        ratio = f"{r['download_label_ms'] / r['list_ms']:.1f}" if r["download_label_ms"] else "-"
        report.table(f"| {r['grid']} | {r['input']} | {r['records']} | {r['largest']} | {r['list_ms']:.3f} | {r['list_min5_ms']:.3f} | "
                     f"{r['components_ms']:.3f} | {r['list_ms'] / r['components_ms']:.2f} | {label} | {ratio} |")
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
