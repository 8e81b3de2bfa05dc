"""Time of a component match call (gs_fields_match, gs_members_match) against two things beside it, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and each of three inputs -- ``new`` (Species::new), ``developed`` and
``random`` (tools/ratekit.py: ``fill``) -- a snapshot is taken, the Species takes ``--steps-between`` steps (default 32) and V
above ONE threshold is matched with the snapshot under connectivity 8, min_size 1.  The match call is timed in turn with

* the two ``component_list`` calls of the same planes and rule (the snapshot's V and the current V): what a match costs beyond
  the two lists it holds;
* a download of both planes plus the scipy restatement -- ``scipy.ndimage.label`` twice and a ``np.unique`` over the label
  pairs of the cells set in both --, where scipy is present: what a user does without the call (``--label-calls`` times,
  default 1: it takes seconds at 16384^2).  Its overlaps are checked against the device's.

The calls block and allocate and free their label, record and overlap memory inside, so every figure is the wall time of the
call (``time.perf_counter`` around it, after a warm-up call; medians of ``--calls``); the time between device events on the
compute stream is given beside it.  The match call's wall time includes copying the lists and overlaps into numpy arrays.
The same for an ensemble of 512 members of 64 x 128 (gs_members_match against two gs_members_component_list).  The kernels'
registers, LDS and scratch (tools/codeobj.py) head the page.

    python tools/match_rate.py [--calls 9] [--label-calls 1] [--steps-between 32] [--grids 16384x16384,4096x4096,1080x1920]
                               [--json FILE] [--md profiles/match.md]

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
from components_rate import scipy_ndimage  # noqa: E402

TV = 0.25
KERNELS = ("gs_comp_tile_k<false, true>", "gs_comp_border_k", "gs_comp_flatten_k", "gs_list_count_k", "gs_list_scan_k",
           "gs_list_write_k", "gs_list_gather_k", "gs_match_pairs_k")
HEADER = ["| grid | input | before / after records | overlaps | match (ms) | two lists (ms) | match / two lists | match, device (ms) | "
          "download + label + join (ms) | host / match |",
          "|---|---|---|---|---|---|---|---|---|---|"]


def resources():
    """The markdown table of the kernels a match launches, from the built library's code objects."""
    import codeobj

    found = {k.name.split("(")[0]: k for k in codeobj.kernels(disassemble=False)}
    lines = ["| kernel | VGPRs | SGPRs | LDS (bytes) | scratch | spills |", "|---|---|---|---|---|---|"]
    for name in KERNELS:
        k = found.get(name)
        if k is None:
            raise RuntimeError(f"no kernel {name} in the library")
        lines.append(f"| `{name}` | {k.vgpr} | {k.sgpr} | {k.lds} | {k.scratch} | {k.vgpr_spill + k.sgpr_spill} |")
    return lines


def _host_match(ndimage, before, after, threshold, structure):
    """(components before, after, overlaps as rows of (label before, label after, cells)) by scipy."""
    lb, nb = ndimage.label(before > np.float32(threshold), structure)
    la, na = ndimage.label(after > np.float32(threshold), structure)
    both = (lb > 0) & (la > 0)
    keys = lb[both].astype(np.int64) * (na + 1) + la[both]
    uniq, cells = np.unique(keys, return_counts=True)
    return nb, na, np.stack([uniq // (na + 1) - 1, uniq % (na + 1) - 1, cells], axis=1).reshape(-1, 3)


def _same(match, host):
    nb, na, rows = host
    ov = match.overlaps
    return (match.before.count, match.after.count) == (nb, na) and rows.shape[0] == ov.shape[0] and \
        np.array_equal(rows[:, 0], ov["before"]) and np.array_equal(rows[:, 1], ov["after"]) and np.array_equal(rows[:, 2], ov["cells"])


def _row(grid, kind, cells, got, m):
    return {"grid": grid, "input": kind, "cells": cells, "records_before": got.before.count, "records_after": got.after.count,
            "overlaps": int(got.overlaps.shape[0]), **got.counts(), "match_ms": m["match"][0], "match_event_ms": m["match"][1],
            "lists_ms": m["lists"][0], "lists_event_ms": m["lists"][1], "download_label_ms": None}


def time_species(rows, cols, kind, calls, label_calls, between):
    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        ratekit.fill(sim, species, kind)
        snap = species.snapshot()
        sim.perform_steps(species, between)
        _, in_v, _, _ = species.in_out()
        got = species.match_since(snap, TV)

        def lists():
            snap.v.component_list(ctx, TV, True, 8)
            in_v.component_list(ctx, TV, True, 8)

        m = ratekit.medians(ctx, {"match": lambda: species.match_since(snap, TV), "lists": lists}, calls, both=True)
        out = _row(f"{rows}x{cols}", kind, rows * cols, got, m)
        ndimage = scipy_ndimage(label_calls)
        if ndimage is not None:
            eight = ndimage.generate_binary_structure(2, 2)
            host = []
            out["download_label_ms"] = statistics.median(
                ratekit.wall_ms(lambda: host.append(_host_match(ndimage, snap.v.make_scalar_view(ctx), in_v.make_scalar_view(ctx), TV,
                                                                eight)))
                for _ in range(label_calls))
            if not _same(got, host[-1]):
                raise RuntimeError(f"{out['grid']} {kind}: the device's match is not scipy's")
        return out


def time_ensemble(members, rows, cols, calls, label_calls, between):
    with ratekit.ensemble_subject(members, rows, cols) as (sim, ctx, ens):
        ens.perform_steps(16)
        snap = ens.snapshot()
        ens.perform_steps(between)
        got = ens.matches_since(snap, threshold=TV)

        def lists():
            snap.component_lists(threshold=TV)
            ens.component_lists(threshold=TV)

        m = ratekit.medians(ctx, {"match": lambda: ens.matches_since(snap, threshold=TV), "lists": lists}, calls, both=True)
        out = {"grid": f"{members} x {rows}x{cols}", "input": f"new + 16 steps, then {between}", "cells": members * rows * cols,
               "records_before": sum(g.before.count for g in got), "records_after": sum(g.after.count for g in got),
               "overlaps": sum(int(g.overlaps.shape[0]) for g in got), "match_ms": m["match"][0], "match_event_ms": m["match"][1],
               "lists_ms": m["lists"][0], "lists_event_ms": m["lists"][1], "download_label_ms": None}
        ndimage = scipy_ndimage(label_calls)
        if ndimage is not None:
            eight = ndimage.generate_binary_structure(2, 2)
            host = []

            def route():
                before, after = snap.result_views(), ens.result_views()
                host[:] = [_host_match(ndimage, before[i], after[i], TV, eight) for i in range(members)]

            out["download_label_ms"] = statistics.median(ratekit.wall_ms(route) for _ in range(label_calls))
            if not all(_same(g, h) for g, h in zip(got, host)):
                raise RuntimeError("ensemble: the device's matches are not scipy's")
        snap.destroy()
        return out


def _flags(ap):
    ap.add_argument("--label-calls", type=int, default=1, help="timed runs of the download + scipy route (0: none)")
    ap.add_argument("--steps-between", type=int, default=32, help="steps from the snapshot to the state matched with it")
    ap.add_argument("--kinds", default=",".join(KINDS))


def main(argv=None) -> int:
    args = ratekit.observable_args(__doc__, argv, calls=9, add=_flags)
    report = ratekit.Report(args.json, args.md)
    report.table("# Component matches on the device (`gs_fields_match`, `gs_members_match`)", "",
                 "Written by `python tools/match_rate.py`.  The pieces are labelled by the tile kernel's two-label-array form "
                 "(`gs_comp_tile_k<false, true>`), not through an f32 plane.", "",
                 "## Resources (gfx950, hipcc's default float mode)", "", *resources(), "",
                 f"## Times (V above {TV}, connectivity 8, min_size 1; the snapshot lies {args.steps_between} steps back; medians of "
                 f"{args.calls} calls, wall time unless it says device)", "")
    for r, c in ratekit.parse_grids(args.grids):
        for kind in filter(None, args.kinds.split(",")):
            report.row(time_species(r, c, kind, args.calls, args.label_calls, args.steps_between))
    if not args.no_ensemble:
        report.row(time_ensemble(*ENSEMBLE, args.calls, args.label_calls, args.steps_between))
    report.table(*HEADER)
    for r in report.rows:
        label = f"{r['download_label_ms']:.1f}" if r["download_label_ms"] else "-"
        ratio = f"{r['download_label_ms'] / r['match_ms']:.1f}" if r["download_label_ms"] else "-"
        report.table(f"| {r['grid']} | {r['input']} | {r['records_before']} / {r['records_after']} | {r['overlaps']} | "
                     f"{r['match_ms']:.3f} | {r['lists_ms']:.3f} | {r['match_ms'] / r['lists_ms']:.2f} | {r['match_event_ms']:.3f} | "
                     f"{label} | {ratio} |")
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
