"""Time of a comparison of two states (gs_fields_compare, gs_members_compare) with the summary measured beside it, and of
the device copies behind a snapshot, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and for an ensemble of 512 members of 64 x 128: after a few warm-up
steps a snapshot is taken and a few more steps run; then ``Species.change_since`` and ``Species.summary`` are called
``--calls`` times each, in turns, each call timed twice -- device events around it on the context's compute stream (the
row kernel and the copy of its records: what the chip spends) and the host clock around the whole blocking call -- and
``Species.snapshot()`` (two planes created and filled) and ``Snapshot.update`` (filled again) with the host clock.
Medians are reported.  A (U, V) comparison reads four planes (16 bytes per cell) where the summary reads two (8 bytes per
cell): the plane-read rate of each against its device time, and the ratio of the two rates, are what the table is for.

    python tools/change_rate.py [--calls 20] [--grids 16384x16384,4096x4096,1080x1920] [--no-ensemble] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402
from ratekit import ENSEMBLE  # noqa: E402

HEADER = ["| grid | change_since, device (ms) | host call (ms) | plane reads (TB/s) | summary, device (ms) | host call (ms) |"
          " plane reads (TB/s) | read rate, change / summary | snapshot() (ms) | update (ms) | update, read + write (TB/s) |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]


def _host_ms(call):
    """(host ms, result) of one blocking call whose result is kept."""
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def _turns(ctx, compare, summarize, calls):
    """The two calls in turns, so that both see the same chip; their warm-up calls were made by the caller."""
    m = ratekit.medians(ctx, {"change": compare, "summary": summarize}, calls, warm=False, both=True)
    return {"change_device_ms": m["change"][1], "change_host_ms": m["change"][0],
            "summary_device_ms": m["summary"][1], "summary_host_ms": m["summary"][0]}


def time_species(rows, cols, calls):
    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        sim.perform_steps(species, 16)
        first_ms, snap = _host_ms(species.snapshot)
        sim.perform_steps(species, 8)
        species.change_since(snap)  # first launches: code object load
        species.summary()
        out = {"grid": f"{rows}x{cols}", "cells": rows * cols}
        out.update(_turns(ctx, lambda: species.change_since(snap), species.summary, calls))
        out["update_ms"] = statistics.median(ratekit.wall_ms(lambda: snap.update(species)) for _ in range(calls))
        snaps = []
        for _ in range(min(calls, 5)):
            ms, other = _host_ms(species.snapshot)
            other.close()
            snaps.append(ms)
        out["snapshot_ms"] = statistics.median(snaps)
        out["first_snapshot_ms"] = first_ms
        snap.close()
        return out


def time_ensemble(members, rows, cols, calls):
    with ratekit.ensemble_subject(members, rows, cols) as (sim, ctx, ens):
        ens.perform_steps(16)
        first_ms, snap = _host_ms(ens.snapshot)
        ens.perform_steps(8)
        ens.changes_since(snap)
        ens.summaries()
        out = {"grid": f"{members} x {rows}x{cols}", "cells": members * rows * cols}
        out.update(_turns(ctx, lambda: ens.changes_since(snap), ens.summaries, calls))
        out["update_ms"] = statistics.median(ratekit.wall_ms(lambda: snap.copy_from(ens)) for _ in range(calls))
        snaps = []
        for _ in range(min(calls, 5)):
            ms, other = _host_ms(ens.snapshot)
            other.destroy()
            snaps.append(ms)
        out["snapshot_ms"] = statistics.median(snaps)
        out["first_snapshot_ms"] = first_ms
        snap.destroy()
        return out


def main(argv=None) -> int:
    args = ratekit.observable_args(__doc__, argv, calls=20)
    report = ratekit.Report(args.json, args.md)
    rows = [time_species(r, c, args.calls) for r, c in ratekit.parse_grids(args.grids)]
    rows += [] if args.no_ensemble else [time_ensemble(*ENSEMBLE, args.calls)]
    for r in rows:
        r["change_read_tb_per_s"] = 16.0 * r["cells"] / (r["change_device_ms"] * 1e-3) / 1e12
        r["summary_read_tb_per_s"] = 8.0 * r["cells"] / (r["summary_device_ms"] * 1e-3) / 1e12
        r["read_rate_ratio"] = r["change_read_tb_per_s"] / r["summary_read_tb_per_s"]
        r["copy_tb_per_s"] = 16.0 * r["cells"] / (r["update_ms"] * 1e-3) / 1e12  # 8 bytes read + 8 written per cell
        report.row(r)
    report.table(*HEADER, *(
        f"| {r['grid']} | {r['change_device_ms']:.3f} | {r['change_host_ms']:.3f} | {r['change_read_tb_per_s']:.2f} | "
        f"{r['summary_device_ms']:.3f} | {r['summary_host_ms']:.3f} | {r['summary_read_tb_per_s']:.2f} | "
        f"{r['read_rate_ratio']:.2f} | {r['snapshot_ms']:.3f} | {r['update_ms']:.3f} | {r['copy_tb_per_s']:.2f} |" for r in rows))
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
