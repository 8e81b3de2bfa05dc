"""Time of a comparison of two states (gs_fields_compare, gs_members_compare) with the summary measured beside it, and of
the device copies behind a snapshot, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and for an ensemble of 512 members of 64 x 128: after a few warm-up
steps a snapshot is taken and a few more steps run; then ``Species.change_since`` and ``Species.summary`` are called
``--calls`` times each, in turns, each call timed twice -- device events around it on the context's compute stream (the
row kernel and the copy of its records: what the chip spends) and the host clock around the whole blocking call -- and
``Species.snapshot()`` (two planes created and filled) and ``Snapshot.update`` (filled again) with the host clock.
Medians are reported.  A (U, V) comparison reads four planes (16 bytes per cell) where the summary reads two (8 bytes per
cell): the plane-read rate of each against its device time, and the ratio of the two rates, are what the table is for.

    python tools/change_rate.py [--calls 20] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(16384, 16384), (4096, 4096), (1080, 1920)]
ENSEMBLE = (512, 64, 128)  # members, rows, cols


def _timed(ctx, call):
    """(device ms, host ms) of one blocking call."""
    ctx.timer_start()
    t0 = time.perf_counter()
    call()
    host = (time.perf_counter() - t0) * 1e3
    return ctx.timer_stop(), host


def _host_ms(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def _medians(ctx, compare, summarize, calls):
    """The two calls in turns, so that both see the same chip: medians of (device, host) ms of each."""
    c, s = [], []
    for _ in range(calls):
        c.append(_timed(ctx, compare))
        s.append(_timed(ctx, summarize))
    med = lambda xs, i: statistics.median(x[i] for x in xs)  # noqa: E731
    return {"change_device_ms": med(c, 0), "change_host_ms": med(c, 1), "summary_device_ms": med(s, 0),
            "summary_host_ms": med(s, 1)}


def time_species(rows, cols, calls):
    from grayscott_amd import HipArgs, Parameters, Simulation

    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    species = sim.make_species((rows, cols))
    sim.perform_steps(species, 16)
    first_ms, snap = _host_ms(species.snapshot)
    sim.perform_steps(species, 8)
    species.change_since(snap)  # first launches: code object load
    species.summary()
    out = {"grid": f"{rows}x{cols}", "cells": rows * cols}
    out.update(_medians(ctx, lambda: species.change_since(snap), species.summary, calls))
    out["update_ms"] = statistics.median(_host_ms(lambda: snap.update(species))[0] for _ in range(calls))
    snaps = []
    for _ in range(min(calls, 5)):
        ms, other = _host_ms(species.snapshot)
        other.close()
        snaps.append(ms)
    out["snapshot_ms"] = statistics.median(snaps)
    out["first_snapshot_ms"] = first_ms
    snap.close()
    ctx.close()
    return out


def time_ensemble(members, rows, cols, calls):
    from grayscott_amd import HipArgs, Parameters, Simulation

    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    ens = sim.make_ensemble((rows, cols), Parameters(), members=members)
    ens.perform_steps(16)
    first_ms, snap = _host_ms(ens.snapshot)
    ens.perform_steps(8)
    ens.changes_since(snap)
    ens.summaries()
    out = {"grid": f"{members} x {rows}x{cols}", "cells": members * rows * cols}
    out.update(_medians(ctx, lambda: ens.changes_since(snap), ens.summaries, calls))
    out["update_ms"] = statistics.median(_host_ms(lambda: snap.copy_from(ens))[0] for _ in range(calls))
    snaps = []
    for _ in range(min(calls, 5)):
        ms, other = _host_ms(ens.snapshot)
        other.destroy()
        snaps.append(ms)
    out["snapshot_ms"] = statistics.median(snaps)
    out["first_snapshot_ms"] = first_ms
    snap.destroy()
    ens.destroy()
    ctx.close()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--json", default=None, help="also write the rows as a JSON list")
    ap.add_argument("--md", default=None, help="also write the table as markdown")
    args = ap.parse_args(argv)
    import torch  # noqa: F401  (the process's HIP runtime is torch's, as in bench.py and the tests)

    rows = [time_species(r, c, args.calls) for r, c in GRIDS] + [time_ensemble(*ENSEMBLE, args.calls)]
    for r in rows:
        r["change_read_tb_per_s"] = 16.0 * r["cells"] / (r["change_device_ms"] * 1e-3) / 1e12
        r["summary_read_tb_per_s"] = 8.0 * r["cells"] / (r["summary_device_ms"] * 1e-3) / 1e12
        r["read_rate_ratio"] = r["change_read_tb_per_s"] / r["summary_read_tb_per_s"]
        r["copy_tb_per_s"] = 16.0 * r["cells"] / (r["update_ms"] * 1e-3) / 1e12  # 8 bytes read + 8 written per cell
        print(json.dumps(r))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    lines = ["| grid | change_since, device (ms) | host call (ms) | plane reads (TB/s) | summary, device (ms) | host call (ms) |"
             " plane reads (TB/s) | read rate, change / summary | snapshot() (ms) | update (ms) | update, read + write (TB/s) |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['grid']} | {r['change_device_ms']:.3f} | {r['change_host_ms']:.3f} | {r['change_read_tb_per_s']:.2f} | "
                     f"{r['summary_device_ms']:.3f} | {r['summary_host_ms']:.3f} | {r['summary_read_tb_per_s']:.2f} | "
                     f"{r['read_rate_ratio']:.2f} | {r['snapshot_ms']:.3f} | {r['update_ms']:.3f} | {r['copy_tb_per_s']:.2f} |")
    print("\n".join(lines))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
