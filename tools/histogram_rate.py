"""Time of a histogram (gs_fields_histogram, gs_members_histogram) against a summary of the same planes, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and each of three distributions -- ``new`` (Species::new untouched:
one-valued), ``developed`` (uniform random planes after steps: a pattern) and ``random`` (uniform random values over every
bin) -- the histogram of U and V (256 bins unless ``--bins``) and their summary are timed alternately: device events
around the blocking call on the context's compute stream, ``--calls`` times each after a warm-up call, medians reported.
The yardstick is the summary -- the established cost of reading the two planes once with a wave per row --, so the table
gives the ratio histogram / summary per row and the ratio of the one-valued to the random input per grid.  The same for an
ensemble of 512 members of 64 x 128 (gs_members_histogram against gs_members_summarize).

    python tools/histogram_rate.py [--calls 9] [--bins 256] [--grids 16384x16384,4096x4096,1080x1920] [--json FILE] [--md FILE]

GS_HIP_LIBRARY=<a variant built with tools/ab_build.py NAME -DGS_HIST_FORM=n> times another form of the kernel.
Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = "16384x16384,4096x4096,1080x1920"
ENSEMBLE = (512, 64, 128)  # members, rows, cols
KINDS = ("new", "developed", "random")


def _timed(ctx, fn):
    ctx.timer_start()
    fn()
    return ctx.timer_stop()


def _pair(ctx, hist, summ, calls):
    """Medians (ms) of the two calls, timed alternately after one warm-up call each."""
    hist(), summ()
    h, s = [], []
    for _ in range(calls):
        h.append(_timed(ctx, hist))
        s.append(_timed(ctx, summ))
    return statistics.median(h), statistics.median(s)


def _fill(sim, species, kind, rows, cols):
    """Bring `species` (fresh from make_species) into the state `kind`, uploading in blocks of rows."""
    if kind == "new":
        return
    rng = np.random.default_rng(3)
    in_u, in_v, _, _ = species.in_out()
    u = rng.random((rows, cols), dtype=np.float32)
    in_u.upload(sim.context, u)
    u *= np.float32(0.5)
    in_v.upload(sim.context, u)
    if kind == "developed":
        sim.perform_steps(species, 64)


def time_species(rows, cols, kind, bins, calls):
    from grayscott_amd import HipArgs, Parameters, Simulation

    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    species = sim.make_species((rows, cols))
    _fill(sim, species, kind, rows, cols)
    hu, hv = species.histogram(bins)
    h_ms, s_ms = _pair(ctx, lambda: species.histogram(bins), species.summary, calls)
    out = {"grid": f"{rows}x{cols}", "input": kind, "cells": rows * cols, "bins": bins, "histogram_ms": h_ms, "summary_ms": s_ms,
           "filled_bins_u": int(np.count_nonzero(hu.counts)), "filled_bins_v": int(np.count_nonzero(hv.counts)),
           "largest_share_u": float(hu.counts.max()) / (rows * cols)}
    ctx.close()
    return out


def time_ensemble(members, rows, cols, bins, calls):
    from grayscott_amd import HipArgs, Parameters, Simulation

    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    ens = sim.make_ensemble((rows, cols), Parameters(), members=members)
    ens.perform_steps(16)
    h_ms, s_ms = _pair(ctx, lambda: ens.histograms(bins=bins), ens.summaries, calls)
    out = {"grid": f"{members} x {rows}x{cols}", "input": "new + 16 steps", "cells": members * rows * cols, "bins": bins,
           "histogram_ms": h_ms, "summary_ms": s_ms}
    ens.destroy()
    ctx.close()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--grids", default=GRIDS)
    ap.add_argument("--json", default=None, help="also write the rows as a JSON list")
    ap.add_argument("--md", default=None, help="also write the table as markdown")
    args = ap.parse_args(argv)
    import torch  # noqa: F401  (the process's HIP runtime is torch's, as in bench.py and the tests)

    rows = []
    for grid in args.grids.split(","):
        r, c = (int(x) for x in grid.split("x"))
        for kind in KINDS:
            rows.append(time_species(r, c, kind, args.bins, args.calls))
            print(json.dumps(rows[-1]), flush=True)
    rows.append(time_ensemble(*ENSEMBLE, args.bins, args.calls))
    print(json.dumps(rows[-1]), flush=True)
    random_ms = {r["grid"]: r["histogram_ms"] for r in rows if r["input"] == "random"}
    for r in rows:
        r["histogram_over_summary"] = r["histogram_ms"] / r["summary_ms"]
        r["read_tb_per_s"] = 8.0 * r["cells"] / (r["histogram_ms"] * 1e-3) / 1e12
        r["over_random"] = r["histogram_ms"] / random_ms[r["grid"]] if r["grid"] in random_ms else None
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    lines = ["| grid | input | bins | histogram (ms) | summary (ms) | histogram / summary | plane reads (TB/s) | / random input |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        rel = "" if r["over_random"] is None else f"{r['over_random']:.2f}"
        lines.append(f"| {r['grid']} | {r['input']} | {r['bins']} | {r['histogram_ms']:.3f} | {r['summary_ms']:.3f} | "
                     f"{r['histogram_over_summary']:.2f} | {r['read_tb_per_s']:.2f} | {rel} |")
    print("\n".join(lines))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
