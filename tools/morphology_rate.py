"""Time of a morphology call (gs_fields_morphology, gs_members_morphology) against a summary of the same planes, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and each of three inputs -- ``new`` (Species::new untouched),
``developed`` (uniform random planes after steps: a pattern) and ``random`` (uniform random values: half the cells set) --
the bit-quad counts of U and V with one threshold each (nt = 1) and with four (nt = 4) and their summary are timed in turn:
device events around the blocking call on the context's compute stream, ``--calls`` times each after a warm-up call, medians
reported.  The yardstick is the summary -- the established cost of reading the two planes once with a wave per row --, so the
table gives the ratios morphology / summary.  The same for an ensemble of 512 members of 64 x 128 (gs_members_morphology
against gs_members_summarize).

    python tools/morphology_rate.py [--calls 9] [--grids 16384x16384,4096x4096,1080x1920] [--json FILE] [--md FILE]

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
TV, TU = (0.25, 0.1, 0.05, 0.4), (0.5, 0.8, 0.3, 0.95)


def _timed(ctx, fn):
    ctx.timer_start()
    fn()
    return ctx.timer_stop()


def _trio(ctx, one, four, summ, calls):
    """Medians (ms) of the three calls, timed in turn after one warm-up call each."""
    one(), four(), summ()
    a, b, s = [], [], []
    for _ in range(calls):
        a.append(_timed(ctx, one))
        b.append(_timed(ctx, four))
        s.append(_timed(ctx, summ))
    return statistics.median(a), statistics.median(b), statistics.median(s)


def _fill(sim, species, kind, rows, cols):
    """Bring `species` (fresh from make_species) into the state `kind`."""
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


def time_species(rows, cols, kind, calls):
    from grayscott_amd import HipArgs, Parameters, Simulation

    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    species = sim.make_species((rows, cols))
    _fill(sim, species, kind, rows, cols)
    _, mv = species.morphology(TV[:1], TU[:1])
    one_ms, four_ms, s_ms = _trio(ctx, lambda: species.morphology(TV[:1], TU[:1]), lambda: species.morphology(TV, TU),
                                  species.summary, calls)
    out = {"grid": f"{rows}x{cols}", "input": kind, "cells": rows * cols, "nt1_ms": one_ms, "nt4_ms": four_ms, "summary_ms": s_ms,
           "v_area_fraction": mv[0].area_fraction, "v_euler8": mv[0].euler8}
    ctx.close()
    return out


def time_ensemble(members, rows, cols, calls):
    from grayscott_amd import HipArgs, Parameters, Simulation

    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    ens = sim.make_ensemble((rows, cols), Parameters(), members=members)
    ens.perform_steps(16)
    one_ms, four_ms, s_ms = _trio(ctx, lambda: ens.morphologies(v_thresholds=TV[:1], u_thresholds=TU[:1]),
                                  lambda: ens.morphologies(v_thresholds=TV, u_thresholds=TU), ens.summaries, calls)
    out = {"grid": f"{members} x {rows}x{cols}", "input": "new + 16 steps", "cells": members * rows * cols, "nt1_ms": one_ms,
           "nt4_ms": four_ms, "summary_ms": s_ms}
    ens.destroy()
    ctx.close()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--grids", default=GRIDS)
    ap.add_argument("--json", default=None, help="also write the rows as a JSON list")
    ap.add_argument("--md", default=None, help="also write the table as markdown")
    args = ap.parse_args(argv)
    import torch  # noqa: F401  (the process's HIP runtime is torch's, as in bench.py and the tests)

    rows = []
    for grid in args.grids.split(","):
        r, c = (int(x) for x in grid.split("x"))
        for kind in KINDS:
            rows.append(time_species(r, c, kind, args.calls))
            print(json.dumps(rows[-1]), flush=True)
    rows.append(time_ensemble(*ENSEMBLE, args.calls))
    print(json.dumps(rows[-1]), flush=True)
    for r in rows:
        r["nt1_over_summary"] = r["nt1_ms"] / r["summary_ms"]
        r["nt4_over_summary"] = r["nt4_ms"] / r["summary_ms"]
        r["nt1_read_tb_per_s"] = 8.0 * r["cells"] / (r["nt1_ms"] * 1e-3) / 1e12
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    lines = ["| grid | input | nt = 1 (ms) | nt = 4 (ms) | summary (ms) | nt = 1 / summary | nt = 4 / summary | plane reads, nt = 1 (TB/s) |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['grid']} | {r['input']} | {r['nt1_ms']:.3f} | {r['nt4_ms']:.3f} | {r['summary_ms']:.3f} | "
                     f"{r['nt1_over_summary']:.2f} | {r['nt4_over_summary']:.2f} | {r['nt1_read_tb_per_s']:.2f} |")
    print("\n".join(lines))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
