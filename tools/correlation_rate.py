"""Time of a correlation call (gs_fields_correlation, gs_members_correlation) against a summary and a morphology call on the
same planes, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and each of three inputs -- ``new`` (Species::new untouched),
``developed`` (uniform random planes after steps: a pattern) and ``random`` (uniform random values: half the cells set) --
the pair counts of U and V with one threshold each at L = 16, 32 and 64, with four thresholds at L = 32, their summary and
their morphology with one threshold are timed in turn: device events around the blocking call on the context's compute
stream, ``--calls`` times each after a warm-up call, medians reported.  The yardsticks are the summary and the morphology
call, so the table gives the ratios to both.  The same for an ensemble of 512 members of 64 x 128.

    python tools/correlation_rate.py [--calls 9] [--grids 16384x16384,4096x4096,1080x1920] [--json FILE] [--md FILE]

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
COLUMNS = ("l16_ms", "l32_ms", "l64_ms", "nt4_l32_ms", "summary_ms", "morphology_ms")


def _timed(ctx, fn):
    ctx.timer_start()
    fn()
    return ctx.timer_stop()


def _medians(ctx, fns, calls):
    """Medians (ms) of the calls, timed in turn after one warm-up call each."""
    for fn in fns:
        fn()
    t = [[] for _ in fns]
    for _ in range(calls):
        for i, fn in enumerate(fns):
            t[i].append(_timed(ctx, fn))
    return [statistics.median(x) for x in t]


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
    fns = [lambda: species.correlation(TV[:1], TU[:1], max_lag=16), lambda: species.correlation(TV[:1], TU[:1], max_lag=32),
           lambda: species.correlation(TV[:1], TU[:1], max_lag=64), lambda: species.correlation(TV, TU, max_lag=32),
           species.summary, lambda: species.morphology(TV[:1], TU[:1])]
    out = {"grid": f"{rows}x{cols}", "input": kind, "cells": rows * cols}
    out.update(zip(COLUMNS, _medians(ctx, fns, calls)))
    _, cv = species.correlation(TV[:1], TU[:1], max_lag=32)
    out["v_fraction"] = cv[0].fraction
    out["v_first_minimum_rows"] = cv[0].first_minimum(0)
    ctx.close()
    return out


def time_ensemble(members, rows, cols, calls):
    from grayscott_amd import HipArgs, Parameters, Simulation

    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    ens = sim.make_ensemble((rows, cols), Parameters(), members=members)
    ens.perform_steps(16)
    one = {"v_thresholds": TV[:1], "u_thresholds": TU[:1]}
    fns = [lambda: ens.correlations(max_lag=16, **one), lambda: ens.correlations(max_lag=32, **one),
           lambda: ens.correlations(max_lag=64, **one), lambda: ens.correlations(v_thresholds=TV, u_thresholds=TU, max_lag=32),
           ens.summaries, lambda: ens.morphologies(**one)]
    out = {"grid": f"{members} x {rows}x{cols}", "input": "new + 16 steps", "cells": members * rows * cols}
    out.update(zip(COLUMNS, _medians(ctx, fns, calls)))
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
        r["l32_over_summary"] = r["l32_ms"] / r["summary_ms"]
        r["l32_over_morphology"] = r["l32_ms"] / r["morphology_ms"]
        r["l64_over_morphology"] = r["l64_ms"] / r["morphology_ms"]
        r["l32_read_tb_per_s"] = 8.0 * r["cells"] / (r["l32_ms"] * 1e-3) / 1e12
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    lines = ["| grid | input | L = 16 (ms) | L = 32 (ms) | L = 64 (ms) | nt = 4, L = 32 (ms) | summary (ms) | morphology (ms) | "
             "L = 32 / summary | L = 32 / morphology | L = 64 / morphology | plane reads, L = 32 (TB/s) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['grid']} | {r['input']} | {r['l16_ms']:.3f} | {r['l32_ms']:.3f} | {r['l64_ms']:.3f} | "
                     f"{r['nt4_l32_ms']:.3f} | {r['summary_ms']:.3f} | {r['morphology_ms']:.3f} | {r['l32_over_summary']:.2f} | "
                     f"{r['l32_over_morphology']:.2f} | {r['l64_over_morphology']:.2f} | {r['l32_read_tb_per_s']:.2f} |")
    print("\n".join(lines))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
