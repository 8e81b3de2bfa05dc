"""Rates of the zero-flux (Neumann) boundary rule against the clipped rule, in one process.

For every grid (16384^2, 4096^2, 1080 x 1920, 512 x 1024, and 16384^2 as a chain of 2 slabs on one GPU) and rule: a Species
seeded with Species::new's pattern, warm-up calls until the on-line tuner has settled (at most 40), then ``--calls`` calls
of ``--steps`` steps timed with device events around each call (median).  At 1080 x 1920 kernel = AUTO runs the persistent
window kernel for the clipped rule and the marching kernel for the zero-flux rule (which has no window-kernel form); the
clipped rule's marching kernel (kernel = TB) is timed too.  Every timed result is proven as bench.py proves its own: a
second context of the same rule and slabs replays the same number of steps from the same initial state with the
single-step cross-check kernel (GS_KERNEL_SIMPLE, one gs_step per step), and U and V must be bit for bit the same.  Then
an ensemble of 512 zero-flux members of 64 x 128 against the same members run one after another (a sample of them), with
a bit-check of one member.

    python tools/neumann_rate.py [--grids 16384x16384,1080x1920] [--steps 256] [--calls 5] [--md out.md] [--json out.jsonl]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402

GRIDS = "16384x16384,4096x4096,1080x1920,512x1024,16384x16384x2"  # rows x cols [x slabs]
RULES = [("clipped", 0), ("zero flux", 3)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--grids", default=None, help="comma-separated ROWSxCOLS or ROWSxCOLSxSLABS (default: the grids of the table)")
    ap.add_argument("--steps", type=int, default=256, help="steps per timed call")
    ap.add_argument("--calls", type=int, default=5, help="timed calls per grid and rule (median)")
    ap.add_argument("--sample", type=int, default=32, help="ensemble members timed one after another")
    ap.add_argument("--no-ensemble", action="store_true")
    ap.add_argument("--md", default=None, help="also write the tables to this file")
    ap.add_argument("--json", default=None, help="append one JSON line per measurement to this file")
    args = ap.parse_args(argv)
    report = ratekit.Report(args.json, args.md, json_lines=True)
    report.table("| grid | rule | kernel | Mcells x steps / s | / clipped | replay (simple kernel) |", "|---|---|---|---|---|---|")
    ok = True
    for rows, cols, slabs in ratekit.parse_grids(args.grids or GRIDS, slabs=True):
        for label, r, over_clipped in ratekit.rules_in_turn(RULES, lambda rule, pin: dict(
                ratekit.timed_steps(rows, cols, args.steps, args.calls, boundary=rule, kernel=pin, slabs=slabs),
                slabs=slabs, boundary=rule)):
            ok = ok and r["proof"]
            grid = f"{rows} x {cols}" + (f", {slabs} slabs" if slabs > 1 else "")
            report.table(f"| {grid} | {label} | {r['kernel']} | {r['rate']:.0f} | {over_clipped:.3f} | "
                         f"{r['replay_steps']} steps: {'identical' if r['proof'] else 'DIFFERS'} |")
            report.row(r)
    if not args.no_ensemble:
        report.table("", "| ensemble | rule | kernel | ensemble Mcells x steps / s | sequential Mcells x steps / s | speed-up | bit-check |",
                     "|---|---|---|---|---|---|---|")
        for label, rule in RULES:
            e = ratekit.ensemble_against_sequential(512, 64, 128, args.steps, args.calls, args.sample, boundary=rule)
            del e["bitcheck_max_abs_diff"]  # (this tool's records carry the rule instead)
            e["boundary"] = rule
            ok = ok and e["bitcheck"]
            report.table(f"| 512 x 64x128 | {label} | {e['kernel']} | {e['ensemble_rate']:.0f} | {e['sequential_rate']:.0f} "
                         f"({e['sequential_kernel']}) | {e['speedup']:.1f}x | member {e['bitcheck_member']}: "
                         f"{'identical' if e['bitcheck'] else 'DIFFERS'} |")
            report.row(e)
    report.finish()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
