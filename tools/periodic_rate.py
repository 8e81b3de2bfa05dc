"""Rates of the periodic boundary rule against the clipped and zero-halo rules, in one process.

For every grid (16384^2, 4096^2, 1080 x 1920, 512 x 1024) and rule: a Species seeded with Species::new's pattern, warm-up
calls until the on-line tuner has settled (gs_ctx_info names a tuned configuration; at most 40), then ``--calls`` calls of
``--steps`` steps timed with device events around each call (median).  Where kernel = AUTO runs another kernel than the
marching one for the clipped rule (the persistent window kernel at 1080 x 1920), the clipped rule's marching kernel
(kernel = TB) is timed too.  Every timed result is proven as bench.py proves its own: a second context of the same rule
replays the same number of steps from the same initial state with the single-step cross-check kernel (GS_KERNEL_SIMPLE,
one gs_step per step), and U and V must be bit for bit the same.  Then a periodic ensemble of 512 members of 64 x 128 against the same
members run one after another through gs_run (a sample of them), with a bit-check of one member.

    python tools/periodic_rate.py [--grids 16384x16384,1080x1920] [--steps 256] [--calls 5] [--md out.md] [--json out.jsonl]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402

GRIDS = "16384x16384,4096x4096,1080x1920,512x1024"
RULES = [("clipped", 0), ("zero halo", 1), ("periodic", 2)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--grids", default=None, help="comma-separated ROWSxCOLS (default: the four grids of the table)")
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
    for rows, cols in ratekit.parse_grids(args.grids or GRIDS):
        for label, r, over_clipped in ratekit.rules_in_turn(RULES, lambda rule, pin: dict(
                ratekit.timed_steps(rows, cols, args.steps, args.calls, boundary=rule, kernel=pin), boundary=rule)):
            ok = ok and r["proof"]
            report.table(f"| {rows} x {cols} | {label} | {r['kernel']} | {r['rate']:.0f} | {over_clipped:.3f} | "
                         f"{r['replay_steps']} steps: {'identical' if r['proof'] else 'DIFFERS'} |")
            report.row(r)
    if not args.no_ensemble:
        e = ratekit.ensemble_against_sequential(512, 64, 128, args.steps, args.calls, args.sample, boundary=2)
        ok = ok and e["bitcheck"]
        report.table("", "| periodic ensemble | kernel | ensemble Mcells x steps / s | sequential Mcells x steps / s | speed-up | bit-check |",
                     "|---|---|---|---|---|---|")
        report.table(f"| 512 x 64x128 | {e['kernel']} | {e['ensemble_rate']:.0f} | {e['sequential_rate']:.0f} ({e['sequential_kernel']}) | "
                     f"{e['speedup']:.1f}x | member {e['bitcheck_member']}: {'identical' if e['bitcheck'] else 'DIFFERS'} |")
        report.row(e)
    report.finish()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
