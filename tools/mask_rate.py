"""Rates of domain masks (gs_ctx_set_mask) against a grid without walls, in one process.

For every grid (16384^2, 4096^2, 1080 x 1920, 512 x 1024, and 16384^2 as a chain of 2 slabs on one GPU): a Species seeded
with Species::new's pattern, timed as tools/param_map_rate.py times it -- warm-up calls until the on-line tuner has
settled (at most 40), then ``--calls`` calls of ``--steps`` steps timed with device events around each call (median) --
three times: no mask (kernel = AUTO: the window kernel at 1080 x 1920, the tile kernel at 512 x 1024), a maze of 1-cell
walls over about a quarter of the cells (tests/mask_ref.py: maze; kernel = AUTO, which runs the marching kernel's mask
form at every size) and the same mask on the streaming kernel (kernel = STREAM, one step per pass).  Every masked
result is proven: a second context replays the same number of steps from the same initial state and mask with the
masked cross-check kernel (GS_KERNEL_SIMPLE, one gs_step per step), and U and V must be bit for bit the same.  The page
also records the registers of the masked marching kernel's entry and the waves per SIMD they allow.

    python tools/mask_rate.py [--grids 16384x16384,1080x1920] [--steps 256] [--calls 5] [--md profiles/mask.md]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402

GRIDS = "16384x16384,4096x4096,1080x1920,512x1024,16384x16384x2"  # rows x cols [x slabs]


def maze(rows, cols):
    import numpy as np

    from tests.mask_ref import maze

    return maze((rows, cols), np.random.default_rng(0))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--grids", default=None, help="comma-separated ROWSxCOLS or ROWSxCOLSxSLABS (default: the grids of the table)")
    ap.add_argument("--steps", type=int, default=256, help="steps per timed call")
    ap.add_argument("--calls", type=int, default=5, help="timed calls per grid and form (median)")
    ap.add_argument("--md", default=None, help="also write the table to this file")
    ap.add_argument("--json", default=None, help="append one JSON line per measurement to this file")
    args = ap.parse_args(argv)
    import codeobj

    kernels = {k.name: k for k in codeobj.kernels()}
    report = ratekit.Report(args.json, args.md, json_lines=True)
    report.table("| grid | no mask: kernel | Mcells x steps / s | masked: kernel | Mcells x steps / s | masked / no mask | "
                 "masked streaming kernel | marching / streaming | VGPRs | waves per SIMD | replay (masked simple kernel) |",
                 "|---|---|---|---|---|---|---|---|---|---|---|")
    ok = True
    for rows, cols, slabs in ratekit.parse_grids(args.grids or GRIDS, slabs=True):
        walls = maze(rows, cols)
        attach = lambda sim: sim.set_mask(walls)  # noqa: E731

        def timed(steps, masked, kernel=0, prove=False):
            r = ratekit.timed_steps(rows, cols, steps, args.calls, kernel=kernel, slabs=slabs, attach=attach if masked else None,
                                    prove=prove)
            return dict(r, slabs=slabs, masked=masked, pinned_kernel=kernel)

        recs = [timed(args.steps, False), timed(args.steps, True, prove=True), timed(max(16, args.steps // 4), True, kernel=2)]
        uni, mp, st = recs
        ok = ok and mp["proof"]
        entry, vgpr, waves = ratekit.registers(kernels, mp["kernel"], "mask")
        grid = f"{rows} x {cols}" + (f", {slabs} slabs" if slabs > 1 else "")
        report.table(f"| {grid} | {uni['kernel']} | {uni['rate']:.0f} | {mp['kernel']} | {mp['rate']:.0f} | "
                     f"{mp['rate'] / uni['rate']:.3f} | {st['kernel']}: {st['rate']:.0f} | {mp['rate'] / st['rate']:.2f}x | "
                     f"{vgpr} | {waves} | {mp['replay_steps']} steps: {'identical' if mp['proof'] else 'DIFFERS'} |")
        for r in recs:
            report.row(dict(r, entry=entry, vgpr=vgpr, waves_per_simd=waves))
    report.finish()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
