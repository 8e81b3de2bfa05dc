"""Rates of the noise term (gs_ctx_set_noise) against the uniform and the mapped run, in one process.

For every grid (16384^2, 4096^2, 1080 x 1920): a Species seeded with Species::new's pattern, timed as
tools/param_map_rate.py times it -- warm-up calls until the on-line tuner has settled (at most 40), then ``--calls`` calls
of ``--steps`` steps timed with device events around each call (median) -- five times, one after the other in the same
process: the noise form with both sigmas set, with one sigma set, with both sigmas zero (the noise kernels without a draw:
the cost of the form itself), the uniform run (kernel = AUTO, and kernel = TB where AUTO runs another kernel) and the
mapped run (a Munafo map: the other unshared 4-wave form of the marching kernel).  The result with both sigmas set is
proven: a second context replays the same number of steps from the same initial state, seed and start step with the
noise form of the cross-check kernel (GS_KERNEL_SIMPLE, one gs_step per step), and U and V must be bit for bit the same.
The page also records the registers of the noise marching kernel's entry and the waves per SIMD they allow.

    python tools/noise_rate.py [--grids 16384x16384,1080x1920] [--steps 256] [--calls 5] [--md profiles/noise_rates.md]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402
from param_map_rate import munafo  # noqa: E402

GRIDS = "16384x16384,4096x4096,1080x1920"
SIGMA, SEED = 0.01, 20240229


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--grids", default=GRIDS, help="comma-separated ROWSxCOLS")
    ap.add_argument("--steps", type=int, default=256, help="steps per timed call")
    ap.add_argument("--calls", type=int, default=5, help="timed calls per grid and form (median)")
    ap.add_argument("--no-proof", action="store_true", help="skip the replay with the cross-check kernel")
    ap.add_argument("--md", default=None, help="also write the table to this file")
    ap.add_argument("--json", default=None, help="append one JSON line per measurement to this file")
    args = ap.parse_args(argv)
    import codeobj

    kernels = {k.name: k for k in codeobj.kernels()}
    report = ratekit.Report(args.json, args.md, json_lines=True)
    report.table("| grid | uniform: kernel | Mcells x steps / s | mapped | noise, sigmas 0 | noise, one sigma | noise, both sigmas: kernel | "
                 "Mcells x steps / s | both / uniform | both / mapped | VGPRs | waves per SIMD | replay (noise simple kernel) |",
                 "|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    ok = True
    for rows, cols in ratekit.parse_grids(args.grids):
        fmap = munafo(rows, cols)
        forms = {"uniform": None,
                 "mapped": lambda sim: sim.set_param_map(*fmap),
                 "zero": lambda sim: sim.set_noise(0.0, 0.0, seed=SEED),
                 "one": lambda sim: sim.set_noise(SIGMA, 0.0, seed=SEED),
                 "both": lambda sim: sim.set_noise(SIGMA, SIGMA, seed=SEED)}
        recs = {}
        for form, attach in forms.items():
            r = ratekit.timed_steps(rows, cols, args.steps, args.calls, attach=attach, prove=form == "both" and not args.no_proof)
            recs[form] = dict(r, form=form)
            if form == "uniform" and not r["kernel"].startswith("tb-"):   # the marching kernel's own uniform rate beside it
                recs["uniform-tb"] = dict(ratekit.timed_steps(rows, cols, args.steps, args.calls, kernel=3, prove=False), form="uniform-tb")
        uni, both = recs["uniform"], recs["both"]
        ok = ok and both.get("proof", True)
        entry, vgpr, waves = ratekit.registers(kernels, both["kernel"], "noise")
        proof = "not run" if "proof" not in both else f"{both['replay_steps']} steps: {'identical' if both['proof'] else 'DIFFERS'}"
        uni_text = f"{uni['kernel']} | {uni['rate']:.0f}"
        if "uniform-tb" in recs:
            uni_text = f"{uni['kernel']} ({recs['uniform-tb']['kernel']}: {recs['uniform-tb']['rate']:.0f}) | {uni['rate']:.0f}"
        report.table(f"| {rows} x {cols} | {uni_text} | {recs['mapped']['rate']:.0f} | {recs['zero']['rate']:.0f} | "
                     f"{recs['one']['rate']:.0f} | {both['kernel']} | {both['rate']:.0f} | {both['rate'] / uni['rate']:.3f} | "
                     f"{both['rate'] / recs['mapped']['rate']:.3f} | {vgpr} | {waves} | {proof} |")
        for r in recs.values():
            report.row(dict(r, entry=entry, vgpr=vgpr, waves_per_simd=waves))
    report.finish()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
