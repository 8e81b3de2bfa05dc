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
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

GRIDS = [(16384, 16384, 1), (4096, 4096, 1), (1080, 1920, 1), (512, 1024, 1), (16384, 16384, 2)]  # rows, cols, slabs


def maze(rows, cols):
    import numpy as np

    from tests.mask_ref import maze

    return maze((rows, cols), np.random.default_rng(0))


def time_grid(rows, cols, steps, calls, masked, kernel=0, slabs=1, prove=True):
    import numpy as np

    from grayscott_amd import HipArgs, Parameters, Simulation, capi

    devices = [0] * slabs
    walls = maze(rows, cols) if masked else None
    sim = Simulation.new(Parameters(), HipArgs(devices=devices, kernel=kernel))
    ctx = sim.context
    species = sim.make_species((rows, cols))
    if masked:
        sim.set_mask(walls)
    warm = 0
    while True:  # warm-up: until the on-line tuner has settled on the marching kernel's configuration
        sim.perform_steps(species, steps)
        warm += 1
        name = ctx.info()[0]
        if warm >= 40 or not name.startswith("tb-") or "@" in name:
            break
    times = []
    for _ in range(calls):
        ctx.timer_start()
        sim.prepare_steps(species, steps)
        times.append(ctx.timer_stop())
    ctx.sync()
    kernel_name = ctx.info()[0]
    total = steps * (calls + warm)
    out = {"rows": rows, "cols": cols, "slabs": slabs, "masked": masked, "pinned_kernel": kernel, "steps_per_call": steps,
           "calls": calls, "warmup_calls": warm, "kernel": kernel_name, "ms": statistics.median(times), "ms_all": times}
    out["rate"] = rows * cols * steps / (out["ms"] * 1e3)
    if prove:
        iu, iv, _, _ = species.in_out()
        got_u, got_v = iu.make_scalar_view(ctx), iv.make_scalar_view(ctx)
    for c in species.in_out():
        c.destroy()
    ctx.close()
    if not prove:
        return out
    # the proof: the same steps on the same slabs, one gs_step of the (masked) cross-check kernel at a time
    ref = Simulation.new(Parameters(), HipArgs(devices=devices, kernel=capi.GS_KERNEL_SIMPLE))
    rs = ref.make_species((rows, cols))
    if masked:
        ref.set_mask(walls)
    for _ in range(total):
        ref.perform_step(rs)
    ru, rv, _, _ = rs.in_out()
    ref_u, ref_v = ru.make_scalar_view(ref.context), rv.make_scalar_view(ref.context)
    out.update(replay_kernel=ref.context.info()[0], replay_steps=total,
               proof=bool(got_u.tobytes() == ref_u.tobytes() and got_v.tobytes() == ref_v.tobytes()),
               sum_v=float(np.sum(got_v, dtype=np.float64)))
    for c in rs.in_out():
        c.destroy()
    ref.context.close()
    return out


def entry_of(name):
    """The kernel instance behind a reported name of the marching kernel's mask form, e.g. tb-k4c2/strict.op/mask@.. ->
    gs_step_tb_wk_strict<4, 3, 2, 0>."""
    m = re.match(r"tb-k(\d)(c\d)?/(strict|fused)(\.op)?(/periodic|/neumann)?/mask", name)
    if not m:
        return None
    k, c, flavour, op, rule = m.groups()
    cpl = int(c[1:]) if c else 4
    return f"gs_step_tb_wk_{flavour}<{k}, {3 if op else 0}, {cpl}, {RULE_SET.get(rule, 0)}>"


RULE_SET = {"/periodic": 1, "/neumann": 2}


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
    grids = GRIDS
    if args.grids:
        grids = [tuple(int(x) for x in g.split("x")) for g in args.grids.split(",")]
        grids = [g if len(g) == 3 else g + (1,) for g in grids]
    lines = ["| grid | no mask: kernel | Mcells x steps / s | masked: kernel | Mcells x steps / s | masked / no mask | "
             "masked streaming kernel | marching / streaming | VGPRs | waves per SIMD | replay (masked simple kernel) |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    ok = True
    for rows, cols, slabs in grids:
        recs = [time_grid(rows, cols, args.steps, args.calls, False, slabs=slabs, prove=False),
                time_grid(rows, cols, args.steps, args.calls, True, slabs=slabs),
                time_grid(rows, cols, max(16, args.steps // 4), args.calls, True, kernel=2, slabs=slabs, prove=False)]
        uni, mp, st = recs
        ok = ok and mp["proof"]
        entry = entry_of(mp["kernel"].split("@")[0])
        k = kernels.get(entry) if entry else None
        vgpr = k.vgpr if k else None
        waves = min(8, 512 // (((vgpr + 7) // 8) * 8)) if vgpr else None
        grid = f"{rows} x {cols}" + (f", {slabs} slabs" if slabs > 1 else "")
        line = (f"| {grid} | {uni['kernel']} | {uni['rate']:.0f} | {mp['kernel']} | {mp['rate']:.0f} | "
                f"{mp['rate'] / uni['rate']:.3f} | {st['kernel']}: {st['rate']:.0f} | {mp['rate'] / st['rate']:.2f}x | "
                f"{vgpr} | {waves} | {mp['replay_steps']} steps: {'identical' if mp['proof'] else 'DIFFERS'} |")
        lines.append(line)
        print(line, flush=True)
        if args.json:
            with open(args.json, "a") as f:
                for r in recs:
                    f.write(json.dumps(dict(r, entry=entry, vgpr=vgpr, waves_per_simd=waves)) + "\n")
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
