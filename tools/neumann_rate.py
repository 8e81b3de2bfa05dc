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
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

GRIDS = [(16384, 16384, 1), (4096, 4096, 1), (1080, 1920, 1), (512, 1024, 1), (16384, 16384, 2)]  # rows, cols, slabs
RULES = [("clipped", 0), ("zero flux", 3)]


def time_grid(rows, cols, boundary, steps, calls, kernel=0, slabs=1):
    import numpy as np

    from grayscott_amd import HipArgs, Parameters, Simulation, capi

    devices = [0] * slabs
    sim = Simulation.new(Parameters(), HipArgs(devices=devices, boundary=boundary, kernel=kernel))
    ctx = sim.context
    species = sim.make_species((rows, cols))
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
    iu, iv, _, _ = species.in_out()
    got_u, got_v = iu.make_scalar_view(ctx), iv.make_scalar_view(ctx)
    for c in species.in_out():
        c.destroy()
    ctx.close()
    # the proof: the same steps on the same slabs, one gs_step of the cross-check kernel at a time
    ref = Simulation.new(Parameters(), HipArgs(devices=devices, boundary=boundary, kernel=capi.GS_KERNEL_SIMPLE))
    rs = ref.make_species((rows, cols))
    for _ in range(total):
        ref.perform_step(rs)
    ru, rv, _, _ = rs.in_out()
    ref_u, ref_v = ru.make_scalar_view(ref.context), rv.make_scalar_view(ref.context)
    replay = ref.context.info()[0]
    for c in rs.in_out():
        c.destroy()
    ref.context.close()
    ms = statistics.median(times)
    return {"rows": rows, "cols": cols, "slabs": slabs, "boundary": boundary, "steps_per_call": steps, "calls": calls,
            "warmup_calls": warm, "kernel": kernel_name,
            "ms": ms, "ms_all": times, "rate": rows * cols * steps / (ms * 1e3), "replay_kernel": replay, "replay_steps": total,
            "proof": bool(got_u.tobytes() == ref_u.tobytes() and got_v.tobytes() == ref_v.tobytes()),
            "sum_v": float(np.sum(got_v, dtype=np.float64))}


def time_ensemble(members, rows, cols, steps, calls, sample, boundary):
    import numpy as np

    from ensemble_rate import member_params
    from grayscott_amd import HipArgs, Simulation

    params = member_params(members)
    sim = Simulation.new(params[0], HipArgs(devices=[0], boundary=boundary))
    ctx = sim.context
    ens = sim.make_ensemble((rows, cols), params)
    ens.perform_steps(steps)
    times = []
    for _ in range(calls):
        ctx.timer_start()
        ens.prepare_steps(steps)
        times.append(ctx.timer_stop())
    ctx.sync()
    kernel = ctx.info()[0]
    idx = sorted({int(round(i * (members - 1) / max(1, sample - 1))) for i in range(sample)})
    solo = [sim.make_species((rows, cols)) for _ in idx]
    seq, solo_kernel = [], None
    for call in range(calls + 1):  # the first call of every member is its warm-up
        ctx.timer_start()
        for j, i in enumerate(idx):
            ctx.set_params(params[i])
            sim.prepare_steps(solo[j], steps)
        ms = ctx.timer_stop()
        if call:
            seq.append(ms)
        solo_kernel = ctx.info()[0]
    ctx.sync()
    j = len(idx) // 2
    got, ref = ens.result_views(idx[j], 1)[0], solo[j].make_result_view()
    out = {"members": members, "rows": rows, "cols": cols, "boundary": boundary, "kernel": kernel,
           "sequential_kernel": solo_kernel,
           "ensemble_rate": members * rows * cols * steps / (statistics.median(times) * 1e3),
           "sequential_rate": rows * cols * steps / (statistics.median(seq) / len(idx) * 1e3),
           "bitcheck_member": idx[j], "bitcheck": bool(got.tobytes() == ref.tobytes())}
    out["speedup"] = out["ensemble_rate"] / out["sequential_rate"]
    for s in solo:
        for c in s.in_out():
            c.destroy()
    ens.destroy()
    ctx.close()
    return out


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
    grids = GRIDS
    if args.grids:
        grids = [tuple(int(x) for x in g.split("x")) for g in args.grids.split(",")]
        grids = [g if len(g) == 3 else g + (1,) for g in grids]
    lines = ["| grid | rule | kernel | Mcells x steps / s | / clipped | replay (simple kernel) |", "|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    ok = True

    def emit(line, rec):
        lines.append(line)
        print(line, flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(json.dumps(rec) + "\n")

    for rows, cols, slabs in grids:
        base = None
        todo = [(label, rule, 0) for label, rule in RULES]  # (label, gs_boundary, pinned gs_kernel)
        i = 0
        while i < len(todo):
            label, rule, pin = todo[i]
            i += 1
            r = time_grid(rows, cols, rule, args.steps, args.calls, kernel=pin, slabs=slabs)
            base = r["rate"] if (rule == 0 and pin == 0) else base
            if rule == 0 and pin == 0 and not r["kernel"].startswith("tb-"):
                todo.insert(i, ("clipped, kernel = TB", 0, 3))
            ok = ok and r["proof"]
            grid = f"{rows} x {cols}" + (f", {slabs} slabs" if slabs > 1 else "")
            emit(f"| {grid} | {label} | {r['kernel']} | {r['rate']:.0f} | {r['rate'] / base:.3f} | "
                 f"{r['replay_steps']} steps: {'identical' if r['proof'] else 'DIFFERS'} |", r)
    if not args.no_ensemble:
        lines += ["", "| ensemble | rule | kernel | ensemble Mcells x steps / s | sequential Mcells x steps / s | speed-up | bit-check |",
                  "|---|---|---|---|---|---|---|"]
        print("\n".join(lines[-3:]), flush=True)
        for label, rule in RULES:
            e = time_ensemble(512, 64, 128, args.steps, args.calls, args.sample, rule)
            ok = ok and e["bitcheck"]
            emit(f"| 512 x 64x128 | {label} | {e['kernel']} | {e['ensemble_rate']:.0f} | {e['sequential_rate']:.0f} "
                 f"({e['sequential_kernel']}) | {e['speedup']:.1f}x | member {e['bitcheck_member']}: "
                 f"{'identical' if e['bitcheck'] else 'DIFFERS'} |", e)
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
