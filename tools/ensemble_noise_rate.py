"""What noise costs an ensemble (``gs_members_set_noise``), and what an ensemble saves over realisations run one by one.

For every row (members x grid under a boundary rule; by default 512 members of 64 x 128 under the zero-halo rule, the resident
form with 8 cells per thread, the same under the clipped rule, whose members of that size run the windowed form, and 64
members of 256 x 512, the windowed form), in ONE process and timed with device events in turn, so that all see the same
chip state:

  plain       the ensemble without noise;
  zero        the same ensemble with noise attached and all sigmas zero: the noise kernels, no draw;
  noisy       the same ensemble with every member drawing for both species, a seed per member;
  sequential  ``--sample`` of the same members run one after another as lone Species with ``Simulation.set_noise`` on the same
              context (the marching kernel's noise form), scaled to the member count.

Each is a median of ``--calls`` calls of ``--steps`` steps after a warm-up call.  One noisy member is compared bit for bit
with its lone Species.  ``--against ROOT`` times the plain ensemble on this tree and on another built checkout (the parent
commit, say) in alternating fresh processes: the difference between the trees beside the run-to-run spread of either.

    python tools/ensemble_noise_rate.py [--rows 512x64x128:1,512x64x128,64x256x512] [--against ROOT] [--json out.json] [--md out.md]

A row is MEMBERSxROWSxCOLS[:RULE], RULE the gs_boundary value (0 clipped, the default; 1 zero halo; 2 periodic; 3 zero flux).

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

from ratekit import ROOT, Report, device_ms, ensemble_subject, medians

ROWS = [(512, 64, 128, 1), (512, 64, 128, 0), (64, 256, 512, 0)]  # members, rows, cols, gs_boundary
RULE_NAMES = ["clipped", "zero halo", "periodic", "zero flux"]
SIGMAS = (0.02, 0.01)
CHILD_TIMEOUT = 240  # seconds per child process of --against


def parse_row(text):
    size, _, rule = text.partition(":")
    row = tuple(int(x) for x in size.split("x")) + (int(rule or 0),)
    if len(row) != 4 or min(row[:3]) < 1 or not 0 <= row[3] <= 3:
        raise ValueError(f"not a row (MEMBERSxROWSxCOLS[:RULE]): {text!r}")
    return row


def measure(members, rows, cols, boundary, steps, calls, sample, plain_only=False):
    import numpy as np

    from ensemble_rate import member_params

    params = member_params(members)
    seeds = np.arange(members, dtype=np.uint64) + np.uint64(1000)
    with ensemble_subject(members, rows, cols, params, boundary=boundary) as (sim, ctx, plain):
        work = members * rows * cols * steps
        out = {"members": members, "rows": rows, "cols": cols, "boundary": boundary, "steps_per_call": steps, "calls": calls}
        if plain_only:
            plain.perform_steps(steps)
            times = [device_ms(ctx, lambda: plain.prepare_steps(steps)) for _ in range(calls)]
            ctx.sync()
            out.update(kernel=ctx.info()[0], ms=statistics.median(times), ms_all=times)
            return out
        zero, noisy = sim.make_ensemble((rows, cols), params), sim.make_ensemble((rows, cols), params)
        try:
            zero.set_noise(0.0, 0.0, seed=seeds)
            noisy.set_noise(SIGMAS[0], SIGMAS[1], seed=seeds)
            subjects = {"plain": plain, "zero": zero, "noisy": noisy}
            kernels = {}
            for name, ens in subjects.items():  # the warm-up call of each, which also names its kernel
                ens.perform_steps(steps)
                kernels[name] = ctx.info()[0]
            ms = medians(ctx, {name: (lambda e=ens: e.perform_steps(steps)) for name, ens in subjects.items()}, calls, warm=False)
            for name in subjects:
                out[name] = {"kernel": kernels[name], "ms": ms[name], "rate": work / (ms[name] * 1e3)}
            # the same members one after another: lone Species with the member's parameters and noise
            idx = sorted({int(round(i * (members - 1) / max(1, sample - 1))) for i in range(sample)})
            solo = [sim.make_species((rows, cols)) for _ in idx]
            done = {i: 0 for i in idx}
            try:
                def members_in_turn():
                    for j, i in enumerate(idx):
                        ctx.set_params(params[i])
                        sim.set_noise(SIGMAS[0], SIGMAS[1], seed=int(seeds[i]), step=done[i])
                        sim.prepare_steps(solo[j], steps)
                        done[i] += steps
                    ctx.sync()

                seq, solo_kernel = [], None
                for call in range(calls + 1):  # the first call of every member is its warm-up
                    t = device_ms(ctx, members_in_turn)
                    if call:
                        seq.append(t)
                    solo_kernel = ctx.info()[0]
                j = len(idx) // 2
                ref_u, ref_v = (p.make_scalar_view(ctx) for p in solo[j].in_out()[:2])
                sim.clear_noise()
                # the bit-check: a fresh noisy ensemble member after as many steps as its lone Species took
                check = sim.make_ensemble((rows, cols), [params[idx[j]]])
                try:
                    check.set_noise(SIGMAS[0], SIGMAS[1], seed=int(seeds[idx[j]]))
                    check.perform_steps(done[idx[j]])
                    same = bool(check.u_views()[0].tobytes() == ref_u.tobytes() and check.result_views()[0].tobytes() == ref_v.tobytes())
                finally:
                    check.destroy()
            finally:
                for s in solo:
                    for plane in s.in_out():
                        plane.destroy()
            seq_ms = statistics.median(seq) / len(idx) * members
            out["sequential"] = {"kernel": solo_kernel, "sampled": len(idx), "ms": seq_ms, "rate": work / (seq_ms * 1e3)}
            out.update(bitcheck_member=idx[j], bitcheck_steps=done[idx[j]], bitcheck=same)
        finally:
            zero.destroy()
            noisy.destroy()
    return out


def run_child(root, row, steps, calls):
    """The plain ensemble of ``row`` in a fresh process on the tree at ``root`` under its own time limit -> its record."""
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child",
           "x".join(str(x) for x in row[:3]) + f":{row[3]}", "--steps", str(steps), "--calls", str(calls)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, GS_NOISE_RATE_ROOT=root), cwd=root)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"the plain ensemble on {root}: exit status {r.returncode}; stopping")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", default=None, help="comma-separated MEMBERSxROWSxCOLS[:RULE] (default: 512x64x128:1,512x64x128,64x256x512)")
    ap.add_argument("--steps", type=int, default=256, help="steps per call")
    ap.add_argument("--calls", type=int, default=5, help="timed calls per measurement")
    ap.add_argument("--sample", type=int, default=8, help="members run one after another as lone Species")
    ap.add_argument("--against", default=None, metavar="ROOT", help="another built checkout to time the plain ensemble on")
    ap.add_argument("--pairs", type=int, default=3, help="process pairs per row of the comparison with --against")
    ap.add_argument("--json", default=None, help="also write the records as a JSON list")
    ap.add_argument("--md", default=None, help="also write the tables as markdown")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.child:  # (the tree to measure comes first on the path: its grayscott_amd, its tools)
        root = os.environ.get("GS_NOISE_RATE_ROOT", ROOT)
        sys.path[:0] = [root, os.path.join(root, "tools")]
        print(json.dumps(measure(*parse_row(args.child), args.steps, args.calls, 0, plain_only=True)))
        return 0
    import torch  # noqa: F401  (the process's HIP runtime is torch's, as in bench.py and the tests)

    rows = ROWS if not args.rows else [parse_row(r) for r in args.rows.split(",")]
    report = Report(args.json, args.md)
    report.table("| members x grid | run | kernel | ms per call | Mcell-steps/s | vs plain |", "|---|---|---|---|---|---|")
    for m, r, c, rule in rows:
        rec = report.row(measure(m, r, c, rule, args.steps, args.calls, args.sample))
        for name in ("plain", "zero", "noisy", "sequential"):
            x = rec[name]
            label = name if name != "sequential" else f"sequential ({x['sampled']} sampled)"
            report.table(f"| {m} x {r}x{c}, {RULE_NAMES[rule]} | {label} | {x['kernel']} | {x['ms']:.3f} | {x['rate']:.0f} | {x['ms'] / rec['plain']['ms']:.2f} |")
        report.table(f"| {m} x {r}x{c}, {RULE_NAMES[rule]} | noisy member {rec['bitcheck_member']} against its lone Species after {rec['bitcheck_steps']} steps | "
                     f"{'bit for bit' if rec['bitcheck'] else 'DIFFERS'} | | | |")
        if not rec["bitcheck"]:
            report.finish()
            raise SystemExit("a noisy member differs from its lone Species; stopping")
    if args.against:
        report.table("", "| members x grid | tree | ms per call, plain ensemble (median per process) | median | spread |", "|---|---|---|---|---|")
        for row in rows:
            got = {"this": [], "other": []}
            for _ in range(args.pairs):
                for name, root in (("this", ROOT), ("other", os.path.abspath(args.against))):
                    got[name].append(report.row(dict(run_child(root, row, args.steps, args.calls), tree=name))["ms"])
            label = f"{row[0]} x {row[1]}x{row[2]}, {RULE_NAMES[row[3]]}"
            for name in ("this", "other"):
                v = got[name]
                report.table(f"| {label} | {name} | {', '.join(f'{x:.3f}' for x in v)} | {statistics.median(v):.3f} | "
                             f"{(max(v) - min(v)) / statistics.median(v) * 100:.2f} % |")
            d = statistics.median(got["this"]) / statistics.median(got["other"]) - 1
            report.table(f"| {label} | this / other - 1 | | {d * 100:+.2f} % | |")
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
