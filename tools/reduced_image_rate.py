"""What a reduced result image (gs_field_download_reduced_async) costs and what it buys, in one process.

Three measurements, each printed as a markdown table (and, with --json, written as one JSON document):

    staging   device time (gs_timer_start / gs_timer_stop: HIP events on the compute stream) of the staging kernel of one
              overlapped image -- gs_pack_rows_k for factor 1, the reduction kernels for 2, 4, 8, 16 (and what --factors
              adds) -- at 16384 x 16384 and 1080 x 1920; the previous image has left its staging buffer before the clock
              starts.  Median, minimum and maximum of --calls calls per point, the factors taken in turn within every
              round so that all of them see the same minutes of the machine.  The plane-read rate is 4 bytes per cell
              over that time.
    pattern   tools/call_pattern.py's case (c) at 1080 x 1920: calls of 32 steps with an overlapped V image each, two images
              in flight, at factors 1, 2, 4, 8, next to the same calls with no image at all.  Mcells x steps / s, median of 3
              runs of --pattern-calls calls.
    large     python -m grayscott_amd.simulate -r 16384 -c 16384 -e 32 -n 20 to a .npy target with --hip-image-reduce 8 and
              16 (and 1 with --large-full: a 20 GiB file), against prepare_steps alone for the same number of steps.

    python tools/reduced_image_rate.py [--only staging,pattern,large] [--calls 20] [--json FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def staging(calls, factors, grids):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from grayscott_amd.simulation import pinned_empty

    rows_out = []
    for rows, cols in grids:
        sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
        ctx = sim.context
        species = sim.make_species((rows, cols))
        sim.perform_steps(species, 16)
        v = species.in_out()[1]
        images = {f: pinned_empty(v.reduced_shape(f)) for f in factors}

        def one(f):
            ctx.download_wait()                     # both staging buffers are free, nothing else runs
            ctx.sync()
            ctx.timer_start()
            v.write_scalar_view_after(ctx, images[f], reduce=f)
            ms = ctx.timer_stop()
            ctx.download_wait()
            return ms

        for f in factors:                           # first launches: code object load, staging buffers allocated
            one(f)
            one(f)
        times = {f: [] for f in factors}
        for _ in range(calls):
            for f in factors:
                times[f].append(one(f))
        for f in factors:
            t = times[f]
            med = statistics.median(t)
            rows_out.append({"grid": f"{rows}x{cols}", "factor": f, "kernel": "gs_pack_rows_k" if f == 1 else
                             ("gs_reduce_vec_k" if f in (2, 4) else "gs_reduce_lds_k"), "median_ms": med, "min_ms": min(t),
                             "max_ms": max(t), "read_tb_per_s": 4.0 * rows * cols / (med * 1e-3) / 1e12, "calls": len(t)})
        ctx.close()
    print("| grid | factor | staging kernel | device time, median (ms) | min - max (ms) | plane reads (TB/s) | against factor 1 |")
    print("|---|---|---|---|---|---|---|")
    for r in rows_out:
        base = next(b for b in rows_out if b["grid"] == r["grid"] and b["factor"] == 1) if 1 in factors else None
        rel = f"{r['median_ms'] / base['median_ms']:.2f}" if base else "-"
        print(f"| {r['grid']} | {r['factor']} | `{r['kernel']}` | {r['median_ms']:.4f} | {r['min_ms']:.4f} - {r['max_ms']:.4f} | "
              f"{r['read_tb_per_s']:.2f} | {rel} |", flush=True)
    return rows_out


def pattern(calls, factors, rows=1080, cols=1920, n=32):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from grayscott_amd.simulation import pinned_empty

    cells = rows * cols
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    sp = sim.make_species([rows, cols])
    sim.perform_steps(sp, 4000)                     # on-line tuning done
    v_shape = {f: sp.in_out()[1].reduced_shape(f) for f in factors}

    def run(f):
        pinned = [pinned_empty(v_shape[f]) for _ in range(3)] if f else None

        def body():
            for i in range(calls):
                sim.prepare_steps(sp, n)
                if f:
                    sp.write_result_view_after(pinned[i % 3], reduce=f)
                    if i:
                        ctx.download_wait(in_flight=1)
            ctx.download_wait()
            ctx.sync()

        body()
        rates = []
        for _ in range(3):
            ctx.sync()
            t0 = time.perf_counter()
            body()
            rates.append(cells * n * calls / (time.perf_counter() - t0) / 1e6)
        return rates

    out = []
    for f in [0] + list(factors):
        rates = run(f)
        out.append({"factor": f, "median": statistics.median(rates), "min": min(rates), "max": max(rates),
                    "image_bytes": v_shape[f][0] * v_shape[f][1] * 4 if f else 0, "kernel": ctx.info()[0]})
    ctx.close()
    print(f"grid {rows} x {cols}, calls of {n} steps, {calls} calls per run, median of 3 runs; Mcells x steps / s")
    print("| image per call | bytes per image | rate, median | min - max | kernel of the steps |")
    print("|---|---|---|---|---|")
    for r in out:
        what = "none" if r["factor"] == 0 else ("full V plane" if r["factor"] == 1 else f"V reduced by {r['factor']}")
        print(f"| {what} | {r['image_bytes']:,} | {r['median']:,.0f} | {r['min']:,.0f} - {r['max']:,.0f} | `{r['kernel']}` |", flush=True)
    return out


def large(factors, rows=16384, cols=16384, n_images=20, extra=32):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from grayscott_amd import simulate

    cells = rows * cols
    out = []
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    sp = sim.make_species([rows, cols])
    sim.perform_steps(sp, 4 * extra)                # tuned
    t0 = time.perf_counter()
    for _ in range(n_images):
        sim.prepare_steps(sp, extra)
    sim.context.sync()
    dt = time.perf_counter() - t0
    out.append({"factor": 0, "seconds": dt, "rate": cells * extra * n_images / dt / 1e6, "image_bytes": 0})
    sim.context.close()
    with tempfile.TemporaryDirectory() as tmp:
        for f in factors:
            target = os.path.join(tmp, f"reduce{f}.npy")
            args = simulate.parse(["-r", str(rows), "-c", str(cols), "-e", str(extra), "-n", str(n_images), "-o", target,
                                   "--hip-image-reduce", str(f)])
            t0 = time.perf_counter()
            info = simulate.run(args)
            dt = time.perf_counter() - t0
            out.append({"factor": f, "seconds": dt, "loop_seconds": info["seconds"], "rate": cells * extra * n_images / dt / 1e6,
                        "image_bytes": info["image_bytes"]})
            os.remove(target)
    print(f"simulate -r {rows} -c {cols} -e {extra} -n {n_images} to a .npy target; seconds end to end (context, Species and "
          "placement included for the simulate runs; the steps-only line is the timed loop of a tuned context)")
    print("| run | image bytes written | seconds | Mcells x steps / s |")
    print("|---|---|---|---|")
    for r in out:
        what = "prepare_steps only" if r["factor"] == 0 else f"--hip-image-reduce {r['factor']}"
        print(f"| {what} | {r['image_bytes']:,} | {r['seconds']:.2f} | {r['rate']:,.0f} |", flush=True)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", default="staging,pattern,large")
    ap.add_argument("--calls", type=int, default=20, help="timed calls per point of the staging table")
    ap.add_argument("--factors", default="1,2,4,8,16,3,64", help="factors of the staging table")
    ap.add_argument("--pattern-calls", type=int, default=200)
    ap.add_argument("--large-full", action="store_true", help="the large run at factor 1 too (a 20 GiB target)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    import torch  # noqa: F401  (the process's HIP runtime is torch's, as in bench.py and the tests)

    only = args.only.split(",")
    doc = {}
    if "staging" in only:
        doc["staging"] = staging(args.calls, [int(x) for x in args.factors.split(",")], [(16384, 16384), (1080, 1920)])
    if "pattern" in only:
        doc["pattern"] = pattern(args.pattern_calls, [1, 2, 4, 8])
    if "large" in only:
        doc["large"] = large(([1] if args.large_full else []) + [8, 16])
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
