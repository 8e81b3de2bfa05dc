"""Time of a components call (gs_fields_components, gs_members_components) against two things beside it, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and each of three inputs -- ``new`` (Species::new untouched),
``developed`` (uniform random planes after steps: a spot pattern) and ``random`` (cells set with probability 0.59, the
4-connected percolation regime: the worst case for union-find) -- the connected components of V at ONE threshold are timed
under connectivity 8 and under 4, in turn with

* ``gs_fields_morphology`` with one threshold on the same plane: the one-pass floor of reading the plane;
* a download of the plane plus ``scipy.ndimage.label`` and a ``bincount`` of the sizes, where scipy is present: what a user
  does without the call (``--label-calls`` times, default 1: it takes seconds at 16384^2).

The calls block and the components call allocates and frees its label memory inside, so every figure is the wall time of the
call (``time.perf_counter`` around it, after a warm-up call; medians of ``--calls``); the time between device events on the
compute stream is given beside it for the two device calls.  The same for an ensemble of 512 members of 64 x 128
(gs_members_components against gs_members_morphology; the download is of both species of all members).

    python tools/components_rate.py [--calls 9] [--label-calls 1] [--grids 16384x16384,4096x4096,1080x1920] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = "16384x16384,4096x4096,1080x1920"
ENSEMBLE = (512, 64, 128)  # members, rows, cols
KINDS = ("new", "developed", "random")
TV, TU = 0.25, 0.5
DENSITY = 0.59


def _label():
    try:
        from scipy import ndimage
    except ImportError:
        return None
    return ndimage


def _both(ctx, fn):
    """(wall ms, device-event ms) of one blocking call."""
    ctx.timer_start()
    t0 = time.perf_counter()
    fn()
    wall = (time.perf_counter() - t0) * 1e3
    return wall, ctx.timer_stop()


def _wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _medians(ctx, fns, calls):
    """{name: (wall ms, event ms)}: the calls timed in turn after one warm-up call each."""
    for fn in fns.values():
        fn()
    got = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            got[k].append(_both(ctx, fn))
    return {k: (statistics.median(w for w, _ in v), statistics.median(e for _, e in v)) for k, v in got.items()}


def _fill(sim, species, kind, rows, cols):
    """Bring `species` (fresh from make_species) into the state `kind`."""
    if kind == "new":
        return
    rng = np.random.default_rng(3)
    in_u, in_v, _, _ = species.in_out()
    if kind == "random":
        v = np.where(rng.random((rows, cols), dtype=np.float32) < np.float32(DENSITY), np.float32(0.5), np.float32(0.0))
        in_v.upload(sim.context, v.astype(np.float32))
        return
    u = rng.random((rows, cols), dtype=np.float32)
    in_u.upload(sim.context, u)
    u *= np.float32(0.5)
    in_v.upload(sim.context, u)
    sim.perform_steps(species, 64)


def _host_label(ndimage, plane, threshold, structure):
    labels, n = ndimage.label(plane > np.float32(threshold), structure)
    sizes = np.bincount(labels.ravel())[1:]
    return n, int(sizes.max()) if n else 0


def time_species(rows, cols, kind, calls, label_calls):
    from grayscott_amd import HipArgs, Parameters, Simulation

    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    species = sim.make_species((rows, cols))
    _fill(sim, species, kind, rows, cols)
    _, in_v, _, _ = species.in_out()
    c8 = in_v.components(ctx, [TV], True, 8)[0]
    m = _medians(ctx, {"c8": lambda: in_v.components(ctx, [TV], True, 8), "c4": lambda: in_v.components(ctx, [TV], True, 4),
                       "morph": lambda: in_v.morphology(ctx, [TV])}, calls)
    out = {"grid": f"{rows}x{cols}", "input": kind, "cells": rows * cols, "components8_ms": m["c8"][0], "components4_ms": m["c4"][0],
           "morphology_ms": m["morph"][0], "components8_event_ms": m["c8"][1], "components4_event_ms": m["c4"][1],
           "morphology_event_ms": m["morph"][1], "components": c8.count, "largest_fraction": c8.largest_fraction,
           "label_memory_bytes": 8 * rows * cols, "download_label_ms": None}
    ndimage = _label()
    if ndimage is not None and label_calls > 0:
        eight = ndimage.generate_binary_structure(2, 2)
        got = []
        out["download_label_ms"] = statistics.median(
            _wall(lambda: got.append(_host_label(ndimage, in_v.make_scalar_view(ctx), TV, eight))) for _ in range(label_calls))
        if got[-1] != (c8.count, c8.largest):
            raise RuntimeError(f"{out['grid']} {kind}: the device counts {(c8.count, c8.largest)}, scipy {got[-1]}")
    ctx.close()
    return out


def time_ensemble(members, rows, cols, calls, label_calls):
    from grayscott_amd import HipArgs, Parameters, Simulation

    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    ens = sim.make_ensemble((rows, cols), Parameters(), members=members)
    ens.perform_steps(16)
    m = _medians(ctx, {"c8": lambda: ens.components(v_thresholds=[TV], u_thresholds=[TU], connectivity=8),
                       "c4": lambda: ens.components(v_thresholds=[TV], u_thresholds=[TU], connectivity=4),
                       "morph": lambda: ens.morphologies(v_thresholds=[TV], u_thresholds=[TU])}, calls)
    out = {"grid": f"{members} x {rows}x{cols}", "input": "new + 16 steps, U and V", "cells": 2 * members * rows * cols,
           "components8_ms": m["c8"][0], "components4_ms": m["c4"][0], "morphology_ms": m["morph"][0],
           "components8_event_ms": m["c8"][1], "components4_event_ms": m["c4"][1], "morphology_event_ms": m["morph"][1],
           "components": None, "largest_fraction": None, "label_memory_bytes": 8 * members * rows * cols, "download_label_ms": None}
    ndimage = _label()
    if ndimage is not None and label_calls > 0:
        eight = ndimage.generate_binary_structure(2, 2)

        def host():
            u, v = ens.u_views(), ens.result_views()
            for i in range(members):
                _host_label(ndimage, -u[i], -TU, eight)
                _host_label(ndimage, v[i], TV, eight)

        out["download_label_ms"] = statistics.median(_wall(host) for _ in range(label_calls))
    ens.destroy()
    ctx.close()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--label-calls", type=int, default=1, help="timed runs of the download + scipy.ndimage.label (0: none)")
    ap.add_argument("--grids", default=GRIDS)
    ap.add_argument("--no-ensemble", action="store_true")
    ap.add_argument("--json", default=None, help="also write the rows as a JSON list")
    ap.add_argument("--md", default=None, help="also write the table as markdown")
    args = ap.parse_args(argv)
    import torch  # noqa: F401  (the process's HIP runtime is torch's, as in bench.py and the tests)

    rows = []
    for grid in [g for g in args.grids.split(",") if g]:
        r, c = (int(x) for x in grid.split("x"))
        for kind in KINDS:
            rows.append(time_species(r, c, kind, args.calls, args.label_calls))
            print(json.dumps(rows[-1]), flush=True)
    if not args.no_ensemble:
        rows.append(time_ensemble(*ENSEMBLE, args.calls, args.label_calls))
        print(json.dumps(rows[-1]), flush=True)
    for r in rows:
        r["components8_over_morphology"] = r["components8_ms"] / r["morphology_ms"]
        r["label_over_components8"] = r["download_label_ms"] / r["components8_ms"] if r["download_label_ms"] else None
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    lines = ["| grid | input | components | components, 8 (ms) | components, 4 (ms) | morphology (ms) | 8 / morphology | "
             "download + label (ms) | label / components |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        label = f"{r['download_label_ms']:.1f}" if r["download_label_ms"] else "-"
        ratio = f"{r['label_over_components8']:.1f}" if r["label_over_components8"] else "-"
        lines.append(f"| {r['grid']} | {r['input']} | {r['components'] if r['components'] is not None else '-'} | "
                     f"{r['components8_ms']:.3f} | {r['components4_ms']:.3f} | {r['morphology_ms']:.3f} | "
                     f"{r['components8_over_morphology']:.1f} | {label} | {ratio} |")
    print("\n".join(lines))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
