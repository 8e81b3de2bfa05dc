"""Time of one sample of the time statistics (gs_time_stats_accumulate, gs_members_time_stats_accumulate) beside three things
measured in the same process: a summary of the same planes, a device-to-device copy of exactly the bytes the call moves, and
the host route it replaces.

For every Species grid (16384^2, 4096^2, 1080 x 1920) and for an ensemble of 512 members of 64 x 128, for the group sets
{sum}, {sum, squares}, {extremes} and all four, for V alone and for U + V (an ensemble always samples both): after a few
warm-up steps ``accumulate`` is called ``--calls`` times in turns with the summary and the copy, each timed with device
events, and the medians are reported.  The call reads the sample (4 bytes per cell and plane) and reads and writes every
selected accumulator (2 x 8 for sum and for squares, 2 x (4 + 4) for the extremes and for the crossings): that many bytes
travel, and the copy -- half of them read, half written, one torch ``copy_`` between two device buffers -- is the yardstick:
``accumulate / copy`` is what to judge the kernel by.  The host route is what a user without the feature does per sample:
both planes downloaded and the same accumulators updated in numpy (``--host-calls`` times, default 1; 0 skips it).

    python tools/time_stats_rate.py [--calls 10] [--host-calls 1] [--grids 16384x16384,4096x4096,1080x1920] [--no-ensemble]
                                    [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402
from ratekit import ENSEMBLE  # noqa: E402

GROUP_SETS = (("sum", 1), ("sum+squares", 3), ("extremes", 4), ("all", 15))
HEADER = ["| grid | planes | groups | bytes per cell and plane | accumulate, device (ms) | moved (TB/s) | copy of the same bytes (ms) |"
          " accumulate / copy | summary, device (ms) | host route (ms) |",
          "|---|---|---|---|---|---|---|---|---|---|"]


def bytes_per_cell(groups: int) -> int:
    """What one sample moves per cell and plane: the sample read, every selected accumulator read and written."""
    return 4 + (16 if groups & 1 else 0) + (16 if groups & 2 else 0) + (16 if groups & 4 else 0) + (16 if groups & 8 else 0)


def copy_ms(nbytes: int, calls: int):
    """A function that times one device-to-device copy that moves ``nbytes`` (half read, half written) with torch's events."""
    import torch

    src = torch.zeros(max(nbytes // 2, 1), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)

    def once():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    return once


def host_update(acc, planes, groups, stamp):
    """The restated rule in numpy on downloaded planes (tests/time_stats_ref.py states it for the tests)."""
    import numpy as np

    for a, x in zip(acc, planes):
        if groups & 1:
            a["sum"] += x
        if groups & 2:
            x64 = x.astype(np.float64)
            a["squares"] += x64 * x64
        if groups & 4:
            np.minimum(a["min"], x, out=a["min"], where=x < a["min"])
            np.maximum(a["max"], x, out=a["max"], where=x > a["max"])
        if groups & 8:
            hit = x > np.float32(0.25)
            a["set_count"] += hit
            a["first_stamp"][hit & (a["first_stamp"] == 0xFFFFFFFF)] = stamp


def host_acc(shape, n):
    import numpy as np

    return [{"sum": np.zeros(shape), "squares": np.zeros(shape), "min": np.full(shape, np.inf, np.float32),
             "max": np.full(shape, -np.inf, np.float32), "set_count": np.zeros(shape, np.uint32),
             "first_stamp": np.full(shape, 0xFFFFFFFF, np.uint32)} for _ in range(n)]


def measure(ctx, label, cells, nplanes, groups_name, groups, accumulate, summarize, download, shape, calls, host_calls):
    per = bytes_per_cell(groups)
    moved = per * cells * nplanes
    copy = copy_ms(moved, calls)
    accumulate()
    summarize()
    copy()
    got = {"accumulate": [], "summary": [], "copy": []}
    for _ in range(calls):
        got["accumulate"].append(ratekit.device_ms(ctx, accumulate))
        got["summary"].append(ratekit.device_ms(ctx, summarize))
        got["copy"].append(copy())
    host = None
    if host_calls:
        acc = host_acc(shape, nplanes)
        host = statistics.median(ratekit.wall_ms(lambda: host_update(acc, download(), groups, 7)) for _ in range(host_calls))
    a, s, c = (statistics.median(got[k]) for k in ("accumulate", "summary", "copy"))
    return {"grid": label, "cells": cells, "planes": nplanes, "groups": groups_name, "bytes_per_cell_and_plane": per,
            "accumulate_device_ms": a, "moved_tb_per_s": moved / (a * 1e-3) / 1e12, "copy_ms": c,
            "copy_tb_per_s": moved / (c * 1e-3) / 1e12, "accumulate_over_copy": a / c, "summary_device_ms": s, "host_route_ms": host}


def species_rows(rows, cols, calls, host_calls):
    from grayscott_amd import capi
    from grayscott_amd.simulation import summarize_fields

    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        sim.perform_steps(species, 16)
        in_u, in_v, _, _ = species.in_out()
        lib = ctx._lib
        t, above = (ctypes.c_float * 2)(0.25, 0.25), (ctypes.c_int32 * 2)(1, 1)
        for planes in ([in_v], [in_u, in_v]):
            n = len(planes)
            arr = (ctypes.c_void_p * n)(*[p.handle for p in planes])
            for name, groups in GROUP_SETS:
                h = ctypes.c_void_p()
                capi.check(lib.gs_time_stats_create(ctx.handle, ctypes.byref(h), rows, cols, n, groups, t, above))
                stamp = [0]

                def accumulate():
                    stamp[0] += 1
                    capi.check(lib.gs_time_stats_accumulate(ctx.handle, h, arr, n, stamp[0]))
                try:
                    yield measure(ctx, f"{rows}x{cols}", rows * cols, n, name, groups, accumulate,
                                  lambda: summarize_fields(ctx, planes), lambda: [p.make_scalar_view(ctx) for p in planes],
                                  (rows, cols), calls, host_calls)
                finally:
                    capi.check(lib.gs_time_stats_destroy(ctx.handle, h))


def ensemble_rows(members, rows, cols, calls, host_calls):
    with ratekit.ensemble_subject(members, rows, cols) as (sim, ctx, ens):
        ens.perform_steps(16)
        for name, groups in GROUP_SETS:
            stats = ens.time_stats(groups, v_threshold=0.25, u_threshold=0.25)
            stamp = [0]

            def accumulate():
                stamp[0] += 1
                stats.accumulate(stamp[0])
            try:
                yield measure(ctx, f"{members} x {rows}x{cols}", members * rows * cols, 2, name, groups, accumulate, ens.summaries,
                              lambda: [ens.u_views(), ens.result_views()], (members, rows, cols), calls, host_calls)
            finally:
                stats.close()


def main(argv=None) -> int:
    args = ratekit.observable_args(__doc__, argv, calls=10,
                                   add=lambda ap: ap.add_argument("--host-calls", type=int, default=1))
    report = ratekit.Report(args.json, args.md)
    rows = []
    for r, c in ratekit.parse_grids(args.grids):
        rows += [report.row(x) for x in species_rows(r, c, args.calls, args.host_calls)]
    if not args.no_ensemble:
        rows += [report.row(x) for x in ensemble_rows(*ENSEMBLE, args.calls, args.host_calls)]
    report.table(*HEADER, *(
        f"| {r['grid']} | {r['planes']} | {r['groups']} | {r['bytes_per_cell_and_plane']} | {r['accumulate_device_ms']:.3f} | "
        f"{r['moved_tb_per_s']:.2f} | {r['copy_ms']:.3f} | {r['accumulate_over_copy']:.2f} | {r['summary_device_ms']:.3f} | "
        + ("-" if r["host_route_ms"] is None else f"{r['host_route_ms']:.1f}") + " |" for r in rows))
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
