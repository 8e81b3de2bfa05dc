"""Time of the bundle statistics (gs_members_bundle_stats) beside three things measured in the same process: a summary of the
same members, a device-to-device copy of the same members, and the host route the call replaces.

For every configuration MEMBERSxROWSxCOLSxSPAN (default: 512 members of 64 x 128 with spans 8 and 32, 64 members of 256 x 512
with span 8) and for the result sets {mean, variance} and all five: after a few warm-up steps the call is made ``--calls``
times in turns with ``gs_members_summarize`` and ``gs_members_copy`` of the same members, each timed with device events and
the host clock, and the medians are reported.  The call reads every member once (4 bytes per cell, member and species) and
writes n result planes per bundle (4 n / span bytes per cell, member and species); the summary reads exactly the same bytes
once and writes next to nothing, so it is the yardstick: ``bundle / summary`` is what to judge the kernel by.  The copy reads
and writes the members' bytes.  The host route is what a user without the feature does: both species downloaded and the
results formed in numpy (``--host-calls`` times, default 1; 0 skips it).  The result ensembles are made before the clock
starts.

    python tools/bundle_stats_rate.py [--calls 10] [--host-calls 1] [--configs 512x64x128x8,512x64x128x32,64x256x512x8]
                                      [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402

CONFIGS = "512x64x128x8,512x64x128x32,64x256x512x8"
RESULT_SETS = (("mean+variance", ("mean", "variance")), ("all five", ("mean", "variance", "min", "max", "occupancy")))
HEADER = ["| members x grid | span | results | read (MB) | written (MB) | bundle, device (ms) | bundle, wall (ms) | read (TB/s) |"
          " summary, device (ms) | bundle / summary | copy, device (ms) | host route (ms) |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
KEYS = ("config", "members", "rows", "cols", "span", "results", "read_bytes", "written_bytes", "bundle_device_ms", "bundle_wall_ms",
        "read_tb_per_s", "summary_device_ms", "summary_wall_ms", "bundle_over_summary", "copy_device_ms", "copy_wall_ms",
        "host_route_ms")


def parse_configs(text):
    """[(members, rows, cols, span)] of a comma-separated list of MEMBERSxROWSxCOLSxSPAN, span dividing members."""
    out = []
    for item in filter(None, text.split(",")):
        try:
            c = tuple(int(x) for x in item.split("x"))
        except ValueError:
            c = ()
        if len(c) != 4 or min(c) < 1 or c[0] % c[3]:
            raise ValueError(f"not a configuration (MEMBERSxROWSxCOLSxSPAN, SPAN dividing MEMBERS): {item!r}")
        out.append(c)
    return out


def traffic(members, rows, cols, span, n):
    """(bytes read, bytes written) of one call with n results: every member's U and V once, n planes per bundle and species."""
    cells = rows * cols
    return 2 * 4 * members * cells, 2 * 4 * n * (members // span) * cells


def host_route(ens, span, names):
    """Both species downloaded, the results formed in numpy (f64 sums over the member axis)."""
    import numpy as np

    out = {}
    for x in (ens.u_views(), ens.result_views()):
        b = x.reshape((x.shape[0] // span, span) + x.shape[1:])
        if "mean" in names or "variance" in names:
            mean = b.mean(axis=1, dtype=np.float64)
            out["mean"] = mean.astype(np.float32)
        if "variance" in names:
            out["variance"] = np.maximum((b.astype(np.float64) ** 2).mean(axis=1) - mean * mean, 0.0).astype(np.float32)
        if "min" in names:
            out["min"], out["max"] = b.min(axis=1), b.max(axis=1)
        if "occupancy" in names:
            out["occupancy"] = (b > np.float32(0.25)).mean(axis=1, dtype=np.float64).astype(np.float32)
    return out


def config_rows(members, rows, cols, span, calls, host_calls):
    from grayscott_amd.simulation import Ensemble

    with ratekit.ensemble_subject(members, rows, cols) as (sim, ctx, ens):
        ens.perform_steps(16)
        snap = ens.snapshot()
        try:
            for label, names in RESULT_SETS:
                out = {name: Ensemble(ctx, members // span, (rows, cols)) for name in names}
                try:
                    fns = {"bundle": lambda: ens.bundle_stats(span, names, v_threshold=0.25, u_threshold=0.5, out=out),
                           "summary": ens.summaries, "copy": lambda: snap.copy_from(ens)}
                    got = ratekit.medians(ctx, fns, calls, both=True)
                finally:
                    for e in out.values():
                        e.destroy()
                host = None
                if host_calls:
                    host = statistics.median(ratekit.wall_ms(lambda: host_route(ens, span, names)) for _ in range(host_calls))
                read, written = traffic(members, rows, cols, span, len(names))
                (bw, bd), (sw, sd), (cw, cd) = got["bundle"], got["summary"], got["copy"]
                yield {"config": f"{members} x {rows}x{cols}", "members": members, "rows": rows, "cols": cols, "span": span,
                       "results": label, "read_bytes": read, "written_bytes": written, "bundle_device_ms": bd, "bundle_wall_ms": bw,
                       "read_tb_per_s": read / (bd * 1e-3) / 1e12, "summary_device_ms": sd, "summary_wall_ms": sw,
                       "bundle_over_summary": bd / sd, "copy_device_ms": cd, "copy_wall_ms": cw, "host_route_ms": host}
        finally:
            snap.destroy()


def main(argv=None) -> int:
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--configs", default=CONFIGS)
    ap.add_argument("--json", default=None, help="also write the rows as a JSON list")
    ap.add_argument("--md", default=None, help="also write the table as markdown")
    args = ap.parse_args(argv)
    configs = parse_configs(args.configs)
    import torch  # noqa: F401  (the process's HIP runtime is torch's, as in bench.py and the tests)

    report = ratekit.Report(args.json, args.md)
    rows = []
    for c in configs:
        rows += [report.row(x) for x in config_rows(*c, args.calls, args.host_calls)]
    report.table(*HEADER, *(
        f"| {r['config']} | {r['span']} | {r['results']} | {r['read_bytes'] / 1e6:.1f} | {r['written_bytes'] / 1e6:.1f} | "
        f"{r['bundle_device_ms']:.3f} | {r['bundle_wall_ms']:.3f} | {r['read_tb_per_s']:.2f} | {r['summary_device_ms']:.3f} | "
        f"{r['bundle_over_summary']:.2f} | {r['copy_device_ms']:.3f} | "
        + ("-" if r["host_route_ms"] is None else f"{r['host_route_ms']:.1f}") + " |" for r in rows))
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
