"""Time of the regional connected components (gs_fields_region_components) against three things beside it, in one process.

For every Species grid (16384^2, 4096^2, 1080 x 1920), every region shape (64x64, 256x256, 1024x1024) and each of three inputs
-- ``new`` (Species::new untouched), ``random`` (cells of V set with probability 0.59, the 4-connected percolation regime: the
worst case for union-find) and ``full`` (every cell of V set: one component per region, every union made) -- the components
of every region of V at ONE threshold are timed under connectivity 8 and under 4, in turn with

* ``gs_fields_components`` under connectivity 8 on the same plane: the same labelling without walls and with one tally;
* ``gs_fields_region_morphology`` with one threshold on the same plane and regions: the one-pass floor of the regional family;
* the host route, where scipy is present and the grid has at most ``--host-cells`` cells: a download of the plane plus
  ``scipy.ndimage.label`` and a ``bincount`` on every crop, once per row (wall clock).

The calls block and the component calls allocate and free their label memory inside, so every figure is the wall time of the
call (``--calls`` times each in turn after a warm-up call, medians).  The regional call is the Python wrapper's, whose result
is allocated anew in every call.  A regional call whose result is over GS_REGION_COMPONENTS_MAX results per field is refused by
the library: its cells hold ``-``.  Where the host route runs, its component counts are compared with the device's.

    python tools/region_components_rate.py [--calls 5] [--grids 16384x16384,4096x4096,1080x1920]
                                           [--regions 64x64,256x256,1024x1024] [--no-host] [--host-cells N] [--json FILE] [--md FILE]

Needs the MI355X: there is no CPU path.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ratekit  # noqa: E402

KINDS = ("new", "random", "full")
REGIONS = "64x64,256x256,1024x1024"
TV = 0.25
DENSITY = 0.59
HEADER = ["| grid | region | input | components | region components, 8 (ms) | region components, 4 (ms) | components, 8 (ms) | "
          "8 / whole grid | region morphology (ms) | host route (ms) |",
          "|---|---|---|---|---|---|---|---|---|---|"]


def fill(sim, species, kind):
    """``new`` leaves Species::new; ``random`` is V = 0.5 on cells drawn with probability DENSITY and 0 on the others; ``full``
    is V = 0.5 everywhere."""
    import numpy as np

    if kind == "new":
        return
    shape = tuple(species.shape())
    if kind == "full":
        v = np.full(shape, 0.5, np.float32)
    else:
        rng = np.random.default_rng(3)
        v = np.where(rng.random(shape, dtype=np.float32) < np.float32(DENSITY), np.float32(0.5), np.float32(0.0)).astype(np.float32)
    species.in_out()[1].upload(sim.context, v)


def scipy_ndimage():
    try:
        from scipy import ndimage
    except ImportError:
        return None
    return ndimage


def host_route(ndimage, ctx, in_v, region):
    """Download of V, then label and bincount of every crop: (components, largest) per region."""
    import numpy as np

    rh, rw = region
    bits = in_v.make_scalar_view(ctx) > np.float32(TV)
    rows, cols = bits.shape
    eight = ndimage.generate_binary_structure(2, 2)
    count = np.zeros((-(-rows // rh), -(-cols // rw)), np.int64)
    largest = np.zeros_like(count)
    for i in range(count.shape[0]):
        for j in range(count.shape[1]):
            labels, n = ndimage.label(bits[i * rh:(i + 1) * rh, j * rw:(j + 1) * rw], eight)
            count[i, j] = n
            largest[i, j] = np.bincount(labels.ravel())[1:].max() if n else 0
    return count, largest


def time_species(rows, cols, regions, kind, calls, host):
    import numpy as np

    from grayscott_amd import capi

    with ratekit.species_subject(rows, cols) as (sim, ctx, species):
        fill(sim, species, kind)
        _, in_v, _, _ = species.in_out()
        for region in regions:
            fns = {"components8": lambda: in_v.components(ctx, [TV], True, 8),
                   "region_morphology": lambda: in_v.region_morphology(ctx, region, [TV])}
            c8 = None
            try:  # (a result over the cap is refused before any device work)
                c8 = in_v.region_components(ctx, region, [TV], True, 8)[0]
                fns["region_components8"] = lambda: in_v.region_components(ctx, region, [TV], True, 8)
                fns["region_components4"] = lambda: in_v.region_components(ctx, region, [TV], True, 4)
            except capi.GsError as e:
                if e.code != capi.GS_ERR_INVALID:
                    raise
            m = ratekit.medians(ctx, fns, calls, both=True)
            rec = {"grid": f"{rows}x{cols}", "region": f"{region[0]}x{region[1]}", "input": kind, "cells": rows * cols,
                   "components": int(c8.count.sum()) if c8 is not None else None, "label_memory_bytes": 8 * rows * cols,
                   "region_components8_ms": None, "region_components4_ms": None, "host_ms": None}
            for name, (wall, event) in m.items():
                rec[name + "_ms"], rec[name + "_event_ms"] = wall, event
            ndimage = scipy_ndimage() if host and c8 is not None else None
            if ndimage is not None:
                got = []
                rec["host_ms"] = ratekit.wall_ms(lambda: got.append(host_route(ndimage, ctx, in_v, region)))
                if not (np.array_equal(got[0][0], c8.count.astype(np.int64)) and np.array_equal(got[0][1], c8.largest.astype(np.int64))):
                    raise RuntimeError(f"{rec['grid']} {rec['region']} {kind}: the device and scipy count different components")
            yield rec


def main(argv=None) -> int:
    def add(ap):
        ap.add_argument("--regions", default=REGIONS, help="comma-separated RHxRW region shapes")
        ap.add_argument("--no-host", action="store_true", help="leave the host route out")
        ap.add_argument("--host-cells", type=int, default=1 << 24, help="the host route is timed on grids of at most this many cells")

    args = ratekit.observable_args(__doc__, argv, calls=5, add=add)
    report = ratekit.Report(args.json, args.md)
    regions = ratekit.parse_grids(args.regions)
    for r, c in ratekit.parse_grids(args.grids):
        for kind in KINDS:
            for rec in time_species(r, c, regions, kind, args.calls, not args.no_host and r * c <= args.host_cells):
                report.row(rec)

    def ms(x, digits=3):
        return f"{x:.{digits}f}" if x is not None else "-"

    for r in report.rows:
        r["region_components8_ratio"] = (r["region_components8_ms"] / r["components8_ms"]
                                         if r["region_components8_ms"] is not None else None)
    report.table(*HEADER, *(f"| {r['grid']} | {r['region']} | {r['input']} | {r['components'] if r['components'] is not None else '-'} | "
                            f"{ms(r['region_components8_ms'])} | {ms(r['region_components4_ms'])} | {r['components8_ms']:.3f} | "
                            f"{ms(r['region_components8_ratio'], 2)} | {r['region_morphology_ms']:.3f} | {ms(r['host_ms'], 1)} |"
                            for r in report.rows))
    report.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
