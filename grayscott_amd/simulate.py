"""``simulate``-equivalent driver loop on the HIP backend.

Mirrors /root/reference/simulate/src/main.rs:46-127: ``nbimage`` images, ``nbextrastep`` steps
between images, the V plane of every image handed to a writer thread through a bounded queue
with buffer recycling (main.rs:73-121), shared CLI flags of ui/src/lib.rs:18-46.  Like the
reference's ``async-gpu`` path (main.rs:99-106) the steps and the download of the result are
enqueued together: the download of image i overlaps the steps of image i+1.

    python -m grayscott_amd.simulate -n 100 -r 1080 -c 1920 -o out.h5

Output: the reference writes an HDF5 dataset ``matrix[nbimage, rows, cols]`` f32
(data/src/hdf5.rs:36-63).  ``-o name.h5`` (or ``.hdf5``) writes that dataset through the minimal
HDF5 writer of ``grayscott_amd/hdf5_min.py`` (libhdf5 / h5py are not in this image: see the status
note there); any other name gives a ``.npy`` file (numpy format 1.0, C order) with the same array.

Parameter maps (``gs_ctx_set_param_map``): ``--hip-feed-map F0:F1`` makes F vary linearly along the rows,
``--hip-kill-map K0:K1`` makes k vary linearly along the columns (Munafo's (F, k) map), ``--hip-param-map FILE.npz``
takes arrays ``feed`` and ``kill`` of the grid's shape.  The linear value of index i out of n is
``np.float32(a + (b - a) * i / (n - 1))`` computed in float64, a single row or column taking ``a``; a rate without a
map option is the uniform ``-f`` / ``-k`` value.  The output keeps the reference's format; the map's definition goes
into a JSON sidecar, ``-o``'s name with ``.param_map.json``.

Reduced images (``gs_field_download_reduced_async``): ``--hip-image-reduce F`` (1..64, default 1) writes every image
averaged over F x F blocks on the device -- the dataset becomes ``matrix[nbimage, ceil(rows / F), ceil(cols / F)]`` and
1 / F^2 of the bytes cross the link and reach the file; the steps are untouched.  With F = 1 the output is byte for byte
what it is without the option.

Domain masks (``gs_ctx_set_mask``): ``--hip-mask FILE.npy`` (or ``FILE.npz`` with an array ``mask``) of the grid's shape
makes the cells where it is nonzero walls.  It combines with every other option but the parameter map's, which it
refuses.

Noise (``gs_ctx_set_noise``): ``--hip-noise SU[:SV]`` adds a seeded stochastic increment to every step -- ``sigma * xi`` per
species, ``xi`` uniform on [-1, 1) and a pure function of (``--hip-noise-seed N``, step index, row, column); the run's first
step has index ``--hip-noise-step S`` (default 0).  The result file is bit-reproducible from the command line, whatever
kernel, fusion depth or slab count computes it.  Together with a parameter map or a mask the library refuses.

Regional observables (``gs_fields_region_summaries``, ``gs_fields_region_morphology``): ``--hip-regions RH[xRW]`` cuts the
grid into regions of RH x RW cells (RW a multiple of 4, at least 16; one number: square) and writes, next to the output,
``<stem>.regions.npz``: per observed image the summaries of U and V and the bit-quad counts of V (``--hip-region-threshold-v
A[,B...]``, default 0.25, set above) and, if asked for, of U (``--hip-region-threshold-u``, set below) of every region, all
formed on the device -- ``--hip-regions-every N`` observes every N-th image, the default is the last image alone.  With a
parameter map the file also holds ``feed`` and ``kill``, the regions' means of the maps (numpy, float64): the file is then the
phase diagram.  In a multi-process run rank 0 writes.  The two calls block: an observed image is waited for before the next
steps are enqueued, so with ``--hip-regions-every 1`` no download overlaps the steps of the next image any more (the pipeline of
two images in flight runs dry at every observed image); the default, the last image alone, costs nothing before the end.
``--hip-region-corr-lags L`` (1..64; needs ``--hip-regions``) adds the regions' two-point pair counts
(``gs_fields_region_correlation``, a region's border being a wall for pairs) at the same thresholds: ``pairs_v`` (and ``pairs_u``)
as [samples, nt, RR, RC, 4, L + 1] and ``corr_lags`` = L -- the wavelength axis of the phase diagram.
``--hip-region-hist-bins B`` (1..4096; needs ``--hip-regions``) adds the regions' histograms (``gs_fields_region_histogram``):
``hist_u`` and ``hist_v`` as [samples, RR, RC, B + 3] uint64 -- counts, then below, above, nan -- over
``--hip-region-hist-range-u A:B`` and ``--hip-region-hist-range-v A:B`` (each 0:1 by default), with ``hist_bins``,
``hist_range_u`` and ``hist_range_v``: any threshold, the median and the quantiles of every region, chosen after the run.
``--hip-region-components [4|8]`` (8 without a value; needs ``--hip-regions``) adds the regions' connected components
(``gs_fields_region_components``, a region's border being a wall) at the same thresholds: ``components_v`` (and
``components_u`` with ``--hip-region-threshold-u``) as [samples, nt, RR, RC, 35] uint64 -- components, set_cells, largest,
by_size[32] -- and ``comp_connectivity``: how many spots every region holds, how large, and whether one percolates it.
``--hip-region-change`` (needs ``--hip-regions``) adds the regions' change over the last image interval
(``gs_fields_region_compare``): image k against image k - 1 (the initial state for k = 1), the earlier state being a device
snapshot that is taken only before an interval that ends in an observed image -- ``change_{sum_abs,sum_sq,max_abs,differing,
nonfinite}_{u,v}`` as [samples, RR, RC] and ``change_steps``, the interval in steps.  ``--hip-region-steady-tol T`` (finite, at
least 0; needs ``--hip-region-change``) adds ``steady`` [samples, RR, RC], bool: neither U nor V moved by more than T in any cell of
the region and no cell is non-finite.  The run is not ended early on it.
``--hip-region-spectrum-tile T`` (16, 32, 64 or 128; needs ``--hip-regions``) adds the regions' tile-averaged power spectra
(``gs_fields_region_spectrum``, tiles anchored at every region's first row and column) under
``--hip-region-spectrum-window hann|none`` (hann by default; needs the tile option): ``spectrum_u`` and ``spectrum_v`` as
[samples, RR, RC, T, T/2 + 1] float64, the raw sums, ``spectrum_tiles_u`` and ``spectrum_tiles_v`` as [samples, RR, RC, 2]
uint64 -- tiles used, skipped --, with ``spectrum_tile`` and ``spectrum_window``: the wavelength with sub-cell resolution and
the stripes' orientation of every region, with no threshold (``RegionSpectrum.from_raw`` makes the object).

Time statistics (``gs_time_stats``): ``--hip-time-stats-every N`` samples U and V every N steps -- from step S on with
``--hip-time-stats-from S`` (default N; 0: the initial state too), at steps S, S + N, ..., each stamped with its step count -- into per-cell accumulators on
the device and writes, at the end, ``<stem>.timestats.npz``: ``samples``, ``steps`` and the planes ``mean_v``, ``var_v``,
``min_v``, ``max_v`` (and ``_u``), with ``--hip-time-stats-threshold-v T`` also ``occupancy_v`` and ``arrival_v`` (V set above
T; -1 where the front never arrived).  A sample waits for the steps enqueued before it and splits an image's steps where it
falls between two images; the images are bit for bit what they are without the option.  In a multi-process run every rank
writes its own rows, ``<stem>.timestats.rank<q>.npz`` with ``rows`` = its row range.
"""
from __future__ import annotations

import argparse
import json
import os
import queue
import sys
import threading
import time

import numpy as np

from . import hdf5_min
from .simulation import HipArgs, Parameters, Simulation, pinned_empty


def parse(argv=None):
    ap = argparse.ArgumentParser(prog="simulate", description="Perform Gray-Scott simulation")
    ap.add_argument("-k", "--killrate", type=float, default=None)        # ui/src/lib.rs:20-22
    ap.add_argument("-f", "--feedrate", type=float, default=None)        # :24-26
    ap.add_argument("-e", "--nbextrastep", type=int, default=None)       # :28-30 (default 32, main.rs:52)
    ap.add_argument("-r", "--nbrow", type=int, default=1080)             # :32-34
    ap.add_argument("-c", "--nbcol", type=int, default=1920)             # :36-38
    ap.add_argument("-t", "--deltat", type=float, default=None)          # :40-42
    ap.add_argument("-n", "--nbimage", type=int, default=1000)           # main.rs:29-31
    ap.add_argument("-o", "--output", default="output.h5")               # main.rs:33-35, ui/src/lib.rs:72-75
    ap.add_argument("--output-buffer", type=int, default=2)              # main.rs:37-43
    add_backend_args(ap)
    add_param_map_args(ap)
    add_mask_args(ap)
    add_noise_args(ap)
    add_image_args(ap)
    add_region_args(ap)
    add_time_stats_args(ap)
    args = ap.parse_args(argv)
    check_time_stats_args(ap, args, "hip_time_stats", "--hip-time-stats")
    tu, tv = args.hip_region_threshold_u, args.hip_region_threshold_v or [0.25]
    if tu is not None and len(tu) != len(tv):
        ap.error(f"--hip-region-threshold-u wants as many thresholds as --hip-region-threshold-v ({len(tv)}), not {len(tu)}")
    if args.hip_region_corr_lags is not None and args.hip_regions is None:
        ap.error("--hip-region-corr-lags needs --hip-regions")
    if args.hip_region_hist_bins is not None and args.hip_regions is None:
        ap.error("--hip-region-hist-bins needs --hip-regions")
    if args.hip_region_components is not None and args.hip_regions is None:
        ap.error("--hip-region-components needs --hip-regions")
    if args.hip_region_change and args.hip_regions is None:
        ap.error("--hip-region-change needs --hip-regions")
    if args.hip_region_spectrum_tile is not None and args.hip_regions is None:
        ap.error("--hip-region-spectrum-tile needs --hip-regions")
    if args.hip_region_spectrum_window is not None and args.hip_region_spectrum_tile is None:
        ap.error("--hip-region-spectrum-window needs --hip-region-spectrum-tile")
    if args.hip_region_spectrum_tile is not None and args.hip_region_spectrum_window is None:
        args.hip_region_spectrum_window = "hann"
    if args.hip_region_steady_tol is not None and not args.hip_region_change:
        ap.error("--hip-region-steady-tol needs --hip-region-change")
    for name in ("u", "v"):
        if getattr(args, f"hip_region_hist_range_{name}") is not None and args.hip_region_hist_bins is None:
            ap.error(f"--hip-region-hist-range-{name} needs --hip-region-hist-bins")
    return args


def add_backend_args(ap: argparse.ArgumentParser) -> None:
    """The ``--hip-*`` group (shared with ``grayscott_amd.sweep``)."""
    # The backend's own parameters, flattened into the command line as the reference flattens
    # `Simulation::CliArgs` (ui/src/lib.rs:43-45, inside the SharedArgs that simulate/src/main.rs:25-27 flattens): the names, meanings and environment
    # variables of rust/compute_hip/src/lib.rs (HipArgs).  Defaults come from the environment (HipArgs' own).
    be = ap.add_argument_group("HIP backend")
    be.add_argument("--hip-devices", default=None, metavar="ID[,ID...]",
                    help="HIP devices that run the simulation, one row slab each, top to bottom [env GS_HIP_DEVICES, 0]")
    be.add_argument("--hip-math", type=int, default=None, help="0 = strict (bit-identical to compute_naive), 1 = fused taps [GS_HIP_MATH]")
    be.add_argument("--hip-rows-per-block", type=int, default=None, help="rows each wavefront marches over, 0 = chosen on line [GS_HIP_ROWS_PER_BLOCK]")
    be.add_argument("--hip-fuse-steps", type=int, default=None, help="time steps fused per pass over HBM, 1..4, 0 = chosen on line [GS_HIP_FUSE_STEPS]")
    be.add_argument("--hip-cols-per-lane", type=int, default=None, help="columns per lane: 4, 2 or 1, 0 = chosen on line [GS_HIP_COLS_PER_LANE]")
    be.add_argument("--hip-no-tune", type=int, default=None, help="1 = never time candidate configurations inside perform_steps [GS_HIP_NO_TUNE]")
    be.add_argument("--hip-kernel", type=int, default=None, help="step kernel (gs_kernel in gs_hip.h), 0 = by grid size and call length [GS_HIP_KERNEL]")
    be.add_argument("--hip-boundary", type=int, default=None, help="0 = compute_naive's clipped window, 1 = zero halo (the SIMD / Vulkan backends' rule), 2 = periodic (single GPU, one process), 3 = zero flux (Neumann: a neighbour outside the grid is the nearest cell inside it) [GS_HIP_BOUNDARY]")
    be.add_argument("--hip-general-kernels", type=int, default=None, help="1 = never run the variants specialised for the default stencil and time step [GS_HIP_GENERAL_KERNELS]")
    be.add_argument("--hip-share-taps", type=int, default=None, help="full difference sharing: 0 = on (form 3) unless measured slower, 1 = within a lane only, 2 = off, 3 = across lanes too [GS_HIP_SHARE_TAPS]")
    be.add_argument("--hip-place-candidates", type=int, default=None, help="most extra blocks gs_fields_place may draw when a Species of >= 2^26 cells is placed by measurement (default 12; 0 = planes as hipMalloc hands them out) [GS_HIP_PLACE_CANDIDATES]")
    be.add_argument("--hip-split", type=int, default=None, help="row bands a single slab is scheduled as [GS_HIP_SPLIT]")
    be.add_argument("--hip-use-graph", type=int, default=None, help="1 = replay batches of 16 passes through a hipGraph [GS_HIP_USE_GRAPH]")
    be.add_argument("--hip-tile-shape", type=int, default=None, help="window of the LDS-window kernel: 1 = 32x64, 2 = 16x64, 3 = 64x64 [GS_HIP_TILE_SHAPE]")
    be.add_argument("--hip-pitch-pad", type=int, default=None, help="extra f32 of row pitch [GS_HIP_PITCH_PAD]")


def add_param_map_args(ap: argparse.ArgumentParser) -> None:
    """The parameter map's options of the ``--hip-*`` group (simulate only)."""
    pm = ap.add_argument_group("HIP backend: parameter map")
    pm.add_argument("--hip-feed-map", default=None, metavar="F0:F1", help="feed rate varying linearly along the rows, F0 on the first, F1 on the last")
    pm.add_argument("--hip-kill-map", default=None, metavar="K0:K1", help="kill rate varying linearly along the columns, K0 on the first, K1 on the last")
    pm.add_argument("--hip-param-map", default=None, metavar="FILE.npz", help="arrays `feed` and `kill` of the grid's shape")


def add_mask_args(ap: argparse.ArgumentParser) -> None:
    """The domain mask's option of the ``--hip-*`` group (simulate only)."""
    mk = ap.add_argument_group("HIP backend: domain mask")
    mk.add_argument("--hip-mask", default=None, metavar="FILE.npy",
                    help="walls where the array (.npy, or array `mask` of a .npz) is nonzero; not with a parameter map")


def add_noise_args(ap: argparse.ArgumentParser) -> None:
    """The noise term's options of the ``--hip-*`` group (simulate only)."""
    nz = ap.add_argument_group("HIP backend: noise")
    nz.add_argument("--hip-noise", default=None, metavar="SU[:SV]",
                    help="seeded noise: sigma of U's and of V's increment per step (SV defaults to 0); not with a parameter map or a mask")
    nz.add_argument("--hip-noise-seed", default=0, type=int, metavar="N", help="the noise's seed (u64, default 0)")
    nz.add_argument("--hip-noise-step", default=0, type=int, metavar="S", help="index of the run's first step (u64, default 0)")


def noise_term(args):
    """``(sigma_u, sigma_v, seed, step)`` as ``--hip-noise`` and its companions ask for, or None."""
    text = getattr(args, "hip_noise", None)
    if text is None:
        return None
    try:
        parts = [float(x) for x in str(text).split(":")]
    except ValueError:
        parts = []
    if len(parts) not in (1, 2):
        raise ValueError(f"--hip-noise wants SU or SU:SV, got {text!r}")
    return parts[0], parts[1] if len(parts) == 2 else 0.0, int(getattr(args, "hip_noise_seed", 0) or 0), int(getattr(args, "hip_noise_step", 0) or 0)


def _reduce_factor(text: str) -> int:
    try:
        value = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"an integer from 1 to 64, not {text!r}") from None
    if not 1 <= value <= 64:
        raise argparse.ArgumentTypeError(f"an integer from 1 to 64, not {value}")
    return value


def add_image_args(ap: argparse.ArgumentParser) -> None:
    """The result images' option of the ``--hip-*`` group (simulate only)."""
    im = ap.add_argument_group("HIP backend: result images")
    im.add_argument("--hip-image-reduce", type=_reduce_factor, default=1, metavar="F",
                    help="write every image averaged over F x F blocks on the device (1..64): matrix[nbimage, ceil(rows / F), "
                         "ceil(cols / F)], 1 / F^2 of the bytes; 1 = the full planes")


def parse_regions(text: str):
    """``RH[xRW]`` as (rh, rw): one number is a square region.  What the library asks of a region shape is checked here
    too, so that a wrong flag fails before anything runs."""
    try:
        parts = [int(x) for x in text.lower().split("x")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"RH[xRW], two integers, not {text!r}") from None
    if len(parts) not in (1, 2):
        raise argparse.ArgumentTypeError(f"RH[xRW], not {text!r}")
    rh, rw = parts[0], parts[-1]
    if rh < 1 or rw < 16 or rw % 4 != 0:
        raise argparse.ArgumentTypeError(f"a region of {rh} x {rw}: RH is at least 1, RW a multiple of 4 and at least 16")
    return rh, rw


def _threshold_list(text: str):
    try:
        values = [float(x) for x in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"1 to 4 numbers A[,B...], not {text!r}") from None
    if not 1 <= len(values) <= 4 or any(np.isnan(v) for v in values):
        raise argparse.ArgumentTypeError(f"1 to 4 numbers A[,B...], none NaN, not {text!r}")
    return values


def _lag_count(text: str) -> int:
    try:
        value = int(text)
    except ValueError:
        value = 0
    if not 1 <= value <= 64:
        raise argparse.ArgumentTypeError(f"a largest lag of 1 to 64, not {text!r}")
    return value


def _bin_count(text: str) -> int:
    try:
        value = int(text)
    except ValueError:
        value = 0
    if not 1 <= value <= 4096:
        raise argparse.ArgumentTypeError(f"1 to 4096 bins, not {text!r}")
    return value


def _hist_range(text: str):
    try:
        lo, hi = (float(x) for x in text.split(":"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"a range A:B, two numbers, not {text!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise argparse.ArgumentTypeError(f"a range A:B with A < B, both finite, not {text!r}")
    return lo, hi


def _tolerance(text: str) -> float:
    try:
        value = float(text)
    except ValueError:
        value = -1.0
    if not (np.isfinite(value) and value >= 0.0):
        raise argparse.ArgumentTypeError(f"a finite tolerance of at least 0, not {text!r}")
    return value


def _positive(text: str) -> int:
    try:
        value = int(text)
    except ValueError:
        value = 0
    if value < 1:
        raise argparse.ArgumentTypeError(f"an integer of at least 1, not {text!r}")
    return value


def add_region_args(ap: argparse.ArgumentParser) -> None:
    """The regional observables' options of the ``--hip-*`` group (simulate only)."""
    rg = ap.add_argument_group("HIP backend: regional observables")
    rg.add_argument("--hip-regions", type=parse_regions, default=None, metavar="RH[xRW]",
                    help="summaries and bit-quad counts of every region of RH x RW cells, formed on the device, into <stem>.regions.npz")
    rg.add_argument("--hip-regions-every", type=_positive, default=None, metavar="N",
                    help="observe every N-th image (default: the last image alone)")
    rg.add_argument("--hip-region-threshold-v", type=_threshold_list, default=None, metavar="A[,B...]",
                    help="V is set above these thresholds (1..4; default 0.25)")
    rg.add_argument("--hip-region-threshold-u", type=_threshold_list, default=None, metavar="A[,B...]",
                    help="U is set below these thresholds (as many as V's; default: U's quads are not counted)")
    rg.add_argument("--hip-region-corr-lags", type=_lag_count, default=None, metavar="L",
                    help="also the regions' two-point pair counts at lags 0..L (1..64) at the region thresholds (needs --hip-regions)")
    rg.add_argument("--hip-region-hist-bins", type=_bin_count, default=None, metavar="B",
                    help="also the regions' histograms of U and V over B (1..4096) equal bins (needs --hip-regions)")
    rg.add_argument("--hip-region-components", type=int, choices=(4, 8), nargs="?", const=8, default=None, metavar="4|8",
                    help="also the regions' connected components of V (and of U with --hip-region-threshold-u) at the region "
                         "thresholds under connectivity 4 or 8 (8 without a value; needs --hip-regions)")
    rg.add_argument("--hip-region-change", action="store_true",
                    help="also the regions' change of U and V over the last image interval, against a device snapshot "
                         "(needs --hip-regions)")
    rg.add_argument("--hip-region-steady-tol", type=_tolerance, default=None, metavar="T",
                    help="also `steady`: the regions in which neither U nor V moved by more than T over that interval "
                         "(finite, at least 0; needs --hip-region-change)")
    rg.add_argument("--hip-region-spectrum-tile", type=int, choices=(16, 32, 64, 128), default=None, metavar="T",
                    help="also the regions' tile-averaged power spectra of U and V, tiles of T (16, 32, 64, 128) cells a side "
                         "anchored at every region's first row and column (needs --hip-regions)")
    rg.add_argument("--hip-region-spectrum-window", choices=("hann", "none"), default=None,
                    help="the window of those tiles (default hann; needs --hip-region-spectrum-tile)")
    rg.add_argument("--hip-region-hist-range-u", type=_hist_range, default=None, metavar="A:B",
                    help="the range of U's histograms (default 0:1; needs --hip-region-hist-bins)")
    rg.add_argument("--hip-region-hist-range-v", type=_hist_range, default=None, metavar="A:B",
                    help="the range of V's histograms (default 0:1; needs --hip-region-hist-bins); a negative A is written "
                         "--hip-region-hist-range-v=A:B")


def add_time_stats_args(ap: argparse.ArgumentParser, prefix: str = "--hip-time-stats") -> None:
    """The time statistics' options (``--hip-time-stats-*`` here, ``--time-stats-*`` in ``grayscott_amd.sweep``)."""
    ts = ap.add_argument_group("HIP backend: time statistics")
    ts.add_argument(f"{prefix}-every", type=int, default=0, metavar="N",
                    help="sample U and V every N steps into per-cell accumulators on the device (<stem>.timestats.npz)")
    ts.add_argument(f"{prefix}-from", type=int, default=None, metavar="S", help="the first sampled step (default N)")
    ts.add_argument(f"{prefix}-threshold-v", type=float, default=None, metavar="T",
                    help="also record for what share of the samples V was above T and at which step it first was")


def check_time_stats_args(ap: argparse.ArgumentParser, args, name: str, flag: str) -> None:
    """The refusals of the time statistics' options; leaves ``<name>_from`` filled in."""
    every, start, t = (getattr(args, f"{name}_{k}") for k in ("every", "from", "threshold_v"))
    if every < 0:
        ap.error(f"{flag}-every must be at least 1 (0 = off)")
    if not every and start is not None:
        ap.error(f"{flag}-from needs {flag}-every")
    if not every and t is not None:
        ap.error(f"{flag}-threshold-v needs {flag}-every")
    if start is not None and start < 0:
        ap.error(f"{flag}-from must be at least 0")
    if t is not None and t != t:
        ap.error(f"{flag}-threshold-v must be a number")
    if every and start is None:
        setattr(args, f"{name}_from", every)


def time_stats_path(output: str, rank: int = 0, world: int = 1) -> str:
    """The time statistics' file next to the output file (one per rank in a multi-process run)."""
    return os.path.splitext(output)[0] + (".timestats.npz" if world == 1 else f".timestats.rank{rank}.npz")


def time_stats_steps(steps: int, every: int, start: int):
    """The sampled steps of a run of ``steps`` steps: ``start``, ``start + every``, ... up to ``steps``."""
    return list(range(start, steps + 1, every)) if every else []


def time_stats_groups(threshold_v) -> tuple:
    return ("sum", "squares", "extremes") + (("crossings",) if threshold_v is not None else ())


def write_time_stats(path: str, samples: int, steps, planes: dict, extra: dict = None) -> None:
    """``planes``: {"mean_v": array, ...} as the ``TimeStats`` result methods name them; everything goes into one .npz."""
    with open(path, "wb") as f:
        np.savez(f, samples=np.int64(samples), steps=np.asarray(steps, np.int64), **planes, **(extra or {}))


TIME_STATS_PLANES = (("mean", "mean"), ("var", "variance"), ("min", "min"), ("max", "max"))
TIME_STATS_CROSSING_PLANES = (("occupancy", "occupancy"), ("arrival", "arrival"))


def time_stats_planes(stats, threshold_v, read) -> dict:
    """Every plane the options ask for from a ``TimeStats``: ``read(plane)`` turns what a result method returns into an array."""
    out = {}
    for species in ("v", "u"):
        for key, method in TIME_STATS_PLANES:
            out[f"{key}_{species}"] = read(getattr(stats, method)(species))
    if threshold_v is not None:
        for key, method in TIME_STATS_CROSSING_PLANES:
            out[f"{key}_v"] = read(getattr(stats, method)("v"))
    return out


def regions_path(output: str) -> str:
    """The regional observables' file next to the output file."""
    return os.path.splitext(output)[0] + ".regions.npz"


def region_means(values, shape, region) -> np.ndarray:
    """The mean of ``values`` -- a [rows, cols] array, or a scalar for a uniform plane -- over every region of ``region`` =
    (rh, rw) cells of a grid of ``shape``, in float64: (ceil(rows / rh), ceil(cols / rw)), ragged regions over their own cells."""
    rows, cols = shape
    rh, rw = region
    a = np.broadcast_to(np.asarray(values, np.float64), (rows, cols))
    row_edges, col_edges = np.arange(0, rows, rh), np.arange(0, cols, rw)
    sums = np.add.reduceat(np.add.reduceat(a, row_edges, axis=0), col_edges, axis=1)
    h = np.minimum(rh, rows - row_edges)
    w = np.minimum(rw, cols - col_edges)
    return sums / (h[:, None] * w[None, :])


def regions_observed(image: int, images: int, every) -> bool:
    """Is image ``image`` (1-based) of ``images`` one that ``--hip-regions-every`` observes?"""
    return image == images if every is None else image % every == 0


def region_hist_args(args):
    """``RegionLog``'s ``hist`` from the ``--hip-region-hist-*`` options: None without ``--hip-region-hist-bins``."""
    bins = getattr(args, "hip_region_hist_bins", None)
    if bins is None:
        return None
    return bins, getattr(args, "hip_region_hist_range_u", None), getattr(args, "hip_region_hist_range_v", None)


def region_spectrum_args(args):
    """``RegionLog``'s ``spectrum`` from the ``--hip-region-spectrum-*`` options: None without the tile option."""
    tile = getattr(args, "hip_region_spectrum_tile", None)
    if tile is None:
        return None
    return tile, getattr(args, "hip_region_spectrum_window", None) or "hann"


class RegionLog:
    """What ``--hip-regions`` collects, one entry per observed image, and the file it becomes."""

    SUMMARY_KEYS = ("sum", "sum_sq", "min", "max", "nonfinite")
    CHANGE_KEYS = ("sum_abs", "sum_sq", "max_abs", "differing", "nonfinite")

    def __init__(self, region, thresholds_v, thresholds_u, corr_lags=None, hist=None, components=None, change=False,
                 steady_tol=None, spectrum=None):
        """``hist``: None, or (bins, U's (lo, hi), V's (lo, hi)) -- a range that is None is (0, 1).  ``components``: None, or
        the connectivity (4 or 8) of the regions' connected components.  ``change``: also the regions' change over the last
        image interval (``before_interval`` takes the earlier state); ``steady_tol``: None, or the tolerance of ``steady``.
        ``spectrum``: None, or (tile, "hann" or "none") of the regions' power spectra."""
        self.region = region
        self.spectrum = None if spectrum is None else (int(spectrum[0]), str(spectrum[1]))
        self.change, self.change_steps, self.snapshot = bool(change), None, None
        self.steady_tol = None if steady_tol is None else float(steady_tol)
        if self.steady_tol is not None and not self.change:
            raise ValueError("--hip-region-steady-tol needs --hip-region-change")
        self.components = None if components is None else int(components)
        self.corr_lags = corr_lags
        self.hist = None if hist is None else (int(hist[0]), tuple(hist[1] or (0.0, 1.0)), tuple(hist[2] or (0.0, 1.0)))
        self.thresholds_v = list(thresholds_v) if thresholds_v else [0.25]
        self.thresholds_u = list(thresholds_u) if thresholds_u else None
        if self.thresholds_u is not None and len(self.thresholds_u) != len(self.thresholds_v):
            raise ValueError("--hip-region-threshold-u wants as many thresholds as --hip-region-threshold-v")
        self.steps, self.rows = [], {}

    def before_interval(self, species, steps: int) -> None:
        """With ``change``: keep the current state on the device (blocking), to compare the state ``steps`` steps on with.
        Called only before an interval that ends in an observed image."""
        if not self.change:
            return
        if self.snapshot is None:
            self.snapshot = species.snapshot()
        else:
            self.snapshot.update(species)
        self.change_steps = int(steps)

    def close(self) -> None:
        if self.snapshot is not None:
            self.snapshot.close()
            self.snapshot = None

    def observe(self, species, step: int) -> None:
        su, sv = species.region_summaries(self.region)
        mu, mv = species.region_morphology(self.region, self.thresholds_v, self.thresholds_u)
        self.steps.append(step)
        for name, s in (("u", su), ("v", sv)):
            for key in self.SUMMARY_KEYS:
                self.rows.setdefault(f"{key}_{name}", []).append(getattr(s, key))
        self.rows.setdefault("cells", []).append(sv.size)
        self.rows.setdefault("quads_v", []).append(np.stack([m.quads for m in mv]))
        if mu:
            self.rows.setdefault("quads_u", []).append(np.stack([m.quads for m in mu]))
        if self.corr_lags is not None:
            cu, cv = species.region_correlation(self.region, self.thresholds_v, self.thresholds_u, self.corr_lags)
            self.rows.setdefault("pairs_v", []).append(np.stack([c.pairs for c in cv]))
            if cu:
                self.rows.setdefault("pairs_u", []).append(np.stack([c.pairs for c in cu]))
        if self.hist is not None:
            bins, u_range, v_range = self.hist
            for name, h in zip(("u", "v"), species.region_histogram(self.region, bins, u_range, v_range)):
                counters = np.concatenate([h.counts, np.stack([h.below, h.above, h.nan], axis=2)], axis=2)  # the C ABI's slots
                self.rows.setdefault(f"hist_{name}", []).append(counters)
        if self.components is not None:
            cu, cv = species.region_components(self.region, self.thresholds_v, self.thresholds_u, connectivity=self.components)
            self.rows.setdefault("components_v", []).append(np.stack([c.counters() for c in cv]))  # the C ABI's 35 words
            if cu:
                self.rows.setdefault("components_u", []).append(np.stack([c.counters() for c in cu]))
        if self.spectrum is not None:
            for name, sp in zip(("u", "v"), species.region_spectrum(self.region, *self.spectrum)):
                self.rows.setdefault(f"spectrum_{name}", []).append(sp.raw)
                self.rows.setdefault(f"spectrum_tiles_{name}", []).append(np.stack([sp.tiles_used, sp.tiles_skipped], axis=2))
        if self.change:
            if self.snapshot is None:
                raise RuntimeError("no earlier state to compare with: before_interval was not called")
            du, dv = species.region_changes_since(self.snapshot, self.region)
            for name, d in (("u", du), ("v", dv)):
                for key in self.CHANGE_KEYS:
                    self.rows.setdefault(f"change_{key}_{name}", []).append(getattr(d, key))
            if self.steady_tol is not None:
                self.rows.setdefault("steady", []).append(du.steady(self.steady_tol) & dv.steady(self.steady_tol))

    def save(self, path: str, shape, pmap=None) -> None:
        out = {"region": np.array(self.region, np.int64), "shape": np.array(shape, np.int64), "steps": np.array(self.steps, np.int64),
               "thresholds_v": np.array(self.thresholds_v, np.float32),
               "thresholds_u": np.array(self.thresholds_u or [], np.float32)}
        if self.corr_lags is not None:
            out["corr_lags"] = np.array(self.corr_lags, np.int64)
        if self.hist is not None:
            out["hist_bins"] = np.array(self.hist[0], np.int64)
            out["hist_range_u"] = np.array(self.hist[1], np.float64)
            out["hist_range_v"] = np.array(self.hist[2], np.float64)
        if self.components is not None:
            out["comp_connectivity"] = np.array(self.components, np.int64)
        if self.spectrum is not None:
            out["spectrum_tile"] = np.array(self.spectrum[0], np.int64)
            out["spectrum_window"] = np.array(self.spectrum[1])
        if self.change:
            out["change_steps"] = np.array(self.change_steps or 0, np.int64)
        if self.steady_tol is not None:
            out["steady_tol"] = np.array(self.steady_tol, np.float64)
        for key, rows in self.rows.items():
            out[key] = rows[0] if key == "cells" else np.stack(rows)
        if pmap is not None:
            out["feed"] = region_means(pmap[0], shape, self.region)
            out["kill"] = region_means(pmap[1], shape, self.region)
        with open(path, "wb") as f:
            np.savez(f, **out)


def image_shape(args):
    """Shape of one image of the output dataset: the grid's, reduced by ``--hip-image-reduce``."""
    f = int(getattr(args, "hip_image_reduce", 1) or 1)
    return (-(-args.nbrow // f), -(-args.nbcol // f))


def domain_mask(args, shape):
    """The wall array ``--hip-mask`` asks for (any dtype, the grid's shape), or None."""
    path = getattr(args, "hip_mask", None)
    if path is None:
        return None
    if any(getattr(args, n, None) is not None for n in ("hip_feed_map", "hip_kill_map", "hip_param_map")):
        raise ValueError("--hip-mask excludes --hip-feed-map, --hip-kill-map and --hip-param-map "
                         "(a domain mask and a parameter map cannot be attached together)")
    if path.lower().endswith(".npz"):
        with np.load(path) as z:
            if "mask" not in z:
                raise ValueError(f"{path}: no array `mask`")
            mask = np.asarray(z["mask"])
    else:
        mask = np.load(path)
    if mask.shape != tuple(shape):
        raise ValueError(f"{path}: the mask is {mask.shape}, the grid is {tuple(shape)}")
    return mask


def linear_values(a: float, b: float, n: int) -> np.ndarray:
    """The linear map's values: ``np.float32(a + (b - a) * i / (n - 1))`` in float64 for i = 0 .. n - 1; n == 1 gives a."""
    if n == 1:
        return np.array([a], np.float32)
    i = np.arange(n, dtype=np.float64)
    return (float(a) + (float(b) - float(a)) * i / (n - 1)).astype(np.float32)


def _range(text: str, flag: str):
    try:
        a, b = (float(x) for x in text.split(":"))
    except ValueError:
        raise ValueError(f"{flag} wants FROM:TO, got {text!r}") from None
    return a, b


def param_map(args, shape, params: Parameters):
    """(feed, kill, definition) of the parameter map the options ask for, or None.  ``feed`` / ``kill``: float32
    [rows, cols] arrays or scalars (uniform planes); ``definition``: what the JSON sidecar records."""
    feed_map, kill_map, path = (getattr(args, n, None) for n in ("hip_feed_map", "hip_kill_map", "hip_param_map"))
    if feed_map is None and kill_map is None and path is None:
        return None
    rows, cols = shape
    if path is not None:
        if feed_map is not None or kill_map is not None:
            raise ValueError("--hip-param-map excludes --hip-feed-map and --hip-kill-map")
        with np.load(path) as z:
            feed, kill = (np.asarray(z[n], np.float32) for n in ("feed", "kill"))
        for name, a in (("feed", feed), ("kill", kill)):
            if a.shape != (rows, cols):
                raise ValueError(f"{path}: `{name}` is {a.shape}, the grid is {(rows, cols)}")
        return feed, kill, {"shape": [rows, cols], "file": os.path.abspath(path)}
    definition = {"shape": [rows, cols], "formula": "float32(a + (b - a) * i / (n - 1)), float64 arithmetic"}
    if feed_map is not None:
        a, b = _range(feed_map, "--hip-feed-map")
        feed = np.repeat(linear_values(a, b, rows)[:, None], cols, axis=1)
        definition["feed"] = {"along": "rows", "from": a, "to": b}
    else:
        feed = np.float32(params.feed_rate)
        definition["feed"] = {"value": float(params.feed_rate)}
    if kill_map is not None:
        a, b = _range(kill_map, "--hip-kill-map")
        kill = np.repeat(linear_values(a, b, cols)[None, :], rows, axis=0)
        definition["kill"] = {"along": "columns", "from": a, "to": b}
    else:
        kill = np.float32(params.kill_rate)
        definition["kill"] = {"value": float(params.kill_rate)}
    return feed, kill, definition


def sidecar_path(output: str) -> str:
    """The parameter map's JSON sidecar next to the output file."""
    return os.path.splitext(output)[0] + ".param_map.json"


def backend_args(args) -> HipArgs:
    """``HipArgs`` from the command line; what it leaves unset keeps its environment default."""
    h = HipArgs()
    if getattr(args, "hip_devices", None):
        h.devices = [int(x) for x in str(args.hip_devices).split(",") if x != ""]
    for name in ("math", "rows_per_block", "fuse_steps", "cols_per_lane", "no_tune", "kernel", "boundary", "general_kernels",
                 "share_taps", "split", "use_graph", "tile_shape", "pitch_pad", "place_candidates"):
        flag = "hip_" + name
        value = getattr(args, flag, None)
        if value is not None:
            setattr(h, name, value)
    return h


def simulation_parameters(args) -> Parameters:
    """``SharedArgs::simulation_parameters`` (ui/src/lib.rs:51-63)."""
    p = Parameters()
    if args.killrate is not None:
        p.kill_rate = args.killrate
    if args.feedrate is not None:
        p.feed_rate = args.feedrate
    if args.deltat is not None:
        p.time_step = args.deltat
    return p


def run(args, hip_args: HipArgs | None = None, out=None) -> dict:
    steps_per_image = args.nbextrastep if args.nbextrastep is not None else 32
    shape = (args.nbrow, args.nbcol)
    reduce = int(getattr(args, "hip_image_reduce", 1) or 1)
    img_shape = image_shape(args)
    if args.output_buffer < 1:
        raise ValueError("--output-buffer must be at least 1")
    params = simulation_parameters(args)
    pmap = param_map(args, shape, params)
    region = getattr(args, "hip_regions", None)
    regions = RegionLog(region, getattr(args, "hip_region_threshold_v", None), getattr(args, "hip_region_threshold_u", None),
                        getattr(args, "hip_region_corr_lags", None), region_hist_args(args),
                        getattr(args, "hip_region_components", None), getattr(args, "hip_region_change", False),
                        getattr(args, "hip_region_steady_tol", None), region_spectrum_args(args)) if region else None
    mask = domain_mask(args, shape)
    sim = Simulation.new(params, hip_args if hip_args is not None else backend_args(args))
    species = sim.make_species(shape)
    ctx = sim.context
    if pmap is not None:
        sim.set_param_map(pmap[0], pmap[1], shape=shape)
        if getattr(args, "rank", 0) == 0:
            with open(sidecar_path(args.output), "w") as f:
                json.dump(pmap[2], f, indent=1)
    if mask is not None:
        sim.set_mask(mask)
    noise = noise_term(args)
    if noise is not None:   # (with a map or a mask attached the library refuses, and its message says which)
        sim.set_noise(noise[0], noise[1], seed=noise[2], step=noise[3])
    if out is None and args.output.lower().endswith((".h5", ".hdf5")):
        out = hdf5_min.create(args.output, (args.nbimage,) + img_shape)   # dataset "matrix" (hdf5.rs:24)
    elif out is None:
        out = np.lib.format.open_memmap(args.output, mode="w+", dtype=np.float32,
                                        shape=(args.nbimage,) + img_shape)

    # I/O thread: writes images down and recycles their buffers (main.rs:73-87)
    full: "queue.Queue" = queue.Queue(maxsize=args.output_buffer)
    free: "queue.Queue" = queue.Queue()
    for _ in range(args.output_buffer + 2):            # +2: the two images on their way from the device
        free.put(pinned_empty(img_shape))
    errors = []
    failed = threading.Event()

    def writer():
        try:
            index = 0
            while True:
                image = full.get()
                if image is None:
                    return
                out[index] = image
                index += 1
                free.put(image)
        except Exception as e:
            # The reference's main loop fails as soon as the writer is gone (`image_send.send(image)?`,
            # main.rs:120).  Here: flag it, wake a main loop that waits for a buffer, and keep draining
            # so that its full.put() never blocks; the loop below stops at its next iteration.
            errors.append(e)
            failed.set()
            free.put(None)
            while full.get() is not None:
                pass

    ts_every = int(getattr(args, "hip_time_stats_every", 0) or 0)
    ts_threshold = getattr(args, "hip_time_stats_threshold_v", None)
    ts_from = getattr(args, "hip_time_stats_from", None)  # (0 is a step like any other: the initial state)
    ts_at = time_stats_steps(args.nbimage * steps_per_image, ts_every, ts_every if ts_from is None else ts_from)
    stats = species.time_stats(time_stats_groups(ts_threshold), v_threshold=ts_threshold) if ts_at else None
    ts_next, ts_taken, done = 0, [], 0
    if ts_at and ts_at[0] == 0:                             # the initial state is a sample too when asked for
        stats.accumulate(0)
        ts_taken.append(0)
        ts_next = 1

    thread = threading.Thread(target=writer, daemon=True)
    thread.start()
    t0 = time.perf_counter()
    pending = []                                            # images on their way from the device, oldest first (at most 2)
    try:
        for index in range(1, args.nbimage + 1):
            image = free.get()
            if failed.is_set() or image is None:
                break
            if regions is not None and regions_observed(index, args.nbimage, getattr(args, "hip_regions_every", None)):
                regions.before_interval(species, steps_per_image)  # (--hip-region-change: blocking, a device copy)
            if stats is None:
                sim.prepare_steps(species, steps_per_image)  # enqueued; nothing here waits for the device
            else:                                           # the same steps, cut where a sample falls
                end = done + steps_per_image
                while done < end:
                    upto = min(end, ts_at[ts_next]) if ts_next < len(ts_at) else end
                    sim.prepare_steps(species, upto - done)
                    done = upto
                    if ts_next < len(ts_at) and done == ts_at[ts_next]:
                        stats.accumulate(done)              # waits for the steps, enqueues one launch, returns
                        ts_taken.append(done)
                        ts_next += 1
            species.write_result_view_after(image, reduce)  # this image: staged + copied behind those steps while we go on
            pending.append(image)
            if regions is not None and regions_observed(index, args.nbimage, getattr(args, "hip_regions_every", None)):
                # blocking: waits for this image's steps, and so for every image enqueued so far (the module's docstring)
                regions.observe(species, index * steps_per_image)
            if len(pending) == 2:
                # two images in flight (the library stages them in two buffers in turn): the host copy of the newer one
                # overlaps the next steps AND the hand-over of the older one, so the PCIe link never idles between images
                ctx.download_wait(in_flight=1)              # the older image is complete ...
                full.put(pending.pop(0))                    # ... hand it to the I/O thread
        if pending and not failed.is_set():
            ctx.download_wait()
            for image in pending:
                full.put(image)
    finally:
        full.put(None)
        thread.join()
        ctx.sync()
        if regions is not None:
            regions.close()
    elapsed = time.perf_counter() - t0
    if errors:
        raise errors[0]
    if hasattr(out, "flush"):
        out.flush()
    if regions is not None and getattr(args, "rank", 0) == 0:
        regions.save(regions_path(args.output), shape, pmap)
    if stats is not None:
        def read(plane):
            a = plane.make_scalar_view(ctx)
            plane.destroy()
            return a

        planes = time_stats_planes(stats, ts_threshold, read) if stats.samples else {}
        r0, r1 = species.in_out()[0].local_rows()
        write_time_stats(time_stats_path(args.output, ctx.args.rank, ctx.args.world), stats.samples, ts_taken, planes,
                         {"rows": np.array([r0, r1], np.int64), "threshold_v": np.float32(np.nan if ts_threshold is None else ts_threshold)})
        stats.close()
    cells = shape[0] * shape[1]
    image_bytes = img_shape[0] * img_shape[1] * 4          # what really crossed the link per image
    info = {
        "images": args.nbimage, "steps_per_image": steps_per_image, "shape": shape, "seconds": elapsed,
        "mcells_steps_per_s": cells * steps_per_image * args.nbimage / elapsed / 1e6,
        "image_MB_per_s": image_bytes * args.nbimage / elapsed / 1e6,
        "image_reduce": reduce, "image_shape": img_shape, "image_bytes": image_bytes * args.nbimage,
    }
    ctx.close()
    return info


def main(argv=None) -> int:
    args = parse(argv)
    info = run(args)
    reduced = "" if info["image_reduce"] == 1 else (", images reduced by {image_reduce} to {image_shape[0]}x{image_shape[1]}: "
                                                    "{image_bytes} bytes moved".format(**info))
    print("simulate: {images} images x {steps_per_image} steps on {shape[0]}x{shape[1]} in {seconds:.3f} s "
          "({mcells_steps_per_s:.0f} Mcells*steps/s, {image_MB_per_s:.0f} MB/s of images{reduced})".format(reduced=reduced, **info),
          file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
