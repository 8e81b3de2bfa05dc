"""Parameter sweep on the HIP backend: one ensemble member per (feed, kill) pair, all advanced in shared launches
(``gs_ensemble_run``).

    python -m grayscott_amd.sweep --feed 0.01:0.06:8 --kill 0.04:0.07:8 -r 256 -c 512 -s 2000 -o sweep.h5

``--feed A:B:N`` / ``--kill A:B:N`` are N evenly spaced values from A to B (both included).  Members are in kill-major
order: member ``i_kill * N_feed + i_feed``.  Every member starts from ``Species::new``'s pattern and runs ``-s`` steps
with the shared flags of ``simulate`` that still apply (``-r -c -t`` and the ``--hip-*`` group).  Output: the final V of
every member as the dataset ``matrix[members, rows, cols]`` f32 -- the layout the reference's ``simulate`` writes, one
image per member, so its ``data-to-pics`` renders one picture per (F, k) pair -- and a JSON sidecar (``-o``'s name with
``.json``) listing ``index``, ``feed`` and ``kill`` of every member.

``--summary-every N`` also records, every N steps and after the last one, the summaries of every member computed on the
device (``Ensemble.summaries``: sum, sum of squares, min and max of the finite cells, non-finite count, for U and V) into
``<output stem>.summary.npz``: ``steps[samples]`` and ``sum``, ``sum_sq``, ``min``, ``max``, ``nonfinite``, each
``[members, samples, 2]`` (last axis: U, V).  ``--no-fields`` skips the HDF5 file of final V planes (the JSON sidecar
is still written).  Neither changes the states: the HDF5 file is byte for byte the same with or without summaries.

``--histogram-every N`` records, at the same steps (every N steps and after the last one), the histograms of every member
counted on the device (``Ensemble.histograms``; the binning rule is include/gs_hip.h's) into ``<output stem>.hist.npz``:
``steps[samples]``, ``counts[members, samples, 2, bins]`` (axis 2: U, V), ``outside[members, samples, 2, 3]`` (below,
above, nan), ``lo[2]`` and ``hi[2]``.  ``--hist-bins B`` (default 256), ``--hist-range-u A:B`` (default 0:1) and
``--hist-range-v A:B`` (default 0:0.5) set the bins.  It works together with ``--summary-every`` and ``--no-fields`` and
leaves the HDF5 file as it is without it.

``--morphology-every N`` records, at the same steps again, the bit-quad counts of every member's thresholded planes counted
on the device (``Ensemble.morphologies``; the rule is include/gs_hip.h's) -- "spots, stripes or holes?" -- into
``<output stem>.morphology.npz``.  ``--morph-threshold-v A[,B,...]`` (1 to 4 values, required with the flag) thresholds V
from above, ``--morph-threshold-u A[,B,...]`` (as many values; default 0.5 for each) thresholds U from below.  The file holds
``steps[samples]``, ``thresholds_u[nt]``, ``thresholds_v[nt]``, ``quads[samples, members, 2, nt, 6]`` (axis 2: U, V; last
axis: Q0, Q1, Q2, Q3, Q4, QD) and, derived from them, ``area_fraction``, ``perimeter``, ``euler4``, ``euler8``, each
``[samples, members, 2, nt]``.  It changes no state either: the HDF5 file is byte for byte the same without it.

``--correlation-every N`` records, at the same steps again, the two-point pair counts of every member's thresholded planes
counted on the device (``Ensemble.correlations``; the rule is include/gs_hip.h's) -- "how far apart are the spots, which way
do the stripes run?" -- into ``<output stem>.correlation.npz``.  ``--corr-threshold-v A[,B,...]`` (1 to 4 values, required
with the flag) thresholds V from above, ``--corr-threshold-u A[,B,...]`` (as many values; default 0.5 for each) thresholds U
from below, ``--corr-lags L`` (1..64, default 32) is the largest lag.  The file holds ``steps[samples]``,
``thresholds_u[nt]``, ``thresholds_v[nt]``, ``max_lag``, ``shape[2]``, ``pairs[samples, members, 2, nt, 4, L + 1]`` (axis 2: U,
V; axis 4: the unit steps (0, 1), (1, 0), (1, 1), (1, -1); last axis: the lag) and ``pairs_total[4, L + 1]``, the pairs that
exist.  It changes no state either: the HDF5 file is byte for byte the same without it.

``--components-every N`` records, at the same steps again, the connected components of every member's thresholded planes
labelled on the device (``Ensemble.components``; the rule is include/gs_hip.h's) -- "how many spots, how large?" -- into
``<output stem>.components.npz``.  ``--comp-threshold-v A[,B,...]`` (1 to 4 values, required with the flag) thresholds V from
above, ``--comp-threshold-u A[,B,...]`` (as many values; default 0.5 for each) thresholds U from below,
``--comp-connectivity 4|8`` (default 8) says whether cells that share only a corner are neighbours.  The file holds
``steps[samples]``, ``thresholds_u[nt]``, ``thresholds_v[nt]``, ``connectivity``, and ``components``, ``set_cells``, ``largest``,
each ``[samples, members, 2, nt]`` (axis 2: U, V), and ``by_size[samples, members, 2, nt, 32]``.  It changes no state either and
works with ``--no-fields``.

``--spots-every N`` records, at the same steps again, WHERE every member's spots are: one record per connected component of
V above ``--spot-threshold-v T`` (required with the flag) formed on the device (``Ensemble.component_lists``; the rule is
include/gs_hip.h's) -- size, coordinate sums (the centroid), first cell, bounding box -- of the components of at least
``--spot-min-size M`` cells (default 1) under ``--spot-connectivity 4|8`` (default 8), into ``<output stem>.spots.npz``:
``steps[samples]``, ``threshold``, ``connectivity``, ``min_size``, ``offsets[samples * members + 1]`` and ``records``, the
lists one after the other as a structured array -- member m's records at sample s are
``records[offsets[s * members + m] : offsets[s * members + m + 1]]``.  It changes no state either and works with
``--no-fields``.

``--track-every N`` records WHAT BECAME of every member's spots between one sample and the next: a snapshot of the ensemble is
kept on the device (``Ensemble.snapshot``), taken at step 0; after every N steps and after the last one every member's V
above ``--track-threshold-v T`` (required with the flag) is matched with its state at the previous sample on the device
(``Ensemble.matches_since``; the rule is include/gs_hip.h's, gs_fields_match), and the snapshot is brought up to date
(``gs_members_copy``).  Components of at least ``--track-min-size M`` cells (default 1) under ``--track-connectivity 4|8``
(default 8) count.  Into ``<output stem>.tracks.npz``: ``steps[samples]``, ``threshold``, ``connectivity``, ``min_size``, the
five event counts ``continued``, ``split``, ``merged``, ``born``, ``died``, each ``[samples, members]``,
``offsets[samples * members + 1]`` and ``overlaps`` -- member m's overlaps at sample s are
``overlaps[offsets[s * members + m] : offsets[s * members + m + 1]]``, record indices as in a ``.spots.npz`` taken at the same
steps with the same rule --, and ``displacement_offsets`` and ``displacements[k, 2]`` (float64; after centroid minus before
centroid of the continued pairs) laid out the same way.  It changes no state either and works with ``--no-fields``.

``--steady-every N`` asks of every member "has it stopped changing?".  A snapshot of the ensemble is kept on the device
(``Ensemble.snapshot``), taken at step 0; after every N steps and after the last one every member is compared with it on the
device (``Ensemble.changes_since``: with d = now - snapshot per cell in f64, the sum of |d|, the sum of d * d and the largest
|d| over the cells finite in both, the count of cells whose bits differ and of cells not finite, for U and V), then the
snapshot is brought up to date (``gs_members_copy``).  The records go to ``<output stem>.steady.npz``: ``steps[samples]``,
``max_abs``, ``sum_abs``, ``sum_sq``, ``differing``, ``nonfinite``, each ``[members, samples, 2]`` (last axis: U, V), and
``settled_step[members]``: the first sampled step at which ``max_abs <= T`` held for both U and V, else -1, with T from
``--steady-tol T`` (default 0: not one bit's worth of change in value).  The flags merge with the sampling loop of
``--summary-every`` and ``--histogram-every`` and change no state: the HDF5 file is byte for byte the same with and without
them.  ``--steady-stop`` ends the run after the first check at which EVERY member is settled: the JSON sidecar's ``steps``
is then the number of steps taken, and (with or without an early end) its member list carries each member's
``settled_step``.  What the rule cannot see: it compares states N steps apart, so a pattern whose period divides N --
an oscillating spot, a rotating spiral that returns onto itself -- looks steady; choose N that is no multiple of a period
you expect, or run twice with coprime N.  Without ``--steady-retire`` members do not stop one by one: all advance until
all have settled (or to the last step).

``--steady-retire`` (needs ``--steady-every``) stops them one by one: after each check every member with ``max_abs <= T``
for both U and V is retired (``Ensemble.set_active``) -- it keeps its state, the launches that follow cover the other
members only, and the run ends when no member is active or the steps are used up.  The snapshot is brought up to date and
the records go on as before: a retired member equals its snapshot, so its later records are zeros, and ``settled_step``
keeps its meaning.  The JSON sidecar then carries ``steps_taken`` per member and its top-level ``steps`` is their maximum;
``<stem>.steady.npz`` gains ``steps_taken[members]``; the HDF5 file holds each member's V after its own ``steps_taken``
steps -- bit for bit what that member is after as many steps in a run without the flag.  Without the flag every output file is
what it was.

``--time-stats-every N`` keeps per-cell statistics over time on the device (``Ensemble.time_stats``): U and V of every member
are sampled every N steps -- from step S on with ``--time-stats-from S`` (default N), at steps S, S + N, ... -- into
accumulators that never leave the device, and ``<output stem>.timestats.npz`` receives ``samples``, ``steps`` and, per member,
the scalars ``var_v_mean``, ``var_v_max`` (0 for a member that stands still, not for one that pulsates or wanders) and
``mean_v_mean``; unless ``--no-fields`` is given also the planes ``mean_v``, ``var_v``, ``min_v``, ``max_v`` (and ``_u``), each
``[members, rows, cols]`` f32, and with ``--time-stats-threshold-v T`` ``occupancy_v`` and ``arrival_v``.  Retired members are
sampled like the others: they repeat their state.

``--spectrum-every N`` records, at the steps of ``--summary-every`` again (every N steps and after the last one), the
tile-averaged power spectra of every member summed on the device (``Ensemble.spectra``; the rule is include/gs_hip.h's) --
"what is the pattern's wavelength?", with no threshold -- into ``<output stem>.spectrum.npz``.  ``--spectrum-tile T`` (16, 32,
64 or 128; default 64) is the tile's side, ``--spectrum-window hann|none`` (default hann) the window.  The file holds
``steps[samples]``, ``tile``, ``window``, ``power[samples, members, 2, T, T/2 + 1]`` (axis 2: U, V; the raw f64 sums),
``tiles[samples, members, 2, 2]`` (last axis: tiles used, tiles skipped) and ``wavelength[samples, members, 2]`` in cells
(``Spectrum.wavelength``; NaN for a flat spectrum).  It changes no state either and works with ``--no-fields``.

``--noise SU[:SV]`` makes the run stochastic (``Ensemble.set_noise``; the definition is include/gs_hip.h's): every step adds
``SU * xi`` to U and ``SV * xi`` to V (SV defaults to 0), ``xi`` uniform on [-1, 1).  ``--realisations R`` (default 1) turns
every (feed, kill) point into R members: member ``point * R + r``, ``point`` in the kill-major order above, runs with seed
``N + r``, ``N`` from ``--noise-seed N`` (default 0), from step 0.  The same seeds at every point are deliberate: common
random numbers across the map, so that neighbouring points differ by their parameters and not by their draws.  A run is
reproducible to the byte.  The JSON sidecar gains ``realisation`` and ``noise_seed`` per member and ``noise`` (sigma_u,
sigma_v, seed, realisations) at top level.  ``--realisations`` above 1 needs ``--noise``.  ``--steady-retire`` and every
``--*-every`` observable work on noisy members as they are: a retired member keeps its step counter.  Without the three flags
every output file is byte for byte what it was.

``--bundle-stats`` forms, after the last step, the ensemble average of every (feed, kill) point on the device
(``Ensemble.bundle_stats``; the definition is include/gs_hip.h's): the ``--realisations R`` members of a point are a bundle, and
``<output stem>.bundles.npz`` receives ``mean_u``, ``mean_v``, ``variance_u``, ``variance_v``, ``min_v`` and ``max_v``, each
``[points, rows, cols]`` f32 with the points in the kill-major order above -- the per-cell statistics across the realisations --
and ``feed[points]``, ``kill[points]`` and ``span`` (= R).  ``--bundle-threshold-v T`` adds ``occupancy_v``, the share of the
realisations in which the cell's V is above T: the probability that it lies inside a spot.  Retired members count with the
state they hold.  It works with ``--no-fields``, the JSON sidecar names the file under ``bundle_stats``, and without the flag
every output file is byte for byte what it was.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from typing import List, Tuple

import numpy as np

from . import hdf5_min
from .simulate import (add_backend_args, add_time_stats_args, backend_args, check_time_stats_args, time_stats_groups,
                       time_stats_planes, time_stats_steps)
from .simulation import (COMPONENT_OVERLAP_DTYPE, COMPONENT_RECORD_DTYPE, SPECTRUM_TILES, SPECTRUM_WINDOWS, Parameters, Simulation,
                         Spectrum, pairs_total, quad_measures)


def value_range(text: str) -> List[float]:
    """``A:B:N`` -> N evenly spaced values from A to B (N = 1: A alone)."""
    parts = text.split(":")
    if len(parts) != 3:
        raise argparse.ArgumentTypeError(f"expected A:B:N, got {text!r}")
    a, b, n = float(parts[0]), float(parts[1]), int(parts[2])
    if n < 1:
        raise argparse.ArgumentTypeError(f"N must be at least 1 in {text!r}")
    return [a] if n == 1 else [float(x) for x in np.linspace(a, b, n)]


def value_pair(text: str) -> Tuple[float, float]:
    """``A:B`` -> (A, B) with A < B."""
    parts = text.split(":")
    if len(parts) != 2:
        raise argparse.ArgumentTypeError(f"expected A:B, got {text!r}")
    a, b = float(parts[0]), float(parts[1])
    if not a < b:
        raise argparse.ArgumentTypeError(f"A must be below B in {text!r}")
    return a, b


def sigma_pair(text: str) -> Tuple[float, float]:
    """``SU[:SV]`` -> (SU, SV): two finite sigmas, none below 0; SV defaults to 0."""
    parts = text.split(":")
    try:
        out = [float(x) for x in parts]
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected SU[:SV], got {text!r}")
    if not 1 <= len(out) <= 2 or not all(0.0 <= x < float("inf") for x in out):
        raise argparse.ArgumentTypeError(f"one or two finite sigmas that are at least 0, got {text!r}")
    return out[0], (out[1] if len(out) == 2 else 0.0)


def threshold_list(text: str) -> List[float]:
    """``A[,B,...]`` -> 1 to 4 thresholds, none of them NaN."""
    try:
        out = [float(x) for x in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected A[,B,...], got {text!r}")
    if not 1 <= len(out) <= 4 or any(x != x for x in out):
        raise argparse.ArgumentTypeError(f"1 to 4 thresholds that are numbers, got {text!r}")
    return out


# The thresholded observables, in the order their flags are checked: (name of --NAME-every, prefix of --PREFIX-threshold-v / -u).
THRESHOLDED = (("components", "comp"), ("morphology", "morph"), ("correlation", "corr"))


def parse(argv=None):
    ap = argparse.ArgumentParser(prog="sweep", description="Gray-Scott parameter sweep, one ensemble member per (feed, kill) "
                                                           "-- with --noise, --realisations of them")
    ap.add_argument("--feed", type=value_range, required=True, metavar="A:B:N", help="feed rates")
    ap.add_argument("--kill", type=value_range, required=True, metavar="A:B:N", help="kill rates")
    ap.add_argument("-s", "--steps", type=int, default=1000, help="steps per member")
    ap.add_argument("-r", "--nbrow", type=int, default=1080)
    ap.add_argument("-c", "--nbcol", type=int, default=1920)
    ap.add_argument("-t", "--deltat", type=float, default=None)
    ap.add_argument("-o", "--output", default="sweep.h5")
    ap.add_argument("--summary-every", type=int, default=0, metavar="N",
                    help="record every member's summaries every N steps and at the end (<output stem>.summary.npz)")
    ap.add_argument("--no-fields", action="store_true", help="do not write the HDF5 file of final V planes")
    ap.add_argument("--histogram-every", type=int, default=0, metavar="N",
                    help="record every member's histograms every N steps and at the end (<output stem>.hist.npz)")
    ap.add_argument("--hist-bins", type=int, default=256, metavar="B", help="bins of the histograms (1..4096)")
    ap.add_argument("--hist-range-u", type=value_pair, default=(0.0, 1.0), metavar="A:B", help="range of U's histogram")
    ap.add_argument("--hist-range-v", type=value_pair, default=(0.0, 0.5), metavar="A:B", help="range of V's histogram")
    ap.add_argument("--morphology-every", type=int, default=0, metavar="N",
                    help="record every member's bit-quad counts every N steps and at the end (<output stem>.morphology.npz)")
    ap.add_argument("--components-every", type=int, default=0, metavar="N",
                    help="record every member's connected components every N steps and at the end (<output stem>.components.npz)")
    ap.add_argument("--comp-threshold-v", type=threshold_list, default=None, metavar="A[,B,...]",
                    help="1 to 4 thresholds above which a V cell is set (required with --components-every)")
    ap.add_argument("--comp-threshold-u", type=threshold_list, default=None, metavar="A[,B,...]",
                    help="as many thresholds below which a U cell is set (default 0.5 for each)")
    ap.add_argument("--comp-connectivity", type=int, default=8, choices=(4, 8),
                    help="cells are neighbours across a side (4) or also across a corner (8, the default)")
    ap.add_argument("--spots-every", type=int, default=0, metavar="N",
                    help="record every member's component list of V every N steps and at the end (<output stem>.spots.npz)")
    ap.add_argument("--spot-threshold-v", type=float, default=None, metavar="T",
                    help="the threshold above which a V cell is set (required with --spots-every)")
    ap.add_argument("--spot-min-size", type=int, default=1, metavar="M", help="list the components of at least M cells (default 1)")
    ap.add_argument("--spot-connectivity", type=int, default=8, choices=(4, 8),
                    help="cells are neighbours across a side (4) or also across a corner (8, the default)")
    ap.add_argument("--morph-threshold-v", type=threshold_list, default=None, metavar="A[,B,...]",
                    help="1 to 4 thresholds: V is set where it is above them")
    ap.add_argument("--morph-threshold-u", type=threshold_list, default=None, metavar="A[,B,...]",
                    help="as many thresholds: U is set where it is below them (default 0.5 each)")
    ap.add_argument("--correlation-every", type=int, default=0, metavar="N",
                    help="record every member's two-point pair counts every N steps and at the end "
                         "(<output stem>.correlation.npz)")
    ap.add_argument("--corr-threshold-v", type=threshold_list, default=None, metavar="A[,B,...]",
                    help="1 to 4 thresholds: V is set where it is above them")
    ap.add_argument("--corr-threshold-u", type=threshold_list, default=None, metavar="A[,B,...]",
                    help="as many thresholds: U is set where it is below them (default 0.5 each)")
    ap.add_argument("--corr-lags", type=int, default=32, metavar="L", help="the largest lag (1..64)")
    ap.add_argument("--track-every", type=int, default=0, metavar="N",
                    help="match every member's components of V with those of the previous sample every N steps and at the end "
                         "(<output stem>.tracks.npz)")
    ap.add_argument("--track-threshold-v", type=float, default=None, metavar="T",
                    help="the threshold above which a V cell is set (required with --track-every)")
    ap.add_argument("--track-min-size", type=int, default=1, metavar="M", help="match the components of at least M cells (default 1)")
    ap.add_argument("--track-connectivity", type=int, default=8, choices=(4, 8),
                    help="4: cells join along edges; 8: also across corners (default 8)")
    ap.add_argument("--steady-every", type=int, default=0, metavar="N",
                    help="compare every member with its state N steps before, every N steps and at the end "
                         "(<output stem>.steady.npz)")
    ap.add_argument("--steady-tol", type=float, default=0.0, metavar="T",
                    help="a member is settled when max |change| over N steps is at most T for U and V (default 0)")
    ap.add_argument("--steady-stop", action="store_true", help="end the run once every member is settled")
    ap.add_argument("--steady-retire", action="store_true",
                    help="retire every member at the check that finds it settled: it keeps its state and stops advancing")
    ap.add_argument("--spectrum-every", type=int, default=0, metavar="N",
                    help="record every member's power spectra every N steps and at the end (<output stem>.spectrum.npz)")
    ap.add_argument("--spectrum-tile", type=int, default=64, choices=SPECTRUM_TILES, metavar="T",
                    help="the side of the spectra's tiles: 16, 32, 64 (the default) or 128 cells")
    ap.add_argument("--spectrum-window", default="hann", choices=sorted(SPECTRUM_WINDOWS),
                    help="the window of a tile: hann (periodic Hann, the default) or none")
    ap.add_argument("--noise", type=sigma_pair, default=None, metavar="SU[:SV]",
                    help="per-step noise amplitudes of U and V (SV defaults to 0): every member runs with noise")
    ap.add_argument("--noise-seed", type=int, default=0, metavar="N", help="realisation r of every point runs with seed N + r (default 0)")
    ap.add_argument("--realisations", type=int, default=1, metavar="R",
                    help="members per (feed, kill) point, each with its own seed (default 1; more need --noise)")
    ap.add_argument("--bundle-stats", action="store_true",
                    help="after the last step, per-cell mean, variance and range across the --realisations of every point "
                         "(<output stem>.bundles.npz)")
    ap.add_argument("--bundle-threshold-v", type=float, default=None, metavar="T",
                    help="with --bundle-stats: also the share of a point's realisations in which V is above T (occupancy_v)")
    add_time_stats_args(ap, "--time-stats")
    add_backend_args(ap)
    args = ap.parse_args(argv)
    if args.bundle_threshold_v is not None and not args.bundle_stats:
        ap.error("--bundle-threshold-v needs --bundle-stats")
    if args.bundle_threshold_v is not None and args.bundle_threshold_v != args.bundle_threshold_v:
        ap.error("--bundle-threshold-v must be a number")
    if args.realisations < 1:
        ap.error("--realisations must be at least 1")
    if args.realisations > 1 and args.noise is None:
        ap.error("--realisations above 1 needs --noise: without it the members of a point would be copies")
    if args.spectrum_every < 0:
        ap.error("--spectrum-every must be at least 1 (0 = off)")
    check_time_stats_args(ap, args, "time_stats", "--time-stats")
    if args.steady_every < 0:
        ap.error("--steady-every must be at least 1 (0 = off)")
    if not args.steady_tol >= 0.0:
        ap.error("--steady-tol must be at least 0")
    if args.steady_stop and not args.steady_every:
        ap.error("--steady-stop needs --steady-every")
    if args.steady_retire and not args.steady_every:
        ap.error("--steady-retire needs --steady-every")
    if args.summary_every < 0:
        ap.error("--summary-every must be at least 1 (0 = off)")
    if args.histogram_every < 0:
        ap.error("--histogram-every must be at least 1 (0 = off)")
    if not 1 <= args.hist_bins <= 4096:
        ap.error("--hist-bins must be in 1..4096")
    for name, short in THRESHOLDED:
        every, tv, tu = (getattr(args, f"{name}_every"), getattr(args, f"{short}_threshold_v"),
                         getattr(args, f"{short}_threshold_u"))
        if every < 0:
            ap.error(f"--{name}-every must be at least 1 (0 = off)")
        if every and tv is None:
            ap.error(f"--{name}-every needs --{short}-threshold-v")
        if tu is None and tv is not None:
            tu = [0.5] * len(tv)
            setattr(args, f"{short}_threshold_u", tu)
        if tv is not None and len(tu) != len(tv):
            ap.error(f"--{short}-threshold-u needs as many values as --{short}-threshold-v")
    if not 1 <= args.corr_lags <= 64:
        ap.error("--corr-lags must be in 1..64")
    if args.track_every < 0:
        ap.error("--track-every must be at least 1 (0 = off)")
    if args.track_every and args.track_threshold_v is None:
        ap.error("--track-every needs --track-threshold-v")
    if args.track_threshold_v is not None and args.track_threshold_v != args.track_threshold_v:
        ap.error("--track-threshold-v must be a number")
    if args.track_min_size < 1:
        ap.error("--track-min-size must be at least 1")
    if args.spots_every < 0:
        ap.error("--spots-every must be at least 1 (0 = off)")
    if args.spots_every and args.spot_threshold_v is None:
        ap.error("--spots-every needs --spot-threshold-v")
    if args.spot_threshold_v is not None and args.spot_threshold_v != args.spot_threshold_v:
        ap.error("--spot-threshold-v must be a number")
    if args.spot_min_size < 1:
        ap.error("--spot-min-size must be at least 1")
    return args


def members(args) -> List[Tuple[int, float, float]]:
    """(index, feed, kill) of every member: the points kill-major, ``--realisations`` members per point side by side."""
    reps = getattr(args, "realisations", 1)
    return [((i * len(args.feed) + j) * reps + r, f, k) for i, k in enumerate(args.kill) for j, f in enumerate(args.feed)
            for r in range(reps)]


def member_seeds(args) -> List[Tuple[int, int]]:
    """(realisation, seed) of every member, in the order of ``members``: realisation r of every point has seed
    ``--noise-seed`` + r (modulo 2^64) -- common random numbers across the map."""
    reps = getattr(args, "realisations", 1)
    return [(i % reps, (args.noise_seed + i % reps) & 0xFFFFFFFFFFFFFFFF) for i in range(len(args.feed) * len(args.kill) * reps)]


def member_params(args) -> List[Parameters]:
    out = []
    for _, feed, kill in members(args):
        p = Parameters(feed_rate=feed, kill_rate=kill)
        if args.deltat is not None:
            p.time_step = args.deltat
        out.append(p)
    return out


def sidecar_path(output: str) -> str:
    return os.path.splitext(output)[0] + ".json"


def summary_path(output: str) -> str:
    return os.path.splitext(output)[0] + ".summary.npz"


def hist_path(output: str) -> str:
    return os.path.splitext(output)[0] + ".hist.npz"


def morphology_path(output: str) -> str:
    return os.path.splitext(output)[0] + ".morphology.npz"


def correlation_path(output: str) -> str:
    return os.path.splitext(output)[0] + ".correlation.npz"


def steady_path(output: str) -> str:
    return os.path.splitext(output)[0] + ".steady.npz"


def time_stats_path(output: str) -> str:
    return os.path.splitext(output)[0] + ".timestats.npz"


def bundles_path(output: str) -> str:
    return os.path.splitext(output)[0] + ".bundles.npz"


BUNDLE_PLANES = (("mean", "u"), ("mean", "v"), ("variance", "u"), ("variance", "v"), ("min", "v"), ("max", "v"))


def bundle_results(threshold_v) -> Tuple[str, ...]:
    """The results ``--bundle-stats`` asks ``Ensemble.bundle_stats`` for."""
    return ("mean", "variance", "min", "max") + (("occupancy",) if threshold_v is not None else ())


def write_bundles(path: str, results: dict, threshold_v, feed, kill, span: int, view) -> None:
    """``results``: {name: what holds the planes of every point}; ``view(x, species)`` reads them as ``[points, rows, cols]``."""
    planes = BUNDLE_PLANES + ((("occupancy", "v"),) if threshold_v is not None else ())
    out = {f"{name}_{species}": np.asarray(view(results[name], species), np.float32) for name, species in planes}
    out.update(feed=np.asarray(feed, np.float64), kill=np.asarray(kill, np.float64), span=np.int64(span))
    with open(path, "wb") as f:
        np.savez(f, **out)


def write_time_stats(path: str, samples: int, steps: List[int], planes: dict, with_planes: bool) -> None:
    """``planes``: {"mean_v": [members, rows, cols], ...}.  Per member the scalars ``var_v_mean`` and ``var_v_max`` (a member
    whose V stands still has both 0, one that pulsates or wanders does not) and ``mean_v_mean``, in float64; with
    ``with_planes`` the planes themselves too."""
    out = {"samples": np.int64(samples), "steps": np.asarray(steps, np.int64)}
    if samples:
        out["var_v_mean"] = planes["var_v"].mean(axis=(1, 2), dtype=np.float64)
        out["var_v_max"] = planes["var_v"].max(axis=(1, 2)).astype(np.float64)
        out["mean_v_mean"] = planes["mean_v"].mean(axis=(1, 2), dtype=np.float64)
        if with_planes:
            out.update(planes)
    with open(path, "wb") as f:
        np.savez(f, **out)


def sample_steps(steps: int, every: int) -> List[int]:
    """Steps after which the summaries are taken: every ``every`` steps and after the last one."""
    out = list(range(every, steps + 1, every))
    if not out or out[-1] != steps:
        out.append(steps)
    return out


def write_summaries(path: str, steps: List[int], samples: List[np.ndarray]) -> None:
    rec = np.stack(samples, axis=1)  # [members, samples, 2] of SUMMARY_DTYPE
    np.savez(path, steps=np.asarray(steps, np.int64),
             **{name: np.ascontiguousarray(rec[name]) for name in rec.dtype.names})


def write_histograms(path: str, steps: List[int], samples: List[np.ndarray], u_range, v_range) -> None:
    h = np.stack(samples, axis=1)  # [members, samples, 2, bins + 3]
    np.savez(path, steps=np.asarray(steps, np.int64), counts=np.ascontiguousarray(h[..., :-3]),
             outside=np.ascontiguousarray(h[..., -3:]), lo=np.asarray([u_range[0], v_range[0]], np.float32),
             hi=np.asarray([u_range[1], v_range[1]], np.float32))


def components_path(output: str) -> str:
    return os.path.splitext(output)[0] + ".components.npz"


def write_components(path: str, steps: List[int], samples: List[np.ndarray], thresholds_u, thresholds_v, connectivity: int) -> None:
    c = np.stack(samples, axis=0)  # [samples, members, 2, nt, 35]: components, set_cells, largest, by_size[32]
    np.savez(path, steps=np.asarray(steps, np.int64), thresholds_u=np.asarray(thresholds_u, np.float32),
             thresholds_v=np.asarray(thresholds_v, np.float32), connectivity=np.int64(connectivity),
             components=np.ascontiguousarray(c[..., 0]), set_cells=np.ascontiguousarray(c[..., 1]),
             largest=np.ascontiguousarray(c[..., 2]), by_size=np.ascontiguousarray(c[..., 3:]))


def spots_path(output: str) -> str:
    return os.path.splitext(output)[0] + ".spots.npz"


def write_spots(path: str, steps: List[int], samples: List[list], threshold: float, connectivity: int, min_size: int) -> None:
    lists = [member for sample in samples for member in sample]  # [samples * members] of ComponentList
    offsets = np.zeros(len(lists) + 1, np.int64)
    offsets[1:] = np.cumsum([c.count for c in lists])
    records = np.concatenate([c.records for c in lists]) if lists else np.zeros(0, COMPONENT_RECORD_DTYPE)
    np.savez(path, steps=np.asarray(steps, np.int64), threshold=np.float32(threshold), connectivity=np.int64(connectivity),
             min_size=np.int64(min_size), offsets=offsets, records=records)


def tracks_path(output: str) -> str:
    return os.path.splitext(output)[0] + ".tracks.npz"


def write_tracks(path: str, steps: List[int], samples: List[list], threshold: float, connectivity: int, min_size: int) -> None:
    matches = [member for sample in samples for member in sample]  # [samples * members] of ComponentMatch
    members = len(samples[0]) if samples else 0
    offsets = np.zeros(len(matches) + 1, np.int64)
    offsets[1:] = np.cumsum([m.overlaps.shape[0] for m in matches])
    moves = [m.displacements() for m in matches]
    move_offsets = np.zeros(len(matches) + 1, np.int64)
    move_offsets[1:] = np.cumsum([d.shape[0] for d in moves])
    counts = [m.counts() for m in matches]
    events = {name: np.array([c[name] for c in counts], np.int64).reshape(len(samples), members)
              for name in ("continued", "split", "merged", "born", "died")}
    np.savez(path, steps=np.asarray(steps, np.int64), threshold=np.float32(threshold), connectivity=np.int64(connectivity),
             min_size=np.int64(min_size), offsets=offsets,
             overlaps=np.concatenate([m.overlaps for m in matches]) if matches else np.zeros(0, COMPONENT_OVERLAP_DTYPE),
             displacement_offsets=move_offsets,
             displacements=np.concatenate(moves).reshape(-1, 2) if moves else np.zeros((0, 2), np.float64), **events)


def write_morphologies(path: str, steps: List[int], samples: List[np.ndarray], thresholds_u, thresholds_v, cells: int) -> None:
    q = np.stack(samples, axis=0)  # [samples, members, 2, nt, 6]
    area, perimeter, euler4, euler8 = quad_measures(q)
    np.savez(path, steps=np.asarray(steps, np.int64), thresholds_u=np.asarray(thresholds_u, np.float32),
             thresholds_v=np.asarray(thresholds_v, np.float32), quads=np.ascontiguousarray(q),
             area_fraction=area / cells if cells else np.full(area.shape, np.nan), perimeter=perimeter, euler4=euler4,
             euler8=euler8)


def write_correlations(path: str, steps: List[int], samples: List[np.ndarray], thresholds_u, thresholds_v, max_lag: int,
                       shape) -> None:
    np.savez(path, steps=np.asarray(steps, np.int64), thresholds_u=np.asarray(thresholds_u, np.float32),
             thresholds_v=np.asarray(thresholds_v, np.float32), max_lag=np.int64(max_lag), shape=np.asarray(shape, np.int64),
             pairs=np.ascontiguousarray(np.stack(samples, axis=0)), pairs_total=pairs_total(shape[0], shape[1], max_lag))


def spectrum_path(output: str) -> str:
    return os.path.splitext(output)[0] + ".spectrum.npz"


def write_spectra(path: str, steps: List[int], samples: List[tuple], tile: int, window: str) -> None:
    power = np.stack([p for p, _ in samples], axis=0)  # [samples, members, 2, T, T/2 + 1]
    tiles = np.stack([t for _, t in samples], axis=0)  # [samples, members, 2, 2]
    wavelength = np.full(power.shape[:3], np.nan)
    for at in np.ndindex(wavelength.shape):
        found = Spectrum.from_raw(power[at], tile, window, tiles[at]).wavelength()
        if found is not None:
            wavelength[at] = found
    np.savez(path, steps=np.asarray(steps, np.int64), tile=np.int64(tile), window=np.str_(window), power=power, tiles=tiles,
             wavelength=wavelength)


def settled_steps(steps: List[int], max_abs: np.ndarray, tol: float) -> np.ndarray:
    """``settled_step[members]``: the first of ``steps`` at which ``max_abs[member, sample]`` is at most ``tol`` for both U
    and V, else -1.  ``max_abs``: ``[members, samples, 2]``."""
    ok = np.all(max_abs <= tol, axis=2)
    first = np.argmax(ok, axis=1)
    at = np.asarray(steps, np.int64)
    return np.where(ok.any(axis=1), at[first] if len(at) else -1, -1).astype(np.int64)


def retire_mask(changes: np.ndarray, tol: float) -> np.ndarray:
    """``bool[members]``: the members one steady check finds settled -- ``max_abs <= tol`` for both U and V.  ``changes``:
    the ``[members, 2]`` record of ``Ensemble.changes_since``.  (A NaN ``tol`` or ``max_abs`` settles nobody.)"""
    return np.all(changes["max_abs"] <= tol, axis=1)


def write_steady(path: str, steps: List[int], samples: List[np.ndarray], tol: float, steps_taken=None) -> np.ndarray:
    rec = np.stack(samples, axis=1)  # [members, samples, 2] of CHANGE_DTYPE
    settled = settled_steps(steps, rec["max_abs"], tol)
    extra = {} if steps_taken is None else {"steps_taken": np.asarray(steps_taken, np.int64)}
    np.savez(path, steps=np.asarray(steps, np.int64), settled_step=settled,
             **{name: np.ascontiguousarray(rec[name]) for name in rec.dtype.names}, **extra)
    return settled


def run(args) -> dict:
    if args.steps < 0:
        raise ValueError("--steps must be at least 0")
    shape = (args.nbrow, args.nbcol)
    params = member_params(args)
    sim = Simulation.new(params[0], backend_args(args))
    ens = sim.make_ensemble(shape, params)
    if args.noise is not None:
        ens.set_noise(args.noise[0], args.noise[1], seed=np.array([seed for _, seed in member_seeds(args)], np.uint64))
    t0 = time.perf_counter()
    summary_at = sample_steps(args.steps, args.summary_every) if args.summary_every else []
    hist_at = sample_steps(args.steps, args.histogram_every) if args.histogram_every else []
    steady_at = sample_steps(args.steps, args.steady_every) if args.steady_every else []
    morph_at = sample_steps(args.steps, args.morphology_every) if args.morphology_every else []
    corr_at = sample_steps(args.steps, args.correlation_every) if args.correlation_every else []
    comp_at = sample_steps(args.steps, args.components_every) if args.components_every else []
    spots_at = sample_steps(args.steps, args.spots_every) if args.spots_every else []
    track_at = sample_steps(args.steps, args.track_every) if args.track_every else []
    spec_at = sample_steps(args.steps, args.spectrum_every) if args.spectrum_every else []
    tstat_at = time_stats_steps(args.steps, args.time_stats_every, args.time_stats_from)
    stats = ens.time_stats(time_stats_groups(args.time_stats_threshold_v), v_threshold=args.time_stats_threshold_v) if tstat_at else None
    tstat_taken = []
    if tstat_at and tstat_at[0] == 0:
        stats.accumulate(0)
        tstat_taken.append(0)
    done, settled, taken = 0, None, None
    if summary_at or hist_at or steady_at or morph_at or corr_at or comp_at or spots_at or track_at or tstat_at or spec_at:
        summaries, hists, changes, morphs, corrs, comps, spots, tracks, spectra = [], [], [], [], [], [], [], [], []
        snap = ens.snapshot() if steady_at else None
        last = ens.snapshot() if track_at else None  # (of its own: the steady checks move theirs at other steps)
        for at in sorted(set(summary_at) | set(hist_at) | set(steady_at) | set(morph_at) | set(corr_at) | set(comp_at)
                         | set(spots_at) | set(track_at) | set(spec_at) | set(tstat_at) | ({args.steps} if tstat_at else set())):
            ens.prepare_steps(at - done)
            done = at
            if at in tstat_at and at not in tstat_taken:
                stats.accumulate(at)  # (waits for the steps; the accumulators stay on the device)
                tstat_taken.append(at)
            if at in summary_at:
                summaries.append(ens.summaries())  # (waits for the steps)
            if at in hist_at:
                hists.append(ens.histograms(bins=args.hist_bins, u_range=args.hist_range_u, v_range=args.hist_range_v))
            if at in morph_at:
                morphs.append(ens.morphologies(v_thresholds=args.morph_threshold_v, u_thresholds=args.morph_threshold_u))
            if at in comp_at:
                comps.append(ens.components(v_thresholds=args.comp_threshold_v, u_thresholds=args.comp_threshold_u,
                                            connectivity=args.comp_connectivity))
            if at in spots_at:
                spots.append(ens.component_lists(species="v", threshold=args.spot_threshold_v, connectivity=args.spot_connectivity,
                                                 min_size=args.spot_min_size))
            if at in track_at:
                tracks.append(ens.matches_since(last, species="v", threshold=args.track_threshold_v,
                                                connectivity=args.track_connectivity, min_size=args.track_min_size))
                last.copy_from(ens)
            if at in corr_at:
                corrs.append(ens.correlations(v_thresholds=args.corr_threshold_v, u_thresholds=args.corr_threshold_u,
                                              max_lag=args.corr_lags))
            if at in spec_at:
                spectra.append(ens.spectra(tile=args.spectrum_tile, window=args.spectrum_window))
            if at in steady_at:
                changes.append(ens.changes_since(snap))
                snap.copy_from(ens)
                if args.steady_retire:
                    resting = retire_mask(changes[-1], args.steady_tol)
                    if np.any(resting & ens.active()):
                        ens.set_active(~resting)  # (a retired member equals its snapshot: it stays in the mask)
                    if resting.all():
                        break
                if args.steady_stop and np.all(settled_steps(steady_at[:len(changes)], np.stack(changes, axis=1)["max_abs"],
                                                             args.steady_tol) >= 0):
                    break
        if summary_at:
            write_summaries(summary_path(args.output), summary_at[:len(summaries)], summaries)
        if hist_at:
            write_histograms(hist_path(args.output), hist_at[:len(hists)], hists, args.hist_range_u, args.hist_range_v)
        if morph_at:
            write_morphologies(morphology_path(args.output), morph_at[:len(morphs)], morphs, args.morph_threshold_u,
                               args.morph_threshold_v, shape[0] * shape[1])
        if comp_at:
            write_components(components_path(args.output), comp_at[:len(comps)], comps, args.comp_threshold_u,
                             args.comp_threshold_v, args.comp_connectivity)
        if spots_at:
            write_spots(spots_path(args.output), spots_at[:len(spots)], spots, args.spot_threshold_v, args.spot_connectivity,
                        args.spot_min_size)
        if track_at:
            write_tracks(tracks_path(args.output), track_at[:len(tracks)], tracks, args.track_threshold_v, args.track_connectivity,
                         args.track_min_size)
            last.destroy()
        if corr_at:
            write_correlations(correlation_path(args.output), corr_at[:len(corrs)], corrs, args.corr_threshold_u,
                               args.corr_threshold_v, args.corr_lags, shape)
        if spec_at:
            write_spectra(spectrum_path(args.output), spec_at[:len(spectra)], spectra, args.spectrum_tile, args.spectrum_window)
        if tstat_at:
            planes = time_stats_planes(stats, args.time_stats_threshold_v, lambda a: a) if stats.samples else {}
            write_time_stats(time_stats_path(args.output), stats.samples, tstat_taken, planes, not args.no_fields)
            stats.close()
        if steady_at:
            if args.steady_retire:
                sim.context.sync()
                taken = ens.steps_taken()
                done = int(taken.max())
            settled = write_steady(steady_path(args.output), steady_at[:len(changes)], changes, args.steady_tol, taken)
            snap.destroy()
    else:
        ens.perform_steps(args.steps)
        done = args.steps
    elapsed = time.perf_counter() - t0
    if args.bundle_stats:
        results = ens.bundle_stats(args.realisations, bundle_results(args.bundle_threshold_v), v_threshold=args.bundle_threshold_v)
        points = members(args)[::args.realisations]
        write_bundles(bundles_path(args.output), results, args.bundle_threshold_v, [f for _, f, _ in points],
                      [k for _, _, k in points], args.realisations,
                      lambda e, species: e.u_views() if species == "u" else e.result_views())
        for e in results.values():
            e.destroy()
    if not args.no_fields:
        out = hdf5_min.create(args.output, (len(params),) + shape)
        per_chunk = max(1, (256 << 20) // (4 * shape[0] * shape[1]))  # download in pieces of ~256 MB
        for first in range(0, len(params), per_chunk):
            count = min(per_chunk, len(params) - first)
            out[first:first + count] = ens.result_views(first, count)
        out.flush()
        del out
    with open(sidecar_path(args.output), "w") as f:
        listed = [{"index": i, "feed": feed, "kill": kill} for i, feed, kill in members(args)]
        if settled is not None:
            for m in listed:
                m["settled_step"] = int(settled[m["index"]])
        if taken is not None:
            for m in listed:
                m["steps_taken"] = int(taken[m["index"]])
        top = {"shape": list(shape), "steps": done, "members": listed}
        if args.noise is not None:
            for m, (r, seed) in zip(listed, member_seeds(args)):
                m["realisation"], m["noise_seed"] = r, seed
            top["noise"] = {"sigma_u": args.noise[0], "sigma_v": args.noise[1], "seed": args.noise_seed,
                            "realisations": args.realisations}
        if args.bundle_stats:
            top["bundle_stats"] = {"file": os.path.basename(bundles_path(args.output)), "span": args.realisations,
                                   "threshold_v": args.bundle_threshold_v}
        json.dump(top, f, indent=1)
    kernel, _ = sim.context.info()
    ens.destroy()
    sim.context.close()
    cells = shape[0] * shape[1]
    member_steps = len(params) * done if taken is None else int(taken.sum())  # (retired members took fewer)
    return {"members": len(params), "shape": shape, "steps": done, "seconds": elapsed, "kernel": kernel,
            "mcells_steps_per_s": member_steps * cells / elapsed / 1e6 if elapsed > 0 else 0.0}


def main(argv=None) -> int:
    info = run(parse(argv))
    print("sweep: {members} members x {steps} steps on {shape[0]}x{shape[1]} in {seconds:.3f} s with {kernel} "
          "({mcells_steps_per_s:.0f} Mcells*steps/s)".format(**info), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
