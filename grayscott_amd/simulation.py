"""Host-side mirror of the reference's backend interface, over the C ABI.

Same names, argument meaning and error behaviour as the Rust items they mirror, so that
the parity tests read like tests of a reference backend:

=========================  ==========================================================
here                       reference (/root/reference/...)
=========================  ==========================================================
``Parameters``             data/src/parameters.rs:13-33, ``Default`` :72-83
``HipConcentration``       ``Concentration`` trait, data/src/concentration/mod.rs:198-296
``Evolving`` / ``Species`` data/src/concentration/mod.rs:17-187
``HipArgs``                ``SimulateBase::CliArgs`` (defaults + env), compute/shared/src/lib.rs:20-25
``Simulation``             ``SimulateBase`` / ``SimulateCreate`` / ``Simulate``,
                           compute/shared/src/lib.rs:19-58
=========================  ==========================================================

The Rust shim a maintainer would add (rust/compute_hip) has exactly this shape; this
module is what the Python harness (tests, bench) uses in its place because the image has
no Rust toolchain.  All arithmetic happens in ``libgs_hip.so``; there is no CPU path.
"""
from __future__ import annotations

import ctypes
import math
import os
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import capi
from .capi import GsError

STENCIL_WEIGHTS = ((0.25, 0.5, 0.25), (0.5, 0.0, 0.5), (0.25, 0.5, 0.25))  # parameters.rs:116-122

# The reference picks its stencil at compile time with cargo features (data/Cargo.toml:28-58,
# parameters.rs:91-122); here every set is a run-time value of ``Parameters.weights`` (the
# reference's ``weights-runtime`` feature).  Only the power-of-two sets can use GS_MATH_FUSED.
STENCILS = {
    "oono-puri": STENCIL_WEIGHTS,                                                    # default
    "5points": ((0.0, 1.0, 0.0), (1.0, 0.0, 1.0), (0.0, 1.0, 0.0)),                 # weights-5points
    "patrakarttunen": ((1 / 6, 4 / 6, 1 / 6), (4 / 6, 0.0, 4 / 6), (1 / 6, 4 / 6, 1 / 6)),   # weights-patrakarttunen
    "pretty": ((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0)),                  # weights-pretty
}


@dataclass
class Parameters:
    """``Parameters`` with ``Parameters::default()`` values (parameters.rs:72-83)."""

    weights: Tuple[Tuple[float, float, float], ...] = STENCIL_WEIGHTS
    diffusion_rate_u: float = 0.1
    diffusion_rate_v: float = 0.05
    feed_rate: float = 0.014
    kill_rate: float = 0.054
    time_step: float = 1.0

    @classmethod
    def with_stencil(cls, name: str, **kw) -> "Parameters":
        """Default parameters with one of the reference's named stencils (``STENCILS``)."""
        return cls(weights=STENCILS[name], **kw)

    def to_c(self) -> capi.GsParams:
        p = capi.GsParams()
        for i in range(3):
            for j in range(3):
                p.w[i][j] = self.weights[i][j]
        p.du, p.dv = self.diffusion_rate_u, self.diffusion_rate_v
        p.feed, p.kill, p.dt = self.feed_rate, self.kill_rate, self.time_step
        return p


def _env_int(name: str, default: int) -> int:
    v = os.environ.get(name)
    return int(v) if v not in (None, "") else default


@dataclass
class HipArgs:
    """Backend ``CliArgs``: every field has a default and an environment variable, as the
    reference requires so that its criterion harness can build a backend from the
    environment alone (compute/shared/src/lib.rs:20-25, benchmark.rs:36-40).

    ``boundary`` is the rule on the grid's edges (``gs_boundary``): ``capi.GS_BOUNDARY_CLIPPED`` (the parity
    target), ``capi.GS_BOUNDARY_ZERO_HALO``, ``capi.GS_BOUNDARY_PERIODIC`` -- the grid wraps around; one device
    and one process only, and neither ``kernel`` = ``GS_KERNEL_WINDOW`` / ``GS_KERNEL_LDS`` nor ``split`` > 1 -- or
    ``capi.GS_BOUNDARY_NEUMANN`` -- zero flux: a neighbour outside the grid is the nearest cell inside it; any devices,
    processes and ``split``, but neither ``kernel`` = ``GS_KERNEL_WINDOW`` nor ``GS_KERNEL_LDS``."""

    devices: Sequence[int] = field(default_factory=lambda: [
        int(x) for x in os.environ.get("GS_HIP_DEVICES", "0").split(",") if x != ""])
    math: int = field(default_factory=lambda: _env_int("GS_HIP_MATH", capi.GS_MATH_STRICT))
    kernel: int = field(default_factory=lambda: _env_int("GS_HIP_KERNEL", capi.GS_KERNEL_AUTO))
    rows_per_block: int = field(default_factory=lambda: _env_int("GS_HIP_ROWS_PER_BLOCK", 0))
    fuse_steps: int = field(default_factory=lambda: _env_int("GS_HIP_FUSE_STEPS", 0))
    use_graph: int = field(default_factory=lambda: _env_int("GS_HIP_USE_GRAPH", 0))
    pitch_pad: int = field(default_factory=lambda: _env_int("GS_HIP_PITCH_PAD", 0))
    split: int = field(default_factory=lambda: _env_int("GS_HIP_SPLIT", 0))
    general_kernels: int = field(default_factory=lambda: _env_int("GS_HIP_GENERAL_KERNELS", 0))
    cols_per_lane: int = field(default_factory=lambda: _env_int("GS_HIP_COLS_PER_LANE", 0))
    boundary: int = field(default_factory=lambda: _env_int("GS_HIP_BOUNDARY", capi.GS_BOUNDARY_CLIPPED))
    no_tune: int = field(default_factory=lambda: _env_int("GS_HIP_NO_TUNE", 0))
    tile_shape: int = field(default_factory=lambda: _env_int("GS_HIP_TILE_SHAPE", 0))
    share_taps: int = field(default_factory=lambda: _env_int("GS_HIP_SHARE_TAPS", 0))
    # not a gs_options field: the most extra blocks gs_fields_place may draw for a Species that make_species creates
    # (every Species of >= PLACE_MIN_CELLS cells per process on a context with one slab per process; 0 = no placement)
    place_candidates: int = field(default_factory=lambda: _env_int("GS_HIP_PLACE_CANDIDATES", 12))
    rank: int = 0
    world: int = 1
    unique_id: Optional[bytes] = None

    def to_c(self) -> capi.GsOptions:
        o = capi.default_options()
        o.math, o.kernel = self.math, self.kernel
        o.rows_per_block, o.fuse_steps = self.rows_per_block, self.fuse_steps
        o.use_graph, o.pitch_pad = self.use_graph, self.pitch_pad
        o.split = self.split
        o.general_kernels = self.general_kernels
        o.cols_per_lane = self.cols_per_lane
        o.boundary = self.boundary
        o.no_tune = self.no_tune
        o.tile_shape = self.tile_shape
        o.share_taps = self.share_taps
        return o


# make_species places a Species by measurement from this many cells per process on (planes of 256 MiB): below, the
# planes largely stay in the 256 MB last-level cache and where they lie in HBM does not show
PLACE_MIN_CELLS = 1 << 26


class HipContext:
    """``Concentration::Context`` of ``HipConcentration``: devices, streams, row partition
    and (multi-process) the RCCL communicator -- one ``gs_ctx``."""

    def __init__(self, params: Parameters, args: Optional[HipArgs] = None):
        args = args or HipArgs()
        lib = capi.load()
        self._lib = lib
        self._h = ctypes.c_void_p()
        cp, co = params.to_c(), args.to_c()
        devs = (ctypes.c_int32 * len(args.devices))(*args.devices)
        uid = ctypes.create_string_buffer(args.unique_id, capi.GS_UNIQUE_ID_BYTES) \
            if args.unique_id else None
        capi.check(lib.gs_ctx_create(ctypes.byref(self._h), ctypes.byref(cp), ctypes.byref(co),
                                     devs, len(args.devices), args.rank, args.world, uid))
        self.args = args

    @property
    def handle(self):
        if not self._h:
            raise GsError(capi.GS_ERR_INVALID, "context already destroyed")
        return self._h

    def set_params(self, params: Parameters) -> None:
        cp = params.to_c()
        capi.check(self._lib.gs_ctx_set_params(self.handle, ctypes.byref(cp)))

    def sync(self) -> None:
        capi.check(self._lib.gs_sync(self.handle))

    def download_wait(self, in_flight: int = 0) -> None:
        """Wait for the asynchronous downloads enqueued so far (not for later steps); ``in_flight=1``: for all but the
        newest (``gs_download_wait_but``: two images on their way, the PCIe link never idles between them)."""
        capi.check(self._lib.gs_download_wait_but(self.handle, int(in_flight)))

    def timer_start(self) -> None:
        capi.check(self._lib.gs_timer_start(self.handle))

    def timer_stop(self) -> float:
        ms = ctypes.c_float(0)
        capi.check(self._lib.gs_timer_stop(self.handle, ctypes.byref(ms)))
        return float(ms.value)

    def get_tuned(self, slab_rows: int, cols: int) -> Tuple[int, int, int, int]:
        """(rows per unit, steps fused per pass, columns per lane, share_taps: 1 = on, 2 = off, 3 = across lanes too) chosen for slabs of
        this shape; zeros when nothing was chosen yet (``gs_ctx_get_tuned``)."""
        a, b, c, d = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        capi.check(self._lib.gs_ctx_get_tuned(self.handle, slab_rows, cols, ctypes.byref(a), ctypes.byref(b),
                                              ctypes.byref(c), ctypes.byref(d)))
        return int(a.value), int(b.value), int(c.value), int(d.value)

    def set_tuned(self, slab_rows: int, cols: int, rows_per_block: int, fuse_steps: int, cols_per_lane: int,
                  share_taps: int = 0) -> None:
        capi.check(self._lib.gs_ctx_set_tuned(self.handle, slab_rows, cols, rows_per_block, fuse_steps,
                                              cols_per_lane, share_taps))

    def place_stats(self) -> Tuple[int, int]:
        """(pair probes timed, extra blocks drawn) by ``gs_fields_place`` on this context so far."""
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        capi.check(self._lib.gs_debug_place_stats(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def comm_info(self) -> Tuple[int, int, int]:
        """(ranks, rank, device) as RCCL reports them for this context's communicator; (0, -1, -1)
        for a single process."""
        a, b, c = ctypes.c_int32(0), ctypes.c_int32(-1), ctypes.c_int32(-1)
        capi.check(self._lib.gs_ctx_comm_info(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def stats(self) -> dict:
        """``gs_ctx_stats``: passes / steps / launches / ghost_refreshes since the context was created and,
        for the passes timed with ``set_pass_timing``, the halo-stream and interior-kernel times (ms)."""
        st = capi.GsStats()
        capi.check(self._lib.gs_ctx_stats(self.handle, ctypes.byref(st)))
        return {name: getattr(st, name) for name, _ in capi.GsStats._fields_ if name != "reserved"}

    def quiet_stats(self) -> Tuple[int, int, int, int]:
        """``gs_ctx_quiet_stats``: units launched by the passes that may leave units at rest alone, units among them
        that left without computing, those passes, and the ones among them that could skip (the third and later full
        passes of their ``gs_run``), all since the context was created."""
        out = (ctypes.c_uint64 * 4)()
        capi.check(self._lib.gs_ctx_quiet_stats(self.handle, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def quiet_edge_stats(self) -> Tuple[int, int, int]:
        """``gs_ctx_quiet_edge_stats``: the units of edge positions among the units launched by those passes (a half-height
        unit counts as one), the ones among them that left without computing, and the interior units next to an edge
        position that did -- ``quiet_stats()[1]`` counts the skipped units with interior positions all around them."""
        out = (ctypes.c_uint64 * 3)()
        capi.check(self._lib.gs_ctx_quiet_edge_stats(self.handle, out))
        return int(out[0]), int(out[1]), int(out[2])

    def set_pass_timing(self, passes: int) -> None:
        capi.check(self._lib.gs_ctx_set_pass_timing(self.handle, passes))

    def info(self) -> Tuple[str, int]:
        buf = ctypes.create_string_buffer(64)
        n = ctypes.c_uint64(0)
        capi.check(self._lib.gs_ctx_info(self.handle, buf, 64, ctypes.byref(n)))
        return buf.value.decode(), int(n.value)

    def close(self) -> None:
        if self._h:
            self._lib.gs_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ``gs_summary`` as a numpy record: what ``Ensemble.summaries`` returns (32 bytes, the C layout, filled in place).
SUMMARY_DTYPE = np.dtype([("sum", "<f8"), ("sum_sq", "<f8"), ("min", "<f4"), ("max", "<f4"), ("nonfinite", "<u8")])


@dataclass(frozen=True)
class Summary:
    """A plane's summary computed on the device (``gs_summary``, include/gs_hip.h): ``sum`` and ``sum_sq`` of its finite
    cells (f64, in the fixed fold order the header defines: bit-reproducible), their ``min`` and ``max`` (+inf / -inf when
    there are none), the count of non-finite cells, and ``size``, the plane's number of cells."""

    sum: float
    sum_sq: float
    min: float
    max: float
    nonfinite: int
    size: int

    @classmethod
    def from_c(cls, s, size: int) -> "Summary":
        return cls(float(s.sum), float(s.sum_sq), float(s.min), float(s.max), int(s.nonfinite), int(size))

    @property
    def cells(self) -> int:
        """Finite cells: the ones the sums, the mean and the standard deviation cover."""
        return self.size - self.nonfinite

    @property
    def mean(self) -> float:
        return self.sum / self.cells if self.cells else float("nan")

    @property
    def std(self) -> float:
        """Population standard deviation of the finite cells, from the two sums."""
        if not self.cells:
            return float("nan")
        m = self.mean
        return float(np.sqrt(max(self.sum_sq / self.cells - m * m, 0.0)))


def _handle_array(fields: Sequence["HipConcentration"]):
    """The planes' handles as the C ABI's field lists take them (an empty list as one null: the library refuses it)."""
    return (ctypes.c_void_p * max(len(fields), 1))(*[f.handle for f in fields])


def summarize_fields(context: "HipContext", fields: Sequence["HipConcentration"]) -> List[Summary]:
    """``gs_fields_summarize``: summaries of 1..4 planes of one shape over the whole global grid, in one call (collective
    in a multi-process context)."""
    n, arr = len(fields), _handle_array(fields)
    out = (capi.GsSummary * max(n, 1))()
    capi.check(context._lib.gs_fields_summarize(context.handle, arr, n, out))
    rows, cols = fields[0].shape()
    return [Summary.from_c(out[i], rows * cols) for i in range(n)]


# ``gs_change`` as a numpy record: what ``Ensemble.changes_since`` returns (40 bytes, the C layout, filled in place).
CHANGE_DTYPE = np.dtype([("sum_abs", "<f8"), ("sum_sq", "<f8"), ("max_abs", "<f8"), ("differing", "<u8"), ("nonfinite", "<u8")])
# gs_noise's layout (24 bytes): what Ensemble.set_noise sends and Ensemble.noise returns, one record per member
NOISE_DTYPE = np.dtype([("sigma_u", "<f4"), ("sigma_v", "<f4"), ("seed", "<u8"), ("step", "<u8")])


@dataclass(frozen=True)
class Change:
    """How far one plane is from another of the same shape, computed on the device (``gs_change``, include/gs_hip.h):
    with d = a - b formed in f64 per cell, ``sum_abs`` = sum |d|, ``sum_sq`` = sum d * d (in the summaries' fixed fold order:
    bit-reproducible) and ``max_abs`` = max |d| over the comparable cells -- those where both planes are finite --,
    ``differing`` the cells whose 32 bits differ (all cells), ``nonfinite`` the cells where either plane is NaN or
    infinite, and ``cells``, the planes' number of cells."""

    sum_abs: float
    sum_sq: float
    max_abs: float
    differing: int
    nonfinite: int
    cells: int

    @classmethod
    def from_c(cls, c, cells: int) -> "Change":
        return cls(float(c.sum_abs), float(c.sum_sq), float(c.max_abs), int(c.differing), int(c.nonfinite), int(cells))

    @property
    def comparable(self) -> int:
        """Cells where both planes are finite: the ones the sums and the maximum cover."""
        return self.cells - self.nonfinite

    @property
    def equal(self) -> bool:
        """The two planes hold the same bits in every cell."""
        return self.differing == 0

    @property
    def mean_abs(self) -> float:
        return self.sum_abs / self.comparable if self.comparable else float("nan")

    @property
    def rms(self) -> float:
        return float(np.sqrt(self.sum_sq / self.comparable)) if self.comparable else float("nan")


def compare_fields(context: "HipContext", a: Sequence["HipConcentration"], b: Sequence["HipConcentration"]) -> List[Change]:
    """``gs_fields_compare``: plane ``a[i]`` against ``b[i]`` for 1..4 pairs of one shape over the whole global grid, in one
    call (blocking; collective in a multi-process context)."""
    if len(a) != len(b):
        raise ValueError("one second plane per first plane")
    n = len(a)
    out = (capi.GsChange * max(n, 1))()
    capi.check(context._lib.gs_fields_compare(context.handle, _handle_array(a), _handle_array(b), n, out))
    rows, cols = a[0].shape()
    return [Change.from_c(out[i], rows * cols) for i in range(n)]


def copy_fields(context: "HipContext", dst: Sequence["HipConcentration"], src: Sequence["HipConcentration"]) -> None:
    """``gs_fields_copy``: ``dst[i]`` receives the cells of ``src[i]`` on the device (1..4 pairs of one shape; blocking).
    The targets are left as an upload leaves them."""
    if len(dst) != len(src):
        raise ValueError("one source per target")
    capi.check(context._lib.gs_fields_copy(context.handle, _handle_array(dst), _handle_array(src), len(dst)))


@dataclass(frozen=True, eq=False)
class Histogram:
    """A plane's histogram computed on the device (``gs_fields_histogram``; the binning rule is include/gs_hip.h's, in
    f32 -- not ``numpy.histogram``'s).  ``counts[i]`` is the number of cells in bin i of ``bins`` equal bins of
    ``[lo, hi]`` (the last bin is closed: a cell equal to ``hi`` is in it), ``below`` / ``above`` those outside the
    range (infinities included), ``nan`` the NaN cells, ``size`` the plane's number of cells -- the sum of all of them.

    ``fraction_above`` and ``quantile`` work at bin resolution and over the in-range cells (``counts``) alone: cells
    below, above and NaN take no part."""

    counts: np.ndarray
    below: int
    above: int
    nan: int
    lo: float
    hi: float
    size: int

    @classmethod
    def from_counters(cls, c: np.ndarray, lo: float, hi: float, size: int) -> "Histogram":
        """From ``bins + 3`` counters as the C ABI writes them: counts, below, above, nan."""
        c = np.asarray(c, np.uint64)
        return cls(c[:-3].copy(), int(c[-3]), int(c[-2]), int(c[-1]), float(lo), float(hi), int(size))

    @property
    def bins(self) -> int:
        return len(self.counts)

    @property
    def in_range(self) -> int:
        """Cells inside ``[lo, hi]``: the ones ``counts`` holds."""
        return int(self.counts.sum(dtype=np.uint64))

    def edges(self) -> np.ndarray:
        """The ``bins + 1`` nominal bin edges ``lo + i (hi - lo) / bins`` in f64.  The true edges -- where the f32 rule
        steps -- lie within rounding of them."""
        return self.lo + (self.hi - self.lo) * np.arange(self.bins + 1, dtype=np.float64) / self.bins

    def fraction_above(self, x: float) -> float:
        """Share of the in-range cells that lie in bins whose nominal lower edge is at least ``x``, i.e. in bins
        ``i >= ceil((x - lo) / (hi - lo) * bins)``: exact when ``x`` is an edge, else the bin that contains ``x`` counts
        as not above.  1.0 for ``x <= lo``, 0.0 for ``x > hi``; NaN when no cell is in range."""
        total = self.in_range
        if not total:
            return float("nan")
        first = int(np.searchsorted(self.edges()[:-1], x, side="left"))  # bins [first, bins) have lower edge >= x
        return int(self.counts[first:].sum(dtype=np.uint64)) / total

    def quantile(self, q: float) -> float:
        """The nominal upper edge of the first bin at which the cumulative count of in-range cells reaches ``q`` times
        their number (at least one cell): an upper bound of the q-quantile of the in-range cells, at most one bin width
        above it.  ``0 <= q <= 1``; NaN when no cell is in range."""
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"quantile {q} outside [0, 1]")
        total = self.in_range
        if not total:
            return float("nan")
        need = max(1, int(np.ceil(q * total)))
        cum = np.cumsum(self.counts, dtype=np.uint64)
        return float(self.edges()[int(np.searchsorted(cum, need, side="left")) + 1])


def _f32_pairs(ranges) -> Tuple["ctypes.Array", "ctypes.Array"]:
    lo = (ctypes.c_float * len(ranges))(*[float(r[0]) for r in ranges])
    hi = (ctypes.c_float * len(ranges))(*[float(r[1]) for r in ranges])
    return lo, hi


def histogram_fields(context: "HipContext", fields: Sequence["HipConcentration"], bins: int,
                     ranges: Sequence[Tuple[float, float]]) -> List[Histogram]:
    """``gs_fields_histogram``: histograms of 1..4 planes of one shape over the whole global grid, plane i over
    ``ranges[i]``, in one call (collective in a multi-process context)."""
    n, bins = len(fields), int(bins)
    if len(ranges) != n:
        raise ValueError("one (lo, hi) range per field")
    arr = _handle_array(fields)
    lo, hi = _f32_pairs(ranges)
    out = np.zeros((max(n, 1), max(bins, 0) + 3), np.uint64)
    capi.check(context._lib.gs_fields_histogram(context.handle, arr, n, lo, hi, bins,
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
    rows, cols = fields[0].shape()
    return [Histogram.from_counters(out[i], lo[i], hi[i], rows * cols) for i in range(n)]


def quad_measures(quads) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``(area, perimeter, euler4, euler8)`` as int64 arrays from bit-quad counts whose LAST axis is the six classes Q0, Q1,
    Q2, Q3, Q4, QD (include/gs_hip.h) -- a ``Morphology.quads`` vector, or what ``Ensemble.morphologies`` returns.  All exact:
    area = (Q1 + 2 Q2 + 2 QD + 3 Q3 + 4 Q4) / 4 set cells, perimeter = Q1 + Q2 + 2 QD + Q3 cell sides between a set and an
    unset cell (the padding ring included), euler8 = (Q1 - Q3 - 2 QD) / 4 and euler4 = (Q1 - Q3 + 2 QD) / 4: components minus
    holes under 8- and 4-connectivity."""
    q = np.asarray(quads).astype(np.int64)
    q1, q2, q3, q4, qd = q[..., 1], q[..., 2], q[..., 3], q[..., 4], q[..., 5]
    area = (q1 + 2 * q2 + 2 * qd + 3 * q3 + 4 * q4) // 4
    perimeter = q1 + q2 + 2 * qd + q3
    return area, perimeter, (q1 - q3 + 2 * qd) // 4, (q1 - q3 - 2 * qd) // 4


@dataclass(frozen=True, eq=False)
class Morphology:
    """The bit-quad counts of one thresholded plane, counted on the device (``gs_fields_morphology``; the rule is
    include/gs_hip.h's): a cell is set when it is above ``threshold`` (``above``) or below it (one f32 comparison; NaN and
    equal cells are not set), the image is padded with one ring of unset cells, and ``quads`` holds how many of its
    ``(rows + 1)(cols + 1)`` 2 x 2 blocks have no, one, two side-sharing, three, four, or two diagonal set cells (Q0, Q1, Q2,
    Q3, Q4, QD).  The derived quantities are exact integers; ``cells`` is the plane's number of cells."""

    quads: np.ndarray
    threshold: float
    above: bool
    cells: int

    @classmethod
    def from_quads(cls, quads, threshold: float, above: bool, cells: int) -> "Morphology":
        return cls(np.array(quads, np.uint64).reshape(6), float(threshold), bool(above), int(cells))

    @property
    def area(self) -> int:
        """Set cells."""
        return int(quad_measures(self.quads)[0])

    @property
    def area_fraction(self) -> float:
        return self.area / self.cells if self.cells else float("nan")

    @property
    def perimeter(self) -> int:
        """Cell sides between a set and an unset cell (4-connected boundary length), the padding ring included."""
        return int(quad_measures(self.quads)[1])

    @property
    def euler4(self) -> int:
        """4-connected components minus their holes."""
        return int(quad_measures(self.quads)[2])

    @property
    def euler8(self) -> int:
        """8-connected components minus their holes: large and positive for spots, about 0 for stripes and labyrinths,
        negative for hole patterns."""
        return int(quad_measures(self.quads)[3])


def _thresholds(values) -> List[float]:
    return [float(values)] if np.isscalar(values) else [float(x) for x in values]


def _field_thresholds(fields, thresholds, above):
    """``(n, nt, thresholds as c_float[n * nt], senses as c_int32[n])`` for the thresholded observables of a field list."""
    n = len(fields)
    if len(thresholds) != n or len(above) != n:
        raise ValueError("one list of thresholds and one sense per field")
    lists = [_thresholds(t) for t in thresholds]
    nt = len(lists[0]) if lists else 0
    if any(len(t) != nt for t in lists):
        raise ValueError("the same number of thresholds for every field")
    flat = [x for t in lists for x in t]
    return (n, nt, (ctypes.c_float * max(len(flat), 1))(*flat),
            (ctypes.c_int32 * max(n, 1))(*[1 if a else 0 for a in above]))


def _member_thresholds(u_thresholds, v_thresholds, above):
    """``(nt, U's then V's thresholds as c_float[2 * nt], (U's, V's) senses as c_int32[2])`` for an ensemble's observables."""
    tu, tv = _thresholds(u_thresholds), _thresholds(v_thresholds)
    if len(tu) != len(tv):
        raise ValueError("the same number of thresholds for U and V")
    return (len(tu), (ctypes.c_float * max(2 * len(tu), 1))(*(tu + tv)),
            (ctypes.c_int32 * 2)(1 if above[0] else 0, 1 if above[1] else 0))


def morphology_fields(context: "HipContext", fields: Sequence["HipConcentration"], thresholds: Sequence[Sequence[float]],
                      above: Sequence[bool]) -> List[List[Morphology]]:
    """``gs_fields_morphology``: bit-quad counts of 1..4 planes of one shape over the whole global grid in one call
    (collective in a multi-process context) -- plane i at each of ``thresholds[i]`` (1..4 per plane, the same number for
    every plane; all counted in one pass) with the sense ``above[i]``.  Returns one list of ``Morphology`` per plane."""
    n, nt, thr, sense = _field_thresholds(fields, thresholds, above)
    out = np.zeros((max(n, 1), max(nt, 1), 6), np.uint64)
    capi.check(context._lib.gs_fields_morphology(context.handle, _handle_array(fields), n, thr, sense, nt,
                                                 out.ctypes.data_as(ctypes.POINTER(capi.GsMorphology))))
    rows, cols = fields[0].shape()
    return [[Morphology.from_quads(out[i, k], thr[i * nt + k], above[i], rows * cols) for k in range(nt)] for i in range(n)]


def region_shape(region) -> Tuple[int, int]:
    """``(rh, rw)`` from a region shape given as a pair, or as one int for a square region."""
    if np.isscalar(region):
        return int(region), int(region)
    rh, rw = region
    return int(rh), int(rw)


def region_grid(rows: int, cols: int, region) -> Tuple[int, int]:
    """``gs_region_grid``: ``(RR, RC)``, the rows and columns of regions that ``region`` cuts a grid of ``rows`` x ``cols``
    cells into (ragged ones at the lower and right edge kept), or the library's refusal of the region shape.  Pure."""
    rh, rw = region_shape(region)
    rr, rc = ctypes.c_uint64(0), ctypes.c_uint64(0)
    capi.check(capi.load().gs_region_grid(int(rows), int(cols), rh, rw, ctypes.byref(rr), ctypes.byref(rc)))
    return int(rr.value), int(rc.value)


def region_sizes(rows: int, cols: int, region, grid: Tuple[int, int]) -> np.ndarray:
    """The number of cells of every region, ``(RR, RC)`` int64: ``rh * rw`` but in a ragged last row or column."""
    rh, rw = region_shape(region)
    h = np.minimum(rh, rows - rh * np.arange(grid[0], dtype=np.int64))
    w = np.minimum(rw, cols - rw * np.arange(grid[1], dtype=np.int64))
    return h[:, None] * w[None, :]


@dataclass(frozen=True, eq=False)
class RegionSummaries:
    """The summaries of every region of one plane, computed on the device (``gs_fields_region_summaries``): arrays of shape
    ``(RR, RC)``, entry (i, j) being bit for bit the ``Summary`` of a plane that holds region (i, j)'s cells alone.  ``region``
    is ``(rh, rw)``, ``shape`` the plane's, ``size`` every region's number of cells."""

    sum: np.ndarray
    sum_sq: np.ndarray
    min: np.ndarray
    max: np.ndarray
    nonfinite: np.ndarray
    size: np.ndarray
    region: Tuple[int, int]
    shape: Tuple[int, int]

    @classmethod
    def from_records(cls, rec: np.ndarray, region, shape) -> "RegionSummaries":
        """From ``(RR, RC)`` records of ``SUMMARY_DTYPE`` as the C ABI writes them."""
        region, shape = region_shape(region), (int(shape[0]), int(shape[1]))
        return cls(rec["sum"].copy(), rec["sum_sq"].copy(), rec["min"].copy(), rec["max"].copy(), rec["nonfinite"].copy(),
                   region_sizes(shape[0], shape[1], region, rec.shape), region, shape)

    @property
    def cells(self) -> np.ndarray:
        """Finite cells per region: the ones the sums, the mean and the variance cover."""
        return self.size - self.nonfinite.astype(np.int64)

    def mean(self) -> np.ndarray:
        """Per region, as ``Summary.mean``: NaN where a region has no finite cell."""
        cells = self.cells.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(cells > 0, self.sum / cells, np.nan)

    def variance(self) -> np.ndarray:
        """Per region, the population variance of the finite cells from the two sums (the square of ``Summary.std``, before
        its root): NaN where a region has no finite cell."""
        cells = self.cells.astype(np.float64)
        m = self.mean()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(cells > 0, np.maximum(self.sum_sq / cells - m * m, 0.0), np.nan)

    def at(self, i: int, j: int) -> Summary:
        return Summary(float(self.sum[i, j]), float(self.sum_sq[i, j]), float(self.min[i, j]), float(self.max[i, j]),
                       int(self.nonfinite[i, j]), int(self.size[i, j]))


@dataclass(frozen=True, eq=False)
class RegionMorphology:
    """The bit-quad counts of every region of one thresholded plane, counted on the device
    (``gs_fields_region_morphology``): ``quads`` of shape ``(RR, RC, 6)``, entry (i, j) being the ``Morphology.quads`` of a
    plane that holds region (i, j)'s cells alone -- the region padded with its own ring of unset cells.  ``cells`` is every
    region's number of cells; the derived arrays are ``quad_measures``' exact integers."""

    quads: np.ndarray
    threshold: float
    above: bool
    cells: np.ndarray
    region: Tuple[int, int]
    shape: Tuple[int, int]

    @classmethod
    def from_quads(cls, quads, threshold: float, above: bool, region, shape) -> "RegionMorphology":
        quads = np.array(quads, np.uint64)
        region, shape = region_shape(region), (int(shape[0]), int(shape[1]))
        return cls(quads, float(threshold), bool(above), region_sizes(shape[0], shape[1], region, quads.shape[:2]), region, shape)

    @property
    def area(self) -> np.ndarray:
        return quad_measures(self.quads)[0]

    @property
    def area_fraction(self) -> np.ndarray:
        return self.area / self.cells

    @property
    def perimeter(self) -> np.ndarray:
        return quad_measures(self.quads)[1]

    @property
    def euler4(self) -> np.ndarray:
        return quad_measures(self.quads)[2]

    @property
    def euler8(self) -> np.ndarray:
        return quad_measures(self.quads)[3]

    def at(self, i: int, j: int) -> Morphology:
        return Morphology.from_quads(self.quads[i, j], self.threshold, self.above, int(self.cells[i, j]))


@dataclass(frozen=True, eq=False)
class RegionChange:
    """The change of every region of one plane against another of the same shape, computed on the device
    (``gs_fields_region_compare``): arrays of shape ``(RR, RC)``, entry (i, j) being bit for bit the ``Change`` of two planes
    that hold region (i, j)'s cells alone.  ``region`` is ``(rh, rw)``, ``shape`` the planes', ``size`` every region's
    number of cells."""

    sum_abs: np.ndarray
    sum_sq: np.ndarray
    max_abs: np.ndarray
    differing: np.ndarray
    nonfinite: np.ndarray
    size: np.ndarray
    region: Tuple[int, int]
    shape: Tuple[int, int]

    @classmethod
    def from_records(cls, rec: np.ndarray, region, shape) -> "RegionChange":
        """From ``(RR, RC)`` records of ``CHANGE_DTYPE`` as the C ABI writes them."""
        region, shape = region_shape(region), (int(shape[0]), int(shape[1]))
        return cls(rec["sum_abs"].copy(), rec["sum_sq"].copy(), rec["max_abs"].copy(), rec["differing"].copy(),
                   rec["nonfinite"].copy(), region_sizes(shape[0], shape[1], region, rec.shape), region, shape)

    @property
    def comparable(self) -> np.ndarray:
        """Cells per region where both planes are finite: the ones the sums and the maximum cover."""
        return self.size - self.nonfinite.astype(np.int64)

    def mean_abs(self) -> np.ndarray:
        """Per region, as ``Change.mean_abs``: NaN where a region has no comparable cell."""
        cells = self.comparable.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(cells > 0, self.sum_abs / cells, np.nan)

    def rms(self) -> np.ndarray:
        """Per region, as ``Change.rms``: NaN where a region has no comparable cell."""
        cells = self.comparable.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(cells > 0, np.sqrt(self.sum_sq / cells), np.nan)

    def steady(self, tol: float) -> np.ndarray:
        """Per region: no comparable cell moved by more than ``tol`` and every cell is comparable."""
        return (self.max_abs <= float(tol)) & (self.nonfinite == 0)

    def at(self, i: int, j: int) -> Change:
        return Change(float(self.sum_abs[i, j]), float(self.sum_sq[i, j]), float(self.max_abs[i, j]), int(self.differing[i, j]),
                      int(self.nonfinite[i, j]), int(self.size[i, j]))


def region_compare_fields(context: "HipContext", a: Sequence["HipConcentration"], b: Sequence["HipConcentration"],
                          region) -> List[RegionChange]:
    """``gs_fields_region_compare``: the change of every region of plane ``a[i]`` against ``b[i]`` for 1..4 pairs of one
    shape in one call (blocking; collective in a multi-process context).  ``region`` is ``(rh, rw)`` or an int for a square
    region."""
    if len(a) != len(b):
        raise ValueError("one second plane per first plane")
    n, (rh, rw) = len(a), region_shape(region)
    shape = a[0].shape() if a else (0, 0)
    try:
        grid = region_grid(shape[0], shape[1], (rh, rw))
    except capi.GsError:
        grid = (0, 0)  # (the call below refuses it, in the header's order)
    out = np.zeros((max(n, 1),) + grid, CHANGE_DTYPE)
    capi.check(context._lib.gs_fields_region_compare(context.handle, _handle_array(a), _handle_array(b), n, rh, rw,
                                                     out.ctypes.data_as(ctypes.POINTER(capi.GsChange))))
    return [RegionChange.from_records(out[i], (rh, rw), shape) for i in range(n)]


def region_summaries_fields(context: "HipContext", fields: Sequence["HipConcentration"], region) -> List[RegionSummaries]:
    """``gs_fields_region_summaries``: the summaries of every region of 1..4 planes of one shape in one call (blocking;
    collective in a multi-process context).  ``region`` is ``(rh, rw)`` or an int for a square region."""
    n, (rh, rw) = len(fields), region_shape(region)
    shape = fields[0].shape() if fields else (0, 0)
    try:
        grid = region_grid(shape[0], shape[1], (rh, rw))
    except capi.GsError:
        grid = (0, 0)  # (the call below refuses it, in the header's order)
    out = np.zeros((max(n, 1),) + grid, SUMMARY_DTYPE)
    capi.check(context._lib.gs_fields_region_summaries(context.handle, _handle_array(fields), n, rh, rw,
                                                       out.ctypes.data_as(ctypes.POINTER(capi.GsSummary))))
    return [RegionSummaries.from_records(out[i], (rh, rw), shape) for i in range(n)]


def region_morphology_fields(context: "HipContext", fields: Sequence["HipConcentration"], region,
                             thresholds: Sequence[Sequence[float]], above: Sequence[bool]) -> List[List[RegionMorphology]]:
    """``gs_fields_region_morphology``: the bit-quad counts of every region of 1..4 planes of one shape in one call
    (blocking; collective in a multi-process context) -- plane i at each of ``thresholds[i]`` (1..4 per plane, one pass) with
    the sense ``above[i]``.  Returns one list of ``RegionMorphology`` per plane, one entry per threshold."""
    n, nt, thr, sense = _field_thresholds(fields, thresholds, above)
    rh, rw = region_shape(region)
    shape = fields[0].shape() if fields else (0, 0)
    try:
        grid = region_grid(shape[0], shape[1], (rh, rw))
    except capi.GsError:
        grid = (0, 0)
    out = np.zeros((max(n, 1),) + grid + (max(nt, 1), 6), np.uint64)
    capi.check(context._lib.gs_fields_region_morphology(context.handle, _handle_array(fields), n, rh, rw, thr, sense, nt,
                                                        out.ctypes.data_as(ctypes.POINTER(capi.GsMorphology))))
    return [[RegionMorphology.from_quads(out[i, :, :, k], thr[i * nt + k], above[i], (rh, rw), shape) for k in range(nt)]
            for i in range(n)]


@dataclass(frozen=True, eq=False)
class Components:
    """The connected components of one thresholded plane, labelled on the device (``gs_fields_components``; the rule is
    include/gs_hip.h's): a cell is set by ``Morphology``'s rule, set cells are neighbours across a side or, under
    ``connectivity`` 8, also across a corner, and components never wrap.  ``by_size[b]`` counts the components of
    ``2^b <= size < 2^(b+1)`` cells (the last bin takes every larger one).  All exact integers."""

    count: int
    set_cells: int
    largest: int
    by_size: np.ndarray
    threshold: float
    above: bool
    connectivity: int

    @classmethod
    def from_counters(cls, words, threshold: float, above: bool, connectivity: int) -> "Components":
        """From the 35 u64 words of a ``gs_components``: components, set_cells, largest, by_size[32]."""
        w = np.array(words, np.uint64).reshape(35)
        return cls(int(w[0]), int(w[1]), int(w[2]), w[3:].copy(), float(threshold), bool(above), int(connectivity))

    @property
    def mean_size(self) -> float:
        """Cells per component; NaN when there is none."""
        return self.set_cells / self.count if self.count else float("nan")

    @property
    def largest_fraction(self) -> float:
        """The largest component's share of the set cells; NaN when none is set."""
        return self.largest / self.set_cells if self.set_cells else float("nan")

    def holes(self, morphology: "Morphology") -> int:
        """Holes of the pattern: components minus the Euler number of the same connectivity, from a ``Morphology`` of the
        same plane, threshold and sense (another threshold or sense is refused)."""
        if np.float32(morphology.threshold) != np.float32(self.threshold) or bool(morphology.above) != self.above:
            raise ValueError("a Morphology of threshold %r (above=%r) for Components of threshold %r (above=%r)"
                             % (morphology.threshold, morphology.above, self.threshold, self.above))
        return self.count - (morphology.euler8 if self.connectivity == 8 else morphology.euler4)


def components_fields(context: "HipContext", fields: Sequence["HipConcentration"], thresholds: Sequence[Sequence[float]],
                      above: Sequence[bool], connectivity: int = 8) -> List[List[Components]]:
    """``gs_fields_components``: the connected components of 1..4 planes of one shape over the whole global grid in one call
    (collective in a multi-process context) -- plane i at each of ``thresholds[i]`` (1..4 per plane, the same number for
    every plane) with the sense ``above[i]`` under ``connectivity`` 4 or 8.  Returns one list of ``Components`` per plane."""
    n, nt, thr, sense = _field_thresholds(fields, thresholds, above)
    out = np.zeros((max(n, 1), max(nt, 1), 35), np.uint64)
    capi.check(context._lib.gs_fields_components(context.handle, _handle_array(fields), n, thr, sense, nt, int(connectivity),
                                                 out.ctypes.data_as(ctypes.POINTER(capi.GsComponents))))
    return [[Components.from_counters(out[i, k], thr[i * nt + k], above[i], connectivity) for k in range(nt)]
            for i in range(n)]


@dataclass(frozen=True, eq=False)
class RegionComponents:
    """The connected components of every region of one thresholded plane, labelled on the device
    (``gs_fields_region_components``): ``count``, ``set_cells`` and ``largest`` of shape ``(RR, RC)`` and ``by_size`` of shape
    ``(RR, RC, 32)``, entry (i, j) being the ``Components`` of a plane that holds region (i, j)'s cells alone -- a region's
    border is a wall, so a spot that straddles one counts once in every region it touches.  All exact integers."""

    count: np.ndarray
    set_cells: np.ndarray
    largest: np.ndarray
    by_size: np.ndarray
    threshold: float
    above: bool
    connectivity: int
    region: Tuple[int, int]
    shape: Tuple[int, int]

    @classmethod
    def from_counters(cls, words, threshold: float, above: bool, connectivity: int, region, shape) -> "RegionComponents":
        """From ``(RR, RC, 35)`` u64 words, a ``gs_components`` per region: components, set_cells, largest, by_size[32]."""
        w = np.array(words, np.uint64)
        return cls(w[..., 0].copy(), w[..., 1].copy(), w[..., 2].copy(), w[..., 3:].copy(), float(threshold), bool(above),
                   int(connectivity), region_shape(region), (int(shape[0]), int(shape[1])))

    def counters(self) -> np.ndarray:
        """The ``(RR, RC, 35)`` u64 words the object was made from."""
        return np.concatenate([self.count[..., None], self.set_cells[..., None], self.largest[..., None], self.by_size], axis=-1)

    def mean_size(self) -> np.ndarray:
        """Cells per component of every region; NaN where there is none."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.count > 0, self.set_cells / self.count, np.nan)

    def largest_fraction(self) -> np.ndarray:
        """The largest component's share of every region's set cells -- near 1 where one component percolates the region --;
        NaN where none is set."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.set_cells > 0, self.largest / self.set_cells, np.nan)

    def holes(self, region_morphology: "RegionMorphology") -> np.ndarray:
        """Holes of every region's pattern: components minus the Euler number of the same connectivity, from a
        ``RegionMorphology`` of the same plane, region shape, threshold and sense (another is refused)."""
        m = region_morphology
        if (np.float32(m.threshold) != np.float32(self.threshold) or bool(m.above) != self.above or m.region != self.region
                or m.quads.shape[:2] != self.count.shape):
            raise ValueError("a RegionMorphology of threshold %r (above=%r), regions %r for RegionComponents of threshold %r "
                             "(above=%r), regions %r" % (m.threshold, m.above, m.region, self.threshold, self.above, self.region))
        return self.count.astype(np.int64) - (m.euler8 if self.connectivity == 8 else m.euler4)

    def at(self, i: int, j: int) -> Components:
        return Components(int(self.count[i, j]), int(self.set_cells[i, j]), int(self.largest[i, j]), self.by_size[i, j].copy(),
                          self.threshold, self.above, self.connectivity)


def region_components_fields(context: "HipContext", fields: Sequence["HipConcentration"], region,
                             thresholds: Sequence[Sequence[float]], above: Sequence[bool],
                             connectivity: int = 8) -> List[List[RegionComponents]]:
    """``gs_fields_region_components``: the connected components of every region of 1..4 planes of one shape in one call
    (blocking; collective in a multi-process context) -- plane i at each of ``thresholds[i]`` (1..4 per plane, the same number
    for every plane) with the sense ``above[i]`` under ``connectivity`` 4 or 8, a region's border being a wall.  Returns one
    list of ``RegionComponents`` per plane, one entry per threshold."""
    n, nt, thr, sense = _field_thresholds(fields, thresholds, above)
    rh, rw = region_shape(region)
    shape = fields[0].shape() if fields else (0, 0)
    try:
        grid = region_grid(shape[0], shape[1], (rh, rw))
    except capi.GsError:
        grid = (0, 0)  # (the call below refuses it, in the header's order)
    out = np.zeros((max(n, 1),) + grid + (max(nt, 1), 35), np.uint64)
    capi.check(context._lib.gs_fields_region_components(context.handle, _handle_array(fields), n, rh, rw, thr, sense, nt,
                                                        int(connectivity), out.ctypes.data_as(ctypes.POINTER(capi.GsComponents))))
    return [[RegionComponents.from_counters(out[i, :, :, k], thr[i * nt + k], above[i], connectivity, (rh, rw), shape)
             for k in range(nt)] for i in range(n)]


COMPONENT_RECORD_DTYPE = np.dtype([("size", np.uint64), ("sum_row", np.uint64), ("sum_col", np.uint64),
                                   ("first_row", np.uint32), ("first_col", np.uint32), ("row_min", np.uint32),
                                   ("row_max", np.uint32), ("col_min", np.uint32), ("col_max", np.uint32)])  # gs_component_record


@dataclass(frozen=True, eq=False)
class ComponentList:
    """One record per connected component of one thresholded plane, formed on the device (``gs_field_component_list``; the
    rule is include/gs_hip.h's, that of ``Components``): ``records`` is a structured array of ``COMPONENT_RECORD_DTYPE`` --
    cells, sums of the cells' row and column indices, first cell in row-major order, bounding box (inclusive) -- of the
    components of at least ``min_size`` cells, in ascending (first_row, first_col) order: the order in which
    ``scipy.ndimage.label`` numbers them.  All exact integers."""

    records: np.ndarray
    rows: int
    cols: int
    threshold: float
    above: bool
    connectivity: int
    min_size: int

    @property
    def count(self) -> int:
        return int(self.records.shape[0])

    @property
    def sizes(self) -> np.ndarray:
        return self.records["size"]

    def centroids(self) -> np.ndarray:
        """``(n, 2)`` float64: (row, column) = sum / size."""
        size = self.records["size"].astype(np.float64)
        return np.stack([self.records["sum_row"] / size, self.records["sum_col"] / size], axis=1).reshape(-1, 2)

    def boxes(self) -> np.ndarray:
        """``(n, 4)`` int64: row_min, row_max, col_min, col_max, inclusive."""
        return np.stack([self.records[k].astype(np.int64) for k in ("row_min", "row_max", "col_min", "col_max")], axis=1).reshape(-1, 4)

    def first_cells(self) -> np.ndarray:
        """``(n, 2)`` int64: every component's first cell in row-major order."""
        return np.stack([self.records["first_row"].astype(np.int64), self.records["first_col"].astype(np.int64)], axis=1).reshape(-1, 2)

    def touches_edge(self) -> np.ndarray:
        """``(n,)`` bool: the bounding box reaches the first or last row or column of the plane."""
        r = self.records
        return ((r["row_min"] == 0) | (r["col_min"] == 0) | (r["row_max"] == max(self.rows - 1, 0)) |
                (r["col_max"] == max(self.cols - 1, 0)))


def _species_plane(species: str, u, v):
    if species not in ("u", "v"):
        raise ValueError("species %r (\"u\" or \"v\")" % (species,))
    return u if species == "u" else v


def _copy_planes(planes, offsets, items, dtype) -> Tuple[np.ndarray, np.ndarray]:
    """(offsets as int64, the items as a structured array of ``dtype``) of a list's or a match's view, copied out."""
    off = np.ctypeslib.as_array(offsets, shape=(planes.value + 1,)).astype(np.int64) if planes.value else np.zeros(1, np.int64)
    n = int(off[-1])
    out = np.zeros(n, dtype)
    if n:
        ctypes.memmove(out.ctypes.data, items, n * dtype.itemsize)
    return off, out


def _copy_lists(lib, handle, shape, threshold, above, connectivity, min_size) -> List[ComponentList]:
    """The planes of a ``gs_component_list`` copied out; the handle stays the caller's."""
    planes, offsets = ctypes.c_uint64(0), ctypes.POINTER(ctypes.c_uint64)()
    records = ctypes.POINTER(capi.GsComponentRecord)()
    capi.check(lib.gs_component_list_view(handle, ctypes.byref(planes), ctypes.byref(offsets), ctypes.byref(records)))
    off, rec = _copy_planes(planes, offsets, records, COMPONENT_RECORD_DTYPE)
    thr = float(np.float32(threshold))
    return [ComponentList(rec[off[i]:off[i + 1]].copy(), int(shape[0]), int(shape[1]), thr, bool(above), int(connectivity),
                          int(min_size)) for i in range(planes.value)]


def _component_lists(lib, handle, shape, threshold, above, connectivity, min_size) -> List[ComponentList]:
    """The planes of a ``gs_component_list`` copied out; the handle is destroyed at once."""
    try:
        return _copy_lists(lib, handle, shape, threshold, above, connectivity, min_size)
    finally:
        lib.gs_component_list_destroy(handle)


def component_list_field(context: "HipContext", field: "HipConcentration", threshold: float, above: bool = True,
                         connectivity: int = 8, min_size: int = 1) -> ComponentList:
    """``gs_field_component_list``: one record per connected component of at least ``min_size`` cells of one plane over the
    whole global grid (single-process contexts), thresholded at ``threshold`` with the sense ``above`` under ``connectivity``
    4 or 8."""
    h = ctypes.c_void_p()
    capi.check(context._lib.gs_field_component_list(context.handle, field.handle, float(threshold), 1 if above else 0,
                                                    int(connectivity), int(min_size), ctypes.byref(h)))
    return _component_lists(context._lib, h, field.shape(), threshold, above, connectivity, min_size)[0]


COMPONENT_OVERLAP_DTYPE = np.dtype([("before", np.uint32), ("after", np.uint32), ("cells", np.uint64)])  # gs_component_overlap


@dataclass(frozen=True, eq=False)
class ComponentMatch:
    """What became of the components of one thresholded plane between two states, formed on the device (``gs_fields_match``;
    the rule is include/gs_hip.h's, that of ``ComponentList``): ``before`` and ``after`` are the two states' component lists
    and ``overlaps`` a structured array of ``COMPONENT_OVERLAP_DTYPE`` -- (before, after, cells): record ``before`` of the
    first list and record ``after`` of the second share ``cells`` grid cells -- with one entry per pair that shares a cell,
    in ascending (before, after) order.  A record's DEGREE is the number of its partners.  All exact integers but
    ``displacements``."""

    before: ComponentList
    after: ComponentList
    overlaps: np.ndarray

    def degree_before(self) -> np.ndarray:
        """``(before.count,)`` int64: the after-records every before-record overlaps."""
        return np.bincount(self.overlaps["before"].astype(np.int64), minlength=self.before.count).astype(np.int64)

    def degree_after(self) -> np.ndarray:
        """``(after.count,)`` int64: the before-records every after-record overlaps."""
        return np.bincount(self.overlaps["after"].astype(np.int64), minlength=self.after.count).astype(np.int64)

    def continued(self) -> np.ndarray:
        """``(k, 2)`` int64: the pairs (before, after) that have no other partner on either side."""
        b, a = self.overlaps["before"].astype(np.int64), self.overlaps["after"].astype(np.int64)
        keep = (self.degree_before()[b] == 1) & (self.degree_after()[a] == 1)
        return np.stack([b[keep], a[keep]], axis=1).reshape(-1, 2)

    def split(self) -> np.ndarray:
        """int64: the before-records with two partners or more."""
        return np.flatnonzero(self.degree_before() >= 2).astype(np.int64)

    def merged(self) -> np.ndarray:
        """int64: the after-records with two partners or more."""
        return np.flatnonzero(self.degree_after() >= 2).astype(np.int64)

    def born(self) -> np.ndarray:
        """int64: the after-records without a partner."""
        return np.flatnonzero(self.degree_after() == 0).astype(np.int64)

    def died(self) -> np.ndarray:
        """int64: the before-records without a partner."""
        return np.flatnonzero(self.degree_before() == 0).astype(np.int64)

    def children(self, i: int) -> np.ndarray:
        """int64: the after-records that before-record ``i`` overlaps, ascending."""
        return self.overlaps["after"][self.overlaps["before"] == int(i)].astype(np.int64)

    def parents(self, j: int) -> np.ndarray:
        """int64: the before-records that after-record ``j`` overlaps, ascending."""
        return self.overlaps["before"][self.overlaps["after"] == int(j)].astype(np.int64)

    def displacements(self) -> np.ndarray:
        """``(k, 2)`` float64: the after centroid minus the before centroid, (rows, columns), of the ``continued`` pairs."""
        pairs = self.continued()
        return (self.after.centroids()[pairs[:, 1]] - self.before.centroids()[pairs[:, 0]]).reshape(-1, 2)

    def counts(self) -> dict:
        """The five event counts: continued pairs, split before-records, merged after-records, born, died."""
        return {"continued": int(self.continued().shape[0]), "split": int(self.split().size), "merged": int(self.merged().size),
                "born": int(self.born().size), "died": int(self.died().size)}


def _component_matches(lib, handle, shape, threshold, above, connectivity, min_size) -> List[ComponentMatch]:
    """The planes of a ``gs_component_match`` copied out; the handle is destroyed at once, and its two lists with it."""
    try:
        before, after = ctypes.c_void_p(), ctypes.c_void_p()
        planes, offsets = ctypes.c_uint64(0), ctypes.POINTER(ctypes.c_uint64)()
        overlaps = ctypes.POINTER(capi.GsComponentOverlap)()
        capi.check(lib.gs_component_match_view(handle, ctypes.byref(before), ctypes.byref(after), ctypes.byref(planes),
                                               ctypes.byref(offsets), ctypes.byref(overlaps)))
        off, ov = _copy_planes(planes, offsets, overlaps, COMPONENT_OVERLAP_DTYPE)
        rule = (shape, threshold, above, connectivity, min_size)
        lists_b, lists_a = _copy_lists(lib, before, *rule), _copy_lists(lib, after, *rule)
    finally:
        lib.gs_component_match_destroy(handle)
    return [ComponentMatch(lists_b[i], lists_a[i], ov[off[i]:off[i + 1]].copy()) for i in range(planes.value)]


def match_fields(context: "HipContext", before: "HipConcentration", after: "HipConcentration", threshold: float,
                 above: bool = True, connectivity: int = 8, min_size: int = 1) -> ComponentMatch:
    """``gs_fields_match``: the component lists of two planes of one shape under one rule and the overlaps of their
    components, over the whole global grid (single-process contexts)."""
    h = ctypes.c_void_p()
    capi.check(context._lib.gs_fields_match(context.handle, before.handle, after.handle, float(threshold), 1 if above else 0,
                                            int(connectivity), int(min_size), ctypes.byref(h)))
    return _component_matches(context._lib, h, after.shape(), threshold, above, connectivity, min_size)[0]


CORRELATION_STEPS = ((0, 1), (1, 0), (1, 1), (1, -1))  # e_k = (dr, dc): along a row, down a column, diagonal, anti-diagonal


def pairs_total(rows: int, cols: int, max_lag: int) -> np.ndarray:
    """``N[k, d]``, the number of cell pairs {p, p + d e_k} inside a grid of rows x cols cells, d = 0 .. max_lag: geometry,
    ``max(rows - d dr, 0) * max(cols - d |dc|, 0)`` (include/gs_hip.h)."""
    d = np.arange(max_lag + 1, dtype=np.int64)
    return np.stack([np.maximum(rows - d * dr, 0) * np.maximum(cols - d * abs(dc), 0) for dr, dc in CORRELATION_STEPS])


@dataclass(frozen=True, eq=False)
class Correlation:
    """The two-point pair counts of one thresholded plane, counted on the device (``gs_fields_correlation``; the rule is
    include/gs_hip.h's): a cell is set when it is above ``threshold`` (``above``) or below it, and ``pairs[k, d]`` is the
    number of cell pairs {p, p + d e_k}, d = 0 .. ``max_lag``, inside the grid with both cells set, for the four unit steps
    e_k of ``CORRELATION_STEPS``.  Pairs never wrap.  Everything else is computed here from these integers."""

    pairs: np.ndarray
    threshold: float
    above: bool
    rows: int
    cols: int

    @classmethod
    def from_pairs(cls, pairs, threshold: float, above: bool, rows: int, cols: int) -> "Correlation":
        p = np.array(pairs, np.uint64)
        return cls(p.reshape(4, p.size // 4), float(threshold), bool(above), int(rows), int(cols))

    @property
    def max_lag(self) -> int:
        return self.pairs.shape[1] - 1

    @property
    def lags(self) -> np.ndarray:
        return np.arange(self.max_lag + 1, dtype=np.int64)

    def pairs_set(self, k: int) -> np.ndarray:
        """Pairs along e_k with both cells set, by lag (uint64)."""
        return self.pairs[k]

    def pairs_total(self, k: int) -> np.ndarray:
        """Pairs along e_k that exist inside the grid, by lag (int64)."""
        return pairs_total(self.rows, self.cols, self.max_lag)[k]

    @property
    def fraction(self) -> float:
        """Set cells over cells."""
        cells = self.rows * self.cols
        return int(self.pairs[0, 0]) / cells if cells else float("nan")

    def s2(self, k: int) -> np.ndarray:
        """The two-point probability along e_k: set pairs over pairs, f64; NaN where no pair exists."""
        total = self.pairs_total(k).astype(np.float64)
        out = np.full(total.shape, np.nan)
        np.divide(self.pairs[k].astype(np.float64), total, out=out, where=total > 0)
        return out

    def autocovariance(self, k: int) -> np.ndarray:
        """``s2(k) - fraction ** 2``: positive where cells that far apart tend to be alike, 0 where they are unrelated."""
        return self.s2(k) - self.fraction ** 2

    def distance(self, k: int) -> np.ndarray:
        """The length of d e_k in cells: d along rows and columns, d sqrt(2) along the diagonals."""
        return self.lags * (1.0 if k < 2 else float(np.sqrt(2.0)))

    def first_zero_crossing(self, k: int) -> Optional[float]:
        """The lag (in steps of e_k, linearly interpolated) at which the autocovariance first reaches 0 from above."""
        c = self.autocovariance(k)
        for d in range(1, c.size):
            if np.isnan(c[d]) or np.isnan(c[d - 1]):
                return None
            if c[d - 1] > 0.0 and c[d] <= 0.0:
                return (d - 1) + c[d - 1] / (c[d - 1] - c[d])
        return None

    def first_minimum(self, k: int) -> Optional[int]:
        """The first lag d >= 1 whose autocovariance is below that of d - 1 and not above that of d + 1 -- half the
        pattern's wavelength along e_k -- or None when there is none inside the lags."""
        c = self.autocovariance(k)
        for d in range(1, c.size - 1):
            if np.isnan(c[d + 1]):
                return None
            if c[d] < c[d - 1] and c[d] <= c[d + 1]:
                return d
        return None

    def first_maximum_after_minimum(self, k: int) -> Optional[int]:
        """The first lag beyond ``first_minimum`` whose autocovariance is above that of d - 1 and not below that of d + 1 --
        the pattern's wavelength along e_k -- or None."""
        m = self.first_minimum(k)
        if m is None:
            return None
        c = self.autocovariance(k)
        for d in range(m + 1, c.size - 1):
            if np.isnan(c[d + 1]):
                return None
            if c[d] > c[d - 1] and c[d] >= c[d + 1]:
                return d
        return None


def correlation_fields(context: "HipContext", fields: Sequence["HipConcentration"], thresholds: Sequence[Sequence[float]],
                       above: Sequence[bool], max_lag: int = 32) -> List[List[Correlation]]:
    """``gs_fields_correlation``: two-point pair counts of 1..4 planes of one shape over the whole global grid in one call
    (collective in a multi-process context) -- plane i at each of ``thresholds[i]`` (1..4 per plane, the same number for
    every plane; all counted in one pass) with the sense ``above[i]``, lags 0 .. ``max_lag`` (1..64).  Returns one list of
    ``Correlation`` per plane."""
    n, nt, thr, sense = _field_thresholds(fields, thresholds, above)
    lags = max_lag + 1 if 1 <= max_lag <= 64 else 1
    out = np.zeros((max(n, 1), max(nt, 1), 4, lags), np.uint64)
    capi.check(context._lib.gs_fields_correlation(context.handle, _handle_array(fields), n, thr, sense, nt, max_lag,
                                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
    rows, cols = fields[0].shape()
    return [[Correlation.from_pairs(out[i, k], thr[i * nt + k], above[i], rows, cols) for k in range(nt)] for i in range(n)]


SPECTRUM_TILES = (16, 32, 64, 128)
SPECTRUM_WINDOWS = {"none": 0, "hann": 1}


def spectrum_tables(tile: int) -> Tuple[np.ndarray, np.ndarray]:
    """``gs_spectrum_tables``: the periodic Hann window ``h[tile]`` (f32) and the twiddles ``W[tile / 2]`` (complex64) that
    the device uses (include/gs_hip.h); needs no device."""
    h = np.zeros(tile, np.float32)
    w = np.zeros(max(tile // 2, 1) * 2, np.float32)
    f32p = ctypes.POINTER(ctypes.c_float)
    capi.check(capi.load().gs_spectrum_tables(int(tile), h.ctypes.data_as(f32p), w.ctypes.data_as(f32p)))
    return h, w.view(np.complex64)[:tile // 2]


def _spectrum_window(window) -> int:
    if isinstance(window, str):
        return SPECTRUM_WINDOWS.get(window, -1)
    return int(window)


@dataclass(frozen=True, eq=False)
class Spectrum:
    """The tile-averaged power spectrum of one plane, summed on the device (``gs_fields_spectrum``; the rule is
    include/gs_hip.h's): ``raw[kr, kc]`` is the sum over the whole ``tile`` x ``tile`` tiles of the plane that hold only
    finite cells of |FFT2(window * (tile - its mean))|^2, kr < tile, kc <= tile / 2 (the other half is its mirror image),
    ``tiles_used`` and ``tiles_skipped`` count those tiles and the ones left out.  Everything else is computed here.
    Frequencies are in cycles per cell: f_r = kr / tile folded into [-1/2, 1/2), f_c = kc / tile."""

    raw: np.ndarray
    tile: int
    window: int
    tiles_used: int
    tiles_skipped: int

    @classmethod
    def from_raw(cls, raw, tile: int, window, tiles=(1, 0)) -> "Spectrum":
        tile = int(tile)
        p = np.array(raw, np.float64).reshape(tile, tile // 2 + 1)
        return cls(p, tile, _spectrum_window(window), int(tiles[0]), int(tiles[1]))

    @property
    def window_energy(self) -> float:
        """The sum of (h_r h_c)^2 over a tile: tile^2 without a window."""
        if not self.window:
            return float(self.tile * self.tile)
        h = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(self.tile) / self.tile)
        return float(np.sum(h * h) ** 2)

    @property
    def power(self) -> np.ndarray:
        """The mean over the tiles used, divided by the window's energy: f64 ``[tile, tile / 2 + 1]``; NaN without a tile."""
        if self.tiles_used == 0:
            return np.full(self.raw.shape, np.nan)
        return self.raw / (self.tiles_used * self.window_energy)

    def frequencies(self) -> Tuple[np.ndarray, np.ndarray]:
        """(f_r[tile], f_c[tile / 2 + 1]) in cycles per cell; f_r is signed."""
        T = self.tile
        k = np.arange(T)
        return np.where(k < T // 2, k, k - T) / T, np.arange(T // 2 + 1) / T

    def _rings(self) -> Tuple[np.ndarray, np.ndarray]:
        fr, fc = self.frequencies()
        ring = np.rint(self.tile * np.sqrt(fr[:, None] ** 2 + fc[None, :] ** 2)).astype(np.int64)
        kc = np.arange(self.tile // 2 + 1)
        weight = np.broadcast_to(np.where((kc > 0) & (kc < self.tile // 2), 2.0, 1.0), ring.shape)
        return ring, weight

    def radial(self) -> np.ndarray:
        """S(|k|) on rings 0 .. tile / 2: ring round(tile sqrt(f_r^2 + f_c^2)) takes every bin with the weight 2 for
        0 < kc < tile / 2 (the bin stands for its mirror image too), else 1; a ring's value is the weighted mean of its
        bins, bins beyond the last ring are dropped."""
        ring, weight = self._rings()
        keep = ring <= self.tile // 2
        n = self.tile // 2 + 1
        total = np.bincount(ring[keep], weights=(weight * self.power)[keep], minlength=n)
        return total / np.bincount(ring[keep], weights=weight[keep], minlength=n)

    def peak_wavenumber(self) -> Optional[float]:
        """The pattern's wavenumber in cycles per cell: the largest ring among 1 .. tile / 2 - 1 of ``radial``, refined by
        a parabola through it and its neighbours; None for a flat spectrum (or none at all)."""
        s = self.radial()
        inner = s[1:self.tile // 2]
        if not np.all(np.isfinite(s)) or not inner.max() > inner.min():
            return None
        k = 1 + int(np.argmax(inner))
        a, b, c = s[k - 1], s[k], s[k + 1]
        bend = a - 2.0 * b + c
        shift = 0.5 * (a - c) / bend if bend < 0.0 else 0.0
        return (k + min(max(shift, -0.5), 0.5)) / self.tile

    def wavelength(self) -> Optional[float]:
        """Cells per period: 1 / ``peak_wavenumber``; None where that is."""
        k = self.peak_wavenumber()
        return 1.0 / k if k else None

    def _moments(self) -> Optional[Tuple[float, float, float]]:
        k = self.peak_wavenumber()
        if k is None:
            return None
        ring, weight = self._rings()
        near = np.abs(ring - int(round(k * self.tile))) <= 1
        fr, fc = self.frequencies()
        w = np.where(near, weight * self.power, 0.0)
        total = w.sum()
        if not total > 0.0:
            return None
        # (a bin and its mirror image (-f_r, -f_c) have the same products: the half plane's moments are the plane's)
        return (float((w * fr[:, None] ** 2).sum() / total), float((w * fc[None, :] ** 2).sum() / total),
                float((w * fr[:, None] * fc[None, :]).sum() / total))

    def orientation(self) -> Optional[float]:
        """The direction of the pattern's wave vector in degrees in [0, 180), measured from the column axis towards the
        row axis: 0 for a pattern that varies along a row (stripes that run down the columns), 90 for one that varies
        down a column -- the principal axis of the power-weighted second moments of (f_r, f_c) over the peak ring +- 1."""
        m = self._moments()
        if m is None:
            return None
        rr, cc, rc = m
        return float(np.degrees(0.5 * np.arctan2(2.0 * rc, cc - rr)) % 180.0)

    def anisotropy(self) -> Optional[float]:
        """0 for power spread evenly over the peak ring, 1 for a single direction: (l1 - l2) / (l1 + l2) of the eigenvalues
        of those second moments."""
        m = self._moments()
        if m is None:
            return None
        rr, cc, rc = m
        return float(np.hypot(cc - rr, 2.0 * rc) / (cc + rr)) if cc + rr > 0.0 else None


def _spectrum_outputs(planes: int, tile: int):
    t = tile if tile in SPECTRUM_TILES else 16  # (a refused tile: the call returns before it writes)
    power = np.zeros((max(planes, 0), t, t // 2 + 1), np.float64)
    tiles = np.zeros((max(planes, 0), 2), np.uint64)
    return power, tiles


def spectrum_fields(context: "HipContext", fields: Sequence["HipConcentration"], tile: int = 64, window="hann") -> List[Spectrum]:
    """``gs_fields_spectrum``: the tile-averaged power spectra of 1..4 planes of one shape over the whole global grid in one
    call (collective in a multi-process context) -- tiles of ``tile`` (16, 32, 64, 128) cells a side, ``window`` "hann" or
    "none".  Returns one ``Spectrum`` per plane."""
    n, tile, win = len(fields), int(tile), _spectrum_window(window)
    power, tiles = _spectrum_outputs(n if 1 <= n <= 4 else 4, tile)
    capi.check(context._lib.gs_fields_spectrum(context.handle, _handle_array(fields), n, tile, win,
                                               power.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                               tiles.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
    return [Spectrum.from_raw(power[i], tile, win, tiles[i]) for i in range(n)]


@dataclass(frozen=True, eq=False)
class RegionCorrelation:
    """The two-point pair counts of every region of one thresholded plane, counted on the device
    (``gs_fields_region_correlation``): ``pairs`` of shape ``(RR, RC, 4, L + 1)``, entry (i, j) being the ``Correlation.pairs``
    of a plane that holds region (i, j)'s cells alone -- a pair across a region border is never formed.  ``cells`` is every
    region's number of cells; the derived arrays are ``Correlation``'s, region by region."""

    pairs: np.ndarray
    threshold: float
    above: bool
    cells: np.ndarray
    region: Tuple[int, int]
    shape: Tuple[int, int]

    @classmethod
    def from_pairs(cls, pairs, threshold: float, above: bool, region, shape) -> "RegionCorrelation":
        pairs = np.array(pairs, np.uint64)
        region, shape = region_shape(region), (int(shape[0]), int(shape[1]))
        return cls(pairs, float(threshold), bool(above), region_sizes(shape[0], shape[1], region, pairs.shape[:2]), region, shape)

    @property
    def max_lag(self) -> int:
        return self.pairs.shape[3] - 1

    def totals(self) -> np.ndarray:
        """The pairs that exist inside every region's own h x w cells, N_k(d), as int64 ``(RR, RC, 4, L + 1)``."""
        rr, rc = self.pairs.shape[:2]
        h = np.minimum(self.region[0], self.shape[0] - self.region[0] * np.arange(rr, dtype=np.int64))[:, None, None]
        w = np.minimum(self.region[1], self.shape[1] - self.region[1] * np.arange(rc, dtype=np.int64))[None, :, None]
        d = np.arange(self.max_lag + 1, dtype=np.int64)[None, None, :]
        return np.stack([np.maximum(h - d * dr, 0) * np.maximum(w - d * abs(dc), 0) for dr, dc in CORRELATION_STEPS], axis=2)

    def s2(self, k: int) -> np.ndarray:
        """Per region, ``Correlation.s2(k)``: f64 ``(RR, RC, L + 1)``, NaN where no pair exists."""
        total = self.totals()[:, :, k].astype(np.float64)
        out = np.full(total.shape, np.nan)
        np.divide(self.pairs[:, :, k].astype(np.float64), total, out=out, where=total > 0)
        return out

    def autocovariance(self, k: int) -> np.ndarray:
        """Per region, ``Correlation.autocovariance(k)``: ``s2(k)`` minus the square of the region's set fraction."""
        cells = self.cells.astype(np.float64)
        fraction = np.full(cells.shape, np.nan)
        np.divide(self.pairs[:, :, 0, 0].astype(np.float64), cells, out=fraction, where=cells > 0)
        return self.s2(k) - (fraction ** 2)[:, :, None]

    def _per_region(self, name: str, k: int) -> np.ndarray:
        out = np.full(self.pairs.shape[:2], -1, np.int64)
        for i, j in np.ndindex(out.shape):
            found = getattr(self.at(i, j), name)(k)
            out[i, j] = -1 if found is None else found
        return out

    def first_minimum(self, k: int) -> np.ndarray:
        """Per region, ``Correlation.first_minimum(k)`` -- half the wavelength along e_k -- as int64, -1 where there is none."""
        return self._per_region("first_minimum", k)

    def first_maximum_after_minimum(self, k: int) -> np.ndarray:
        """Per region, ``Correlation.first_maximum_after_minimum(k)`` -- the wavelength along e_k --, -1 where there is none."""
        return self._per_region("first_maximum_after_minimum", k)

    def at(self, i: int, j: int) -> Correlation:
        h = min(self.region[0], self.shape[0] - self.region[0] * i)
        w = min(self.region[1], self.shape[1] - self.region[1] * j)
        return Correlation.from_pairs(self.pairs[i, j], self.threshold, self.above, h, w)


def region_correlation_fields(context: "HipContext", fields: Sequence["HipConcentration"], region,
                              thresholds: Sequence[Sequence[float]], above: Sequence[bool],
                              max_lag: int = 32) -> List[List[RegionCorrelation]]:
    """``gs_fields_region_correlation``: the two-point pair counts of every region of 1..4 planes of one shape in one call
    (blocking; collective in a multi-process context) -- plane i at each of ``thresholds[i]`` (1..4 per plane, one pass) with
    the sense ``above[i]``, lags 0 .. ``max_lag`` (1..64).  Returns one list of ``RegionCorrelation`` per plane, one entry
    per threshold."""
    n, nt, thr, sense = _field_thresholds(fields, thresholds, above)
    rh, rw = region_shape(region)
    shape = fields[0].shape() if fields else (0, 0)
    lags = max_lag + 1 if 1 <= max_lag <= 64 else 1
    try:
        grid = region_grid(shape[0], shape[1], (rh, rw))
        if grid[0] * grid[1] * max(nt, 1) * 4 * lags > capi.GS_REGION_PAIRS_MAX:
            grid = (0, 0)
    except capi.GsError:
        grid = (0, 0)  # (the call below refuses it, in the header's order)
    out = np.zeros((max(n, 1),) + grid + (max(nt, 1), 4, lags), np.uint64)
    capi.check(context._lib.gs_fields_region_correlation(context.handle, _handle_array(fields), n, rh, rw, thr, sense, nt,
                                                         max_lag, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
    return [[RegionCorrelation.from_pairs(out[i, :, :, k], thr[i * nt + k], above[i], (rh, rw), shape) for k in range(nt)]
            for i in range(n)]


@dataclass(frozen=True, eq=False)
class RegionHistogram:
    """The histograms of every region of one plane, counted on the device (``gs_fields_region_histogram``): ``counts`` of shape
    ``(RR, RC, bins)``, ``below`` / ``above`` / ``nan`` of shape ``(RR, RC)``, entry (i, j) being bit for bit the ``Histogram``
    of a plane that holds region (i, j)'s cells alone over ``[lo, hi]``.  ``cells`` is every region's number of cells -- the
    sum of its counters --, ``region`` is ``(rh, rw)``, ``shape`` the plane's.  ``fraction_above`` and ``quantile`` are
    ``Histogram``'s, region by region."""

    counts: np.ndarray
    below: np.ndarray
    above: np.ndarray
    nan: np.ndarray
    lo: float
    hi: float
    cells: np.ndarray
    region: Tuple[int, int]
    shape: Tuple[int, int]

    @classmethod
    def from_counters(cls, c, lo: float, hi: float, region, shape) -> "RegionHistogram":
        """From ``(RR, RC, bins + 3)`` counters as the C ABI writes them: per region counts, below, above, nan."""
        c = np.asarray(c, np.uint64)
        region, shape = region_shape(region), (int(shape[0]), int(shape[1]))
        return cls(c[:, :, :-3].copy(), c[:, :, -3].copy(), c[:, :, -2].copy(), c[:, :, -1].copy(), float(lo), float(hi),
                   region_sizes(shape[0], shape[1], region, c.shape[:2]), region, shape)

    @property
    def bins(self) -> int:
        return self.counts.shape[2]

    @property
    def in_range(self) -> np.ndarray:
        """Per region, the cells inside ``[lo, hi]``: the ones ``counts`` holds.  uint64 ``(RR, RC)``."""
        return self.counts.sum(axis=2, dtype=np.uint64)

    def edges(self) -> np.ndarray:
        """``Histogram.edges``: the ``bins + 1`` nominal bin edges in f64, the same for every region."""
        return self.lo + (self.hi - self.lo) * np.arange(self.bins + 1, dtype=np.float64) / self.bins

    def fraction_above(self, x: float) -> np.ndarray:
        """Per region, ``Histogram.fraction_above(x)``: f64 ``(RR, RC)``, NaN where no cell of the region is in range."""
        total = self.in_range.astype(np.float64)
        first = int(np.searchsorted(self.edges()[:-1], x, side="left"))
        out = np.full(total.shape, np.nan)
        np.divide(self.counts[:, :, first:].sum(axis=2, dtype=np.uint64).astype(np.float64), total, out=out, where=total > 0)
        return out

    def quantile(self, q: float) -> np.ndarray:
        """Per region, ``Histogram.quantile(q)``: f64 ``(RR, RC)``, NaN where no cell of the region is in range."""
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"quantile {q} outside [0, 1]")
        total = self.in_range
        need = np.maximum(1, np.ceil(q * total.astype(np.float64))).astype(np.uint64)
        cum = np.cumsum(self.counts, axis=2, dtype=np.uint64)
        index = (cum < need[:, :, None]).sum(axis=2)  # the first bin at which the cumulative count reaches `need`
        return np.where(total > 0, self.edges()[np.minimum(index, self.bins - 1) + 1], np.nan)

    def at(self, i: int, j: int) -> Histogram:
        return Histogram(self.counts[i, j].copy(), int(self.below[i, j]), int(self.above[i, j]), int(self.nan[i, j]), self.lo,
                         self.hi, int(self.cells[i, j]))


def region_histogram_fields(context: "HipContext", fields: Sequence["HipConcentration"], region, bins: int,
                            ranges: Sequence[Tuple[float, float]]) -> List[RegionHistogram]:
    """``gs_fields_region_histogram``: the histograms of every region of 1..4 planes of one shape in one call (blocking;
    collective in a multi-process context), plane i over ``ranges[i]`` with ``bins`` (1..4096) bins.  Returns one
    ``RegionHistogram`` per plane."""
    n, bins = len(fields), int(bins)
    if len(ranges) != n:
        raise ValueError("one (lo, hi) range per field")
    rh, rw = region_shape(region)
    shape = fields[0].shape() if fields else (0, 0)
    slots = bins + 3 if 1 <= bins <= 4096 else 3
    try:
        grid = region_grid(shape[0], shape[1], (rh, rw))
        if grid[0] * grid[1] * slots > capi.GS_REGION_HIST_MAX:
            grid = (0, 0)
    except capi.GsError:
        grid = (0, 0)  # (the call below refuses it, in the header's order)
    lo, hi = _f32_pairs(ranges)
    out = np.zeros((max(n, 1),) + grid + (slots,), np.uint64)
    capi.check(context._lib.gs_fields_region_histogram(context.handle, _handle_array(fields), n, rh, rw, lo, hi, bins,
                                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
    return [RegionHistogram.from_counters(out[i], lo[i], hi[i], (rh, rw), shape) for i in range(n)]


@dataclass(frozen=True, eq=False)
class RegionSpectrum:
    """The tile-averaged power spectra of every region of one plane, summed on the device (``gs_fields_region_spectrum``):
    ``raw`` of shape ``(RR, RC, tile, tile / 2 + 1)``, ``tiles_used`` / ``tiles_skipped`` of shape ``(RR, RC)``, entry (i, j)
    being bit for bit the ``Spectrum`` of a plane that holds region (i, j)'s cells alone -- tiles anchored at the region's
    first row and column, a region in which no tile fits all zeros.  ``region`` is ``(rh, rw)``, ``shape`` the plane's.  The
    array methods are ``Spectrum``'s, region by region, NaN where ``Spectrum``'s gives None."""

    raw: np.ndarray
    tiles_used: np.ndarray
    tiles_skipped: np.ndarray
    tile: int
    window: int
    region: Tuple[int, int]
    shape: Tuple[int, int]

    @classmethod
    def from_raw(cls, raw, tiles, tile: int, window, region, shape) -> "RegionSpectrum":
        """From ``(RR, RC, tile, tile / 2 + 1)`` sums and ``(RR, RC, 2)`` counts {used, skipped} as the C ABI writes them."""
        tile = int(tile)
        tiles = np.asarray(tiles, np.uint64)
        rr, rc = tiles.shape[:2]
        p = np.array(raw, np.float64).reshape(rr, rc, tile, tile // 2 + 1)
        return cls(p, tiles[:, :, 0].copy(), tiles[:, :, 1].copy(), tile, _spectrum_window(window), region_shape(region),
                   (int(shape[0]), int(shape[1])))

    def at(self, i: int, j: int) -> Spectrum:
        return Spectrum(self.raw[i, j].copy(), self.tile, self.window, int(self.tiles_used[i, j]), int(self.tiles_skipped[i, j]))

    @property
    def power(self) -> np.ndarray:
        """Per region, ``Spectrum.power``: f64 ``(RR, RC, tile, tile / 2 + 1)``, NaN where a region used no tile."""
        out = np.full(self.raw.shape, np.nan)
        for i, j in np.ndindex(*self.tiles_used.shape):
            out[i, j] = self.at(i, j).power
        return out

    def radial(self) -> np.ndarray:
        """Per region, ``Spectrum.radial()``: f64 ``(RR, RC, tile / 2 + 1)``."""
        out = np.full(self.tiles_used.shape + (self.tile // 2 + 1,), np.nan)
        for i, j in np.ndindex(*self.tiles_used.shape):
            out[i, j] = self.at(i, j).radial()
        return out

    def _each(self, method: str) -> np.ndarray:
        out = np.full(self.tiles_used.shape, np.nan)
        for i, j in np.ndindex(*self.tiles_used.shape):
            value = getattr(self.at(i, j), method)()
            if value is not None:
                out[i, j] = value
        return out

    def peak_wavenumber(self) -> np.ndarray:
        """Per region, ``Spectrum.peak_wavenumber()``: f64 ``(RR, RC)``, NaN where that is None."""
        return self._each("peak_wavenumber")

    def wavelength(self) -> np.ndarray:
        """Per region, ``Spectrum.wavelength()``: f64 ``(RR, RC)``, NaN where that is None."""
        return self._each("wavelength")

    def orientation(self) -> np.ndarray:
        """Per region, ``Spectrum.orientation()``: f64 ``(RR, RC)``, NaN where that is None."""
        return self._each("orientation")

    def anisotropy(self) -> np.ndarray:
        """Per region, ``Spectrum.anisotropy()``: f64 ``(RR, RC)``, NaN where that is None."""
        return self._each("anisotropy")


def region_spectrum_fields(context: "HipContext", fields: Sequence["HipConcentration"], region, tile: int = 64,
                           window="hann") -> List[RegionSpectrum]:
    """``gs_fields_region_spectrum``: the tile-averaged power spectra of every region of 1..4 planes of one shape in one call
    (blocking; collective in a multi-process context) -- tiles of ``tile`` (16, 32, 64, 128) cells a side anchored at every
    region's first row and column, ``window`` "hann" or "none".  Returns one ``RegionSpectrum`` per plane."""
    n, tile, win = len(fields), int(tile), _spectrum_window(window)
    rh, rw = region_shape(region)
    shape = fields[0].shape() if fields else (0, 0)
    t = tile if tile in SPECTRUM_TILES else 16  # (a refused tile: the call returns before it writes)
    try:
        grid = region_grid(shape[0], shape[1], (rh, rw))
        if grid[0] * grid[1] * (t * (t // 2 + 1) + 2) > capi.GS_REGION_SPECTRUM_MAX:
            grid = (0, 0)
    except capi.GsError:
        grid = (0, 0)  # (the call below refuses it, in the header's order)
    power = np.zeros((max(n, 1),) + grid + (t, t // 2 + 1), np.float64)
    tiles = np.zeros((max(n, 1),) + grid + (2,), np.uint64)
    capi.check(context._lib.gs_fields_region_spectrum(context.handle, _handle_array(fields), n, rh, rw, tile, win,
                                                      power.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                      tiles.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
    return [RegionSpectrum.from_raw(power[i], tiles[i], tile, win, (rh, rw), shape) for i in range(n)]


def pinned_empty(shape: Sequence[int]) -> np.ndarray:
    """float32 array in page-locked host memory (``gs_host_alloc``) for overlapped downloads.
    The allocation is released when the last view of it is garbage-collected."""
    import weakref

    lib = capi.load()
    count = int(np.prod(shape))
    ptr = ctypes.c_void_p()
    capi.check(lib.gs_host_alloc(ctypes.byref(ptr), max(count, 1) * 4))
    buf = (ctypes.c_float * max(count, 1)).from_address(ptr.value)
    root = np.frombuffer(buf, dtype=np.float32)        # every view's .base; does not own the memory
    weakref.finalize(root, lib.gs_host_free, ctypes.c_void_p(ptr.value))
    return root[:count].reshape(shape)


class HipConcentration:
    """One species plane in HBM: the ``Concentration`` implementation of this backend."""

    def __init__(self, context: HipContext, shape: Sequence[int]):
        rows, cols = int(shape[0]), int(shape[1])
        self._ctx = context
        self._h = ctypes.c_void_p()
        capi.check(context._lib.gs_field_create(context.handle, ctypes.byref(self._h), rows, cols))
        self._shape = (rows, cols)

    # -- constructors (Concentration::default / zeros / ones, mod.rs:205-218) -------------
    @classmethod
    def default(cls, context: HipContext, shape) -> "HipConcentration":
        return cls(context, shape)

    @classmethod
    def zeros(cls, context: HipContext, shape) -> "HipConcentration":
        return cls(context, shape)  # planes are created zero-filled

    @classmethod
    def ones(cls, context: HipContext, shape) -> "HipConcentration":
        c = cls(context, shape)
        capi.check(context._lib.gs_field_fill(context.handle, c._h, 1.0))
        return c

    @property
    def handle(self):
        if not self._h:
            raise GsError(capi.GS_ERR_INVALID, "concentration already destroyed")
        return self._h

    def shape(self) -> Tuple[int, int]:
        return self._shape

    def raw_shape(self) -> Tuple[int, int]:
        r, p = ctypes.c_uint64(), ctypes.c_uint64()
        capi.check(self._ctx._lib.gs_field_raw_shape(self.handle, ctypes.byref(r), ctypes.byref(p)))
        return int(r.value), int(p.value)

    def local_rows(self) -> Tuple[int, int]:
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        capi.check(self._ctx._lib.gs_field_local_rows(self.handle, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def fill_slice(self, context: HipContext, slice_: Sequence[range], value: float) -> None:
        """``fill_slice(ctx, [rows, cols], value)`` with half-open ranges (mod.rs:230-243)."""
        rr, cc = slice_
        capi.check(context._lib.gs_field_fill_slice(context.handle, self.handle, rr.start, rr.stop,
                                                    cc.start, cc.stop, value))

    def finalize(self, context: HipContext) -> None:
        capi.check(context._lib.gs_field_finalize(context.handle, self.handle))

    def upload(self, context: HipContext, host: np.ndarray) -> None:
        """Test/bench helper: overwrite this process's rows from a dense float32 array."""
        r0, r1 = self.local_rows()
        host = np.ascontiguousarray(host, np.float32)
        if host.shape != (r1 - r0, self._shape[1]):
            raise AssertionError(f"upload shape {host.shape} != local shape {(r1 - r0, self._shape[1])}")
        capi.check(context._lib.gs_field_upload(context.handle, self.handle,
                                                host.ctypes.data_as(ctypes.c_void_p)))

    def device_slabs(self):
        """``gs_field_device_ptr`` for every local slab: ``(address, pitch in f32, global row0, rows, device)``
        tuples, top to bottom -- for zero-copy consumers / producers (a producer calls ``mark_written``)."""
        out = []
        lib = self._ctx._lib
        i = 0
        while True:
            ptr, pitch, r0, rows = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            dev = ctypes.c_int32()
            if lib.gs_field_device_ptr(self.handle, i, ctypes.byref(ptr), ctypes.byref(pitch), ctypes.byref(r0),
                                       ctypes.byref(rows), ctypes.byref(dev)) != capi.GS_OK:
                break
            out.append((int(ptr.value or 0), int(pitch.value), int(r0.value), int(rows.value), int(dev.value)))
            i += 1
        return out

    def torch_views(self):
        """Zero-copy torch views of the local slabs: ``[(global row0, rows, tensor [rows, cols])]`` with the row
        pitch as stride (``__cuda_array_interface__``); for on-device comparisons and producers (a producer calls
        ``mark_written``).  The library's streams are not torch's: ``context.sync()`` before reading."""
        import torch

        class _DeviceArray:
            def __init__(self, address, rows, cols, pitch):
                self.__cuda_array_interface__ = {"shape": (rows, cols), "typestr": "<f4", "data": (address, False),
                                                 "version": 3, "strides": (pitch * 4, 4)}

        cols = self._shape[1]
        return [(row0, rows, torch.as_tensor(_DeviceArray(address, rows, cols, pitch), device=f"cuda:{device}"))
                for address, pitch, row0, rows, device in self.device_slabs() if rows > 0 and cols > 0]

    def mark_written(self, context: HipContext) -> None:
        """``gs_field_mark_written``: cells were written through ``device_slabs`` addresses."""
        capi.check(context._lib.gs_field_mark_written(context.handle, self.handle))

    def reduced_shape(self, factor: int) -> Tuple[int, int]:
        """``gs_field_reduced_shape``: this process's rows x the columns of the image reduced by ``factor`` (the plane
        averaged over ``factor`` x ``factor`` blocks on the device, include/gs_hip.h).  Raises ``GsError`` for a factor
        outside 1..64 (``GS_ERR_INVALID``) and for a slab chain some slab of which does not begin at a multiple of the
        factor (``GS_ERR_UNSUPPORTED``); the device is not touched."""
        cols, r0, r1 = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        capi.check(self._ctx._lib.gs_field_reduced_shape(self.handle, int(factor), None, ctypes.byref(cols),
                                                         ctypes.byref(r0), ctypes.byref(r1)))
        return int(r1.value) - int(r0.value), int(cols.value)

    def _reduced_target(self, target: np.ndarray, reduce: int) -> None:
        want = self.reduced_shape(reduce)
        if tuple(target.shape) != want:
            raise ValueError(f"a target of shape {tuple(target.shape)} cannot take the image reduced by {reduce}: {want}")
        if target.dtype != np.float32 or not target.flags.c_contiguous:
            raise ValueError("a target is a C-contiguous float32 array")

    def make_scalar_view(self, context: HipContext, reduce: int = 1) -> np.ndarray:
        """Owned dense copy of this process's rows (mod.rs:261-275); ``reduce`` > 1: of the reduced image."""
        if reduce != 1:
            out = np.empty(self.reduced_shape(reduce), np.float32)
            self.write_scalar_view(context, out, reduce)
            return out
        r0, r1 = self.local_rows()
        out = np.empty((r1 - r0, self._shape[1]), np.float32)
        self.write_scalar_view(context, out)
        return out

    def write_scalar_view(self, context: HipContext, target: np.ndarray, reduce: int = 1) -> None:
        """``write_scalar_view``; like ``validate_write`` (mod.rs:291-295) a shape mismatch is
        a programming error and asserts.  ``reduce`` > 1 (``gs_field_download_reduced``): ``target`` takes the image
        reduced by that factor; one of the wrong shape raises ``ValueError``."""
        if reduce != 1:
            self._reduced_target(target, reduce)
            capi.check(context._lib.gs_field_download_reduced(context.handle, self.handle, int(reduce),
                                                              target.ctypes.data_as(ctypes.c_void_p)))
            return
        r0, r1 = self.local_rows()
        assert target.shape == (r1 - r0, self._shape[1]), (target.shape, (r1 - r0, self._shape[1]))
        assert target.dtype == np.float32 and target.flags.c_contiguous
        capi.check(context._lib.gs_field_download(context.handle, self.handle,
                                                  target.ctypes.data_as(ctypes.c_void_p)))

    def write_scalar_view_after(self, context: HipContext, target: np.ndarray, reduce: int = 1) -> None:
        """``write_scalar_view_after`` (data/src/concentration/gpu/image/mod.rs:196-206): enqueue
        the download behind the steps already enqueued and return at once; ``target`` (ideally
        from ``pinned_empty``) is valid after ``context.download_wait()``.  ``reduce`` > 1
        (``gs_field_download_reduced_async``): the image reduced by that factor, 1 / reduce^2 of the bytes; a target of
        the wrong shape raises ``ValueError`` before anything is enqueued."""
        if reduce != 1:
            self._reduced_target(target, reduce)
            capi.check(context._lib.gs_field_download_reduced_async(context.handle, self.handle, int(reduce),
                                                                    target.ctypes.data_as(ctypes.c_void_p)))
            return
        r0, r1 = self.local_rows()
        assert target.shape == (r1 - r0, self._shape[1]), (target.shape, (r1 - r0, self._shape[1]))
        assert target.dtype == np.float32 and target.flags.c_contiguous
        capi.check(context._lib.gs_field_download_async(context.handle, self.handle,
                                                        target.ctypes.data_as(ctypes.c_void_p)))

    def colormap(self, context: HipContext, palette: np.ndarray, scale: float = 2.0, reduce: int = 1) -> np.ndarray:
        """The pixels ``data-to-pics`` makes of this plane (data-to-pics/src/main.rs:139-144):
        ``palette[clamp(floor(scale * value * n), 0, n - 1)]`` as uint8 ``[rows, cols, 3]``; ``palette`` is
        ``[n, 3]`` uint8 (the reference: the 256 colours of ``colorous::INFERNO``), ``scale`` its
        ``AMPLITUDE_SCALE`` = 1 / 0.5 (ui/src/lib.rs:117-123).  ``reduce`` > 1 (``gs_field_colormap_reduced``): the
        pixels of the image reduced by that factor, 3 bytes per ``reduce`` x ``reduce`` cells."""
        palette = np.ascontiguousarray(palette, np.uint8)
        assert palette.ndim == 2 and palette.shape[1] == 3 and len(palette) >= 1
        if reduce != 1:
            out = np.empty(self.reduced_shape(reduce) + (3,), np.uint8)
            capi.check(context._lib.gs_field_colormap_reduced(context.handle, self.handle, int(reduce), scale,
                                                              palette.ctypes.data_as(ctypes.c_void_p), len(palette),
                                                              out.ctypes.data_as(ctypes.c_void_p)))
            return out
        r0, r1 = self.local_rows()
        out = np.empty((r1 - r0, self._shape[1], 3), np.uint8)
        capi.check(context._lib.gs_field_colormap(context.handle, self.handle, scale,
                                                  palette.ctypes.data_as(ctypes.c_void_p), len(palette),
                                                  out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def summary(self, context: HipContext) -> Summary:
        """Sum, sum of squares, min and max of the finite cells and the non-finite count of this plane over the whole
        global grid, computed on the device (blocking; collective in a multi-process context)."""
        return summarize_fields(context, [self])[0]

    def histogram(self, context: HipContext, bins: int = 256, range: Tuple[float, float] = (0.0, 1.0)) -> Histogram:
        """How this plane's values are distributed over ``bins`` equal bins of ``range`` over the whole global grid,
        counted on the device (blocking; collective in a multi-process context)."""
        return histogram_fields(context, [self], bins, [range])[0]

    def morphology(self, context: HipContext, thresholds, above: bool = True) -> List[Morphology]:
        """The bit-quad counts of this plane thresholded at each of ``thresholds`` (1..4, one pass) over the whole global
        grid, counted on the device (``gs_fields_morphology``; blocking, collective in a multi-process context): a cell
        is set when it is above (``above``) or below the threshold."""
        return morphology_fields(context, [self], [thresholds], [above])[0]

    def region_summaries(self, context: HipContext, region) -> RegionSummaries:
        """The summary of every region of ``region`` = (rh, rw) cells (an int: square) of this plane, computed on the device
        (``gs_fields_region_summaries``; blocking, collective in a multi-process context)."""
        return region_summaries_fields(context, [self], region)[0]

    def region_morphology(self, context: HipContext, region, thresholds, above: bool = True) -> List[RegionMorphology]:
        """The bit-quad counts of every region of ``region`` = (rh, rw) cells (an int: square) of this plane thresholded at
        each of ``thresholds`` (1..4, one pass), counted on the device (``gs_fields_region_morphology``; blocking, collective
        in a multi-process context)."""
        return region_morphology_fields(context, [self], region, [thresholds], [above])[0]

    def components(self, context: HipContext, thresholds, above: bool = True, connectivity: int = 8) -> List[Components]:
        """The connected components of this plane thresholded at each of ``thresholds`` (1..4) over the whole global grid,
        labelled on the device (``gs_fields_components``; blocking, collective in a multi-process context): a cell is set
        when it is above (``above``) or below the threshold; ``connectivity`` 4 or 8."""
        return components_fields(context, [self], [thresholds], [above], connectivity)[0]

    def region_components(self, context: HipContext, region, thresholds, above: bool = True,
                          connectivity: int = 8) -> List[RegionComponents]:
        """The connected components of every region of ``region`` = (rh, rw) cells (an int: square) of this plane thresholded
        at each of ``thresholds`` (1..4), a region's border being a wall, labelled on the device
        (``gs_fields_region_components``; blocking, collective in a multi-process context)."""
        return region_components_fields(context, [self], region, [thresholds], [above], connectivity)[0]

    def component_list(self, context: HipContext, threshold: float, above: bool = True, connectivity: int = 8,
                       min_size: int = 1) -> ComponentList:
        """One record per connected component of at least ``min_size`` cells of this plane thresholded at ``threshold`` over
        the whole global grid -- size, coordinate sums (the centroid), first cell, bounding box --, formed on the device
        (``gs_field_component_list``; blocking, single-process contexts)."""
        return component_list_field(context, self, threshold, above, connectivity, min_size)

    def match(self, context: HipContext, before: "HipConcentration", threshold: float, above: bool = True,
              connectivity: int = 8, min_size: int = 1) -> ComponentMatch:
        """What became of the components of ``before`` -- a plane of the same shape, an earlier state -- in this plane: both
        planes' component lists under one rule and the overlaps of their components, formed on the device
        (``gs_fields_match``; blocking, single-process contexts)."""
        return match_fields(context, before, self, threshold, above, connectivity, min_size)

    def correlation(self, context: HipContext, thresholds, max_lag: int = 32, above: bool = True) -> List[Correlation]:
        """The two-point pair counts of this plane thresholded at each of ``thresholds`` (1..4, one pass), lags 0 ..
        ``max_lag`` along four directions over the whole global grid, counted on the device (``gs_fields_correlation``;
        blocking, collective in a multi-process context)."""
        return correlation_fields(context, [self], [thresholds], [above], max_lag)[0]

    def spectrum(self, context: HipContext, tile: int = 64, window="hann") -> Spectrum:
        """The tile-averaged power spectrum of this plane over the whole global grid -- tiles of ``tile`` (16, 32, 64, 128)
        cells a side, ``window`` "hann" or "none" --, summed on the device (``gs_fields_spectrum``; blocking, collective in
        a multi-process context)."""
        return spectrum_fields(context, [self], tile, window)[0]

    def region_correlation(self, context: HipContext, region, thresholds, max_lag: int = 32,
                           above: bool = True) -> List[RegionCorrelation]:
        """The two-point pair counts of every region of ``region`` = (rh, rw) cells (an int: square) of this plane thresholded
        at each of ``thresholds`` (1..4, one pass), lags 0 .. ``max_lag``, a region's border being a wall for pairs, counted
        on the device (``gs_fields_region_correlation``; blocking, collective in a multi-process context)."""
        return region_correlation_fields(context, [self], region, [thresholds], [above], max_lag)[0]

    def region_histogram(self, context: HipContext, region, bins: int = 256,
                         range: Tuple[float, float] = (0.0, 1.0)) -> RegionHistogram:
        """How the values of every region of ``region`` = (rh, rw) cells (an int: square) of this plane are distributed over
        ``bins`` equal bins of ``range``, counted on the device (``gs_fields_region_histogram``; blocking, collective in a
        multi-process context)."""
        return region_histogram_fields(context, [self], region, bins, [range])[0]

    def region_spectrum(self, context: HipContext, region, tile: int = 64, window="hann") -> RegionSpectrum:
        """The tile-averaged power spectrum of every region of ``region`` = (rh, rw) cells (an int: square) of this plane --
        tiles of ``tile`` cells a side anchored at the region's first row and column --, summed on the device
        (``gs_fields_region_spectrum``; blocking, collective in a multi-process context)."""
        return region_spectrum_fields(context, [self], region, tile, window)[0]

    def change_from(self, context: HipContext, other: "HipConcentration") -> Change:
        """How far this plane is from ``other`` (this minus other, cell by cell in f64) over the whole global grid,
        computed on the device (``gs_fields_compare``; blocking, collective in a multi-process context)."""
        return compare_fields(context, [self], [other])[0]

    def region_change_from(self, context: HipContext, other: "HipConcentration", region) -> RegionChange:
        """How far every region of ``region`` = (rh, rw) cells (an int: square) of this plane is from the same region of
        ``other`` (this minus other), computed on the device (``gs_fields_region_compare``; blocking, collective in a
        multi-process context)."""
        return region_compare_fields(context, [self], [other], region)[0]

    def destroy(self) -> None:
        if self._h and self._ctx._h:
            self._ctx._lib.gs_field_destroy(self._ctx._h, self._h)
        self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Evolving:
    """Input/output pair of one species (mod.rs:140-187): slot 0 is the input."""

    def __init__(self, pair: List[HipConcentration]):
        self._pair = pair

    @classmethod
    def zeros_out(cls, context, shape):
        return cls([HipConcentration.default(context, shape), HipConcentration.zeros(context, shape)])

    @classmethod
    def ones_out(cls, context, shape):
        return cls([HipConcentration.default(context, shape), HipConcentration.ones(context, shape)])

    def in_out(self):
        return self._pair[0], self._pair[1]

    def out(self):
        return self._pair[1]

    def shape(self):
        return self._pair[0].shape()

    def raw_shape(self):
        return self._pair[0].raw_shape()

    def flip(self, context) -> None:
        self._pair[1].finalize(context)
        self._pair.reverse()


class Snapshot:
    """A state of a ``Species`` kept on the device: one U and one V plane of the snapshot's own, filled by a device copy
    (``gs_fields_copy``) of the species' current in-planes.  Made by ``Species.snapshot``; ``Species.change_since``
    compares with it, ``Species.restore`` goes back to it."""

    def __init__(self, species: "Species"):
        self._context = species.context()
        shape = species.shape()
        self.u = HipConcentration(self._context, shape)
        self.v = HipConcentration(self._context, shape)
        self.update(species)

    def update(self, species: "Species") -> None:
        """Take the species' current state (blocking: waits for the steps enqueued)."""
        in_u, in_v, _, _ = species.in_out()
        copy_fields(self._context, [self.u, self.v], [in_u, in_v])

    def close(self) -> None:
        self.u.destroy()
        self.v.destroy()


class TimeStats:
    """Per-cell statistics over the samples of a run, kept on the device (``gs_time_stats``, include/gs_hip.h): made by
    ``Species.time_stats`` or ``Ensemble.time_stats``, fed with ``accumulate(stamp)`` between ``perform_steps`` calls.
    ``groups`` names what is kept: ``"sum"`` (mean), ``"squares"`` (with ``"sum"``: variance), ``"extremes"`` (min, max),
    ``"crossings"`` (occupancy, arrival; needs a threshold).  For a Species the result planes are ``HipConcentration``s --
    every observable, reduced download and colour map applies to them --, for an ensemble numpy arrays of
    ``[count, rows, cols]``.  No standard deviation is formed on the device: take ``np.sqrt`` of the variance read."""

    GROUPS = {"sum": capi.GS_TSTAT_SUM, "squares": capi.GS_TSTAT_SQUARES, "extremes": capi.GS_TSTAT_EXTREMES,
              "crossings": capi.GS_TSTAT_CROSSINGS}
    RAW = {"sum": (capi.GS_TSTAT_RAW_SUM, np.float64), "squares": (capi.GS_TSTAT_RAW_SQUARES, np.float64),
           "min": (capi.GS_TSTAT_RAW_MIN, np.float32), "max": (capi.GS_TSTAT_RAW_MAX, np.float32),
           "set_count": (capi.GS_TSTAT_RAW_SET_COUNT, np.uint32), "first_stamp": (capi.GS_TSTAT_RAW_FIRST_STAMP, np.uint32)}
    NEVER = 0xFFFFFFFF     # first_stamp of a cell that was never set; no sample may carry it

    @classmethod
    def group_bits(cls, groups) -> int:
        """``groups`` as the C ABI takes them: an int, a name or a sequence of names."""
        if isinstance(groups, (int, np.integer)):
            return int(groups)
        names = [groups] if isinstance(groups, str) else list(groups)
        bits = 0
        for name in names:
            if name not in cls.GROUPS:
                raise ValueError(f"unknown group {name!r}: one of {sorted(cls.GROUPS)}")
            bits |= cls.GROUPS[name]
        return bits

    def __init__(self, context: "HipContext", source, groups, u_threshold=None, v_threshold=None, above=True,
                 first: int = 0, count: Optional[int] = None):
        self._ctx, self._source = context, source
        self._h = ctypes.c_void_p()
        self.groups = self.group_bits(groups)
        thresholds = above_arr = None
        if u_threshold is not None or v_threshold is not None:
            # (a species whose threshold is not given is never set: nothing is above +inf)
            t = [math.inf if x is None else float(x) for x in (u_threshold, v_threshold)]
            senses = [above, above] if isinstance(above, (bool, int)) else list(above)
            senses = [bool(senses[i]) if x is not None else True for i, x in enumerate((u_threshold, v_threshold))]
            thresholds, above_arr = (ctypes.c_float * 2)(*t), (ctypes.c_int32 * 2)(*[int(a) for a in senses])
        self._ensemble = isinstance(source, Ensemble)
        lib = context._lib
        if self._ensemble:
            self._first, self._count = source._range(first, count)
            self._shape = source.shape()
            capi.check(lib.gs_members_time_stats_create(context.handle, ctypes.byref(self._h), source.handle, self._first,
                                                        self._count, self.groups, thresholds, above_arr))
        else:
            self._shape = tuple(source.shape())
            capi.check(lib.gs_time_stats_create(context.handle, ctypes.byref(self._h), self._shape[0], self._shape[1], 2,
                                                self.groups, thresholds, above_arr))

    @property
    def handle(self):
        if not self._h or not self._ctx._h:    # (the context owns the memory: closing it frees what is left)
            raise GsError(capi.GS_ERR_INVALID, "time statistics already closed, or their context is")
        return self._h

    def accumulate(self, stamp: int) -> None:
        """One sample of the source's current state, stamped ``stamp`` (the step count, say; any u32 but 0xffffffff).
        Waits for the steps enqueued, enqueues one launch per slab and returns."""
        lib, ctx = self._ctx._lib, self._ctx
        if self._ensemble:
            capi.check(lib.gs_members_time_stats_accumulate(ctx.handle, self.handle, self._source.handle, int(stamp)))
        else:
            in_u, in_v, _, _ = self._source.in_out()
            capi.check(lib.gs_time_stats_accumulate(ctx.handle, self.handle, _handle_array([in_u, in_v]), 2, int(stamp)))

    @property
    def samples(self) -> int:
        n = ctypes.c_uint64()
        capi.check(self._ctx._lib.gs_time_stats_samples(self.handle, ctypes.byref(n)))
        return int(n.value)

    def reset(self) -> None:
        """Back to a fresh object: every accumulator at its reset value, no samples."""
        capi.check(self._ctx._lib.gs_time_stats_reset(self._ctx.handle, self.handle))

    @staticmethod
    def _plane(species: str) -> int:
        if species not in ("u", "v"):
            raise ValueError(f"species {species!r}: 'u' or 'v'")
        return 0 if species == "u" else 1

    def _result(self, species: str, which: int):
        plane, ctx = self._plane(species), self._ctx
        if self._ensemble:
            out = np.empty((self._count,) + tuple(self._shape), np.float32)
            capi.check(ctx._lib.gs_members_time_stats_result(ctx.handle, self.handle, plane, which,
                                                             out.ctypes.data_as(ctypes.c_void_p)))
            return out
        out = HipConcentration(ctx, self._shape)
        try:
            capi.check(ctx._lib.gs_time_stats_result(ctx.handle, self.handle, plane, which, out.handle))
        except GsError:
            out.destroy()
            raise
        return out

    def mean(self, species: str = "v"):
        """sum / n, rounded once in f64, as f32."""
        return self._result(species, capi.GS_TSTAT_MEAN)

    def variance(self, species: str = "v"):
        """max(squares / n - (sum / n)^2, 0) in f64, as f32 (a NaN stays NaN)."""
        return self._result(species, capi.GS_TSTAT_VARIANCE)

    def min(self, species: str = "v"):
        return self._result(species, capi.GS_TSTAT_MIN)

    def max(self, species: str = "v"):
        """The largest sample of every cell: the trail of a moving spot."""
        return self._result(species, capi.GS_TSTAT_MAX)

    def occupancy(self, species: str = "v"):
        """The share of the samples in which the cell was set (beyond its species' threshold)."""
        return self._result(species, capi.GS_TSTAT_OCCUPANCY)

    def arrival(self, species: str = "v"):
        """The stamp of the first sample in which the cell was set, as f32; -1 where it never was."""
        return self._result(species, capi.GS_TSTAT_ARRIVAL)

    def raw(self, name: str, species: str = "v") -> np.ndarray:
        """A raw accumulator -- ``sum``, ``squares`` (f64), ``min``, ``max`` (f32), ``set_count``, ``first_stamp`` (u32) -- of
        this process's rows as a dense array: ``[rows, cols]``, or ``[count, rows, cols]`` for an ensemble."""
        if name not in self.RAW:
            raise ValueError(f"unknown accumulator {name!r}: one of {sorted(self.RAW)}")
        raw, dtype = self.RAW[name]
        if self._ensemble:
            shape = (self._count,) + tuple(self._shape)
        else:
            r0, r1 = self._source.in_out()[0].local_rows()
            shape = (r1 - r0, self._shape[1])
        out = np.empty(shape, dtype)
        capi.check(self._ctx._lib.gs_time_stats_download(self._ctx.handle, self.handle, self._plane(species), raw,
                                                         out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def close(self) -> None:
        if self._h and self._ctx._h:
            self._ctx._lib.gs_time_stats_destroy(self._ctx._h, self._h)
        self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Species:
    """``Species<HipConcentration>``; ``Species.new`` = ``Species::new`` (mod.rs:36-59)."""

    def __init__(self, context: HipContext, u: Evolving, v: Evolving):
        self._context, self.u, self.v = context, u, v

    @classmethod
    def new(cls, context: HipContext, shape: Sequence[int], place_candidates: int = 0) -> "Species":
        """``Species::new`` (data/src/concentration/mod.rs:36-59).  ``place_candidates`` > 0 (not in the reference): the
        four planes are then placed by measurement with at most n extra blocks drawn (``Species.place``)."""
        shape = (int(shape[0]), int(shape[1]))
        u = Evolving.ones_out(context, shape)
        v = Evolving.zeros_out(context, shape)
        num_range, frac, row_shift = (7, 8), 16, 4
        sl = []
        for i in (0, 1):
            shift = row_shift if i == 0 else 0
            start, end = (max(shape[i] * num_range[j] // frac - shift, 0) for j in (0, 1))
            sl.append(range(start, end))
        u.out().fill_slice(context, sl, 0.0)
        v.out().fill_slice(context, sl, 1.0)
        s = cls(context, u, v)
        s.flip()
        s.placement, s.placement_drawn = None, 0
        if place_candidates > 0:
            s.place(place_candidates)
        return s

    def place(self, candidates: int) -> Tuple[float, float]:
        """Placement by measurement (``gs_fields_place``): planes of one physical region of HBM that a pass writes together
        are slow, so U's and V's planes are given blocks of different regions -- drawing at most ``candidates`` extra blocks,
        moving the planes that have to move with their contents.  Returns and remembers (``placement``) the mean time, in
        ms, of the probe pass (a step's traffic on a slot's two planes) over the blocks they had and the blocks they have now."""
        in_u, in_v, out_u, out_v = self.in_out()
        arr = (ctypes.c_void_p * 4)(in_u.handle, in_v.handle, out_u.handle, out_v.handle)
        first, best = ctypes.c_float(0), ctypes.c_float(0)
        ctx = self._context
        drawn0 = ctx.place_stats()[1]
        capi.check(ctx._lib.gs_fields_place(ctx.handle, arr, int(candidates), ctypes.byref(first), ctypes.byref(best)))
        self.placement = (float(first.value), float(best.value))
        self.placement_drawn = ctx.place_stats()[1] - drawn0      # extra blocks held for a moment by THIS call
        return self.placement

    def context(self) -> HipContext:
        return self._context

    def shape(self):
        return self.u.shape()

    def raw_shape(self):
        return self.u.raw_shape()

    def in_out(self):
        in_u, out_u = self.u.in_out()
        in_v, out_v = self.v.in_out()
        return in_u, in_v, out_u, out_v

    def flip(self) -> None:
        self.u.flip(self._context)
        self.v.flip(self._context)

    def summary(self) -> Tuple[Summary, Summary]:
        """(U, V) summaries of the current state in one call (``gs_fields_summarize``; blocking, collective in a
        multi-process context)."""
        in_u, in_v, _, _ = self.in_out()
        u, v = summarize_fields(self._context, [in_u, in_v])
        return u, v

    def histogram(self, bins: int = 256, u_range: Tuple[float, float] = (0.0, 1.0),
                  v_range: Tuple[float, float] = (0.0, 0.5)) -> Tuple[Histogram, Histogram]:
        """(U, V) histograms of the current state in one call (``gs_fields_histogram``; blocking, collective in a
        multi-process context): ``bins`` equal bins of ``u_range`` for U and of ``v_range`` for V."""
        in_u, in_v, _, _ = self.in_out()
        u, v = histogram_fields(self._context, [in_u, in_v], bins, [u_range, v_range])
        return u, v

    def _v_or_both(self, observe, u_thresholds, v_thresholds, above, *more):
        """``observe`` (one of the ``*_fields`` functions) of the current state as (U's list, V's list), ``above`` = (U's
        sense, V's sense): without ``u_thresholds`` only V is looked at and the U list is empty."""
        in_u, in_v, _, _ = self.in_out()
        if u_thresholds is None:
            return [], observe(self._context, [in_v], [v_thresholds], [above[1]], *more)[0]
        u, v = observe(self._context, [in_u, in_v], [u_thresholds, v_thresholds], list(above), *more)
        return u, v

    def morphology(self, v_thresholds=(0.25,), u_thresholds=None, v_above: bool = True,
                   u_above: bool = False) -> Tuple[List[Morphology], List[Morphology]]:
        """(U, V) bit-quad counts of the current state in one call (``gs_fields_morphology``; blocking, collective in a
        multi-process context): one ``Morphology`` per threshold (1..4 per species, the same number for both).  V carries
        the pattern where it is high and U where it is low, hence the default senses; without ``u_thresholds`` only V is
        looked at and the U list is empty."""
        return self._v_or_both(morphology_fields, u_thresholds, v_thresholds, (u_above, v_above))

    def region_summaries(self, region) -> Tuple[RegionSummaries, RegionSummaries]:
        """(U, V) summaries of every region of ``region`` = (rh, rw) cells (an int: square) of the current state in one call
        (``gs_fields_region_summaries``; blocking, collective in a multi-process context)."""
        in_u, in_v, _, _ = self.in_out()
        u, v = region_summaries_fields(self._context, [in_u, in_v], region)
        return u, v

    def region_morphology(self, region, v_thresholds=(0.25,), u_thresholds=None, v_above: bool = True,
                          u_above: bool = False) -> Tuple[List[RegionMorphology], List[RegionMorphology]]:
        """(U, V) bit-quad counts of every region of the current state in one call (``gs_fields_region_morphology``;
        blocking, collective in a multi-process context): one ``RegionMorphology`` per threshold, thresholds and senses as
        for ``morphology``; without ``u_thresholds`` only V is looked at and the U list is empty."""
        def observe(context, fields, thresholds, above):
            return region_morphology_fields(context, fields, region, thresholds, above)
        return self._v_or_both(observe, u_thresholds, v_thresholds, (u_above, v_above))

    def components(self, v_thresholds=(0.25,), u_thresholds=None,
                   connectivity: int = 8) -> Tuple[List[Components], List[Components]]:
        """(U, V) connected components of the current state in one call (``gs_fields_components``; blocking, collective in a
        multi-process context): one ``Components`` per threshold (1..4 per species, the same number for both).  V is set
        above its thresholds and U below, as ``morphology`` has it; without ``u_thresholds`` only V is looked at and the U
        list is empty."""
        return self._v_or_both(components_fields, u_thresholds, v_thresholds, (False, True), connectivity)

    def region_components(self, region, v_thresholds=(0.25,), u_thresholds=None, v_above: bool = True, u_above: bool = False,
                          connectivity: int = 8) -> Tuple[List[RegionComponents], List[RegionComponents]]:
        """(U, V) connected components of every region of the current state in one call (``gs_fields_region_components``;
        blocking, collective in a multi-process context): one ``RegionComponents`` per threshold, the region shape, thresholds
        and senses as for ``region_morphology``, ``connectivity`` 4 or 8; without ``u_thresholds`` only V is looked at and the
        U list is empty."""
        def observe(context, fields, thresholds, above):
            return region_components_fields(context, fields, region, thresholds, above, connectivity)
        return self._v_or_both(observe, u_thresholds, v_thresholds, (u_above, v_above))

    def component_list(self, threshold: float = 0.25, species: str = "v", above: bool = True, connectivity: int = 8,
                       min_size: int = 1) -> ComponentList:
        """Where the spots of the current state are: one record per connected component of at least ``min_size`` cells of
        ``species`` ("u" or "v") thresholded at ``threshold`` (``gs_field_component_list``; blocking, single-process
        contexts)."""
        in_u, in_v, _, _ = self.in_out()
        return component_list_field(self._context, _species_plane(species, in_u, in_v), threshold, above, connectivity, min_size)

    def match_since(self, snapshot: "Snapshot", threshold: float = 0.25, species: str = "v", above: bool = True,
                    connectivity: int = 8, min_size: int = 1) -> ComponentMatch:
        """What became of the spots since ``snapshot``: the component lists of ``species`` ("u" or "v") in the snapshot and
        in the current state, thresholded at ``threshold``, and the overlaps of their components (``gs_fields_match``;
        blocking, single-process contexts)."""
        in_u, in_v, _, _ = self.in_out()
        return match_fields(self._context, _species_plane(species, snapshot.u, snapshot.v), _species_plane(species, in_u, in_v),
                            threshold, above, connectivity, min_size)

    def correlation(self, v_thresholds=(0.25,), u_thresholds=None, max_lag: int = 32,
                    above: Tuple[bool, bool] = (False, True)) -> Tuple[List[Correlation], List[Correlation]]:
        """(U, V) two-point pair counts of the current state in one call (``gs_fields_correlation``; blocking, collective in
        a multi-process context): one ``Correlation`` per threshold (1..4 per species, the same number for both), lags 0 ..
        ``max_lag`` (1..64).  ``above`` = (U's sense, V's sense): V carries the pattern where it is high and U where it is
        low; without ``u_thresholds`` only V is looked at and the U list is empty."""
        return self._v_or_both(correlation_fields, u_thresholds, v_thresholds, above, max_lag)

    def spectrum(self, tile: int = 64, window="hann") -> Tuple[Spectrum, Spectrum]:
        """(U, V) tile-averaged power spectra of the current state in one call (``gs_fields_spectrum``; blocking, collective
        in a multi-process context): tiles of ``tile`` (16, 32, 64, 128) cells a side, ``window`` "hann" or "none"."""
        in_u, in_v, _, _ = self.in_out()
        u, v = spectrum_fields(self._context, [in_u, in_v], tile, window)
        return u, v

    def region_correlation(self, region, v_thresholds=(0.25,), u_thresholds=None, max_lag: int = 32,
                           above: Tuple[bool, bool] = (False, True)) -> Tuple[List[RegionCorrelation], List[RegionCorrelation]]:
        """(U, V) two-point pair counts of every region of the current state in one call (``gs_fields_region_correlation``;
        blocking, collective in a multi-process context): one ``RegionCorrelation`` per threshold, the region shape as for
        ``region_morphology``, thresholds, lags and senses as for ``correlation``; without ``u_thresholds`` only V is looked
        at and the U list is empty."""
        def observe(context, fields, thresholds, senses):
            return region_correlation_fields(context, fields, region, thresholds, senses, max_lag)
        return self._v_or_both(observe, u_thresholds, v_thresholds, above)

    def region_histogram(self, region, bins: int = 256, u_range: Tuple[float, float] = (0.0, 1.0),
                         v_range: Tuple[float, float] = (0.0, 1.0)) -> Tuple[RegionHistogram, RegionHistogram]:
        """(U, V) histograms of every region of the current state in one call (``gs_fields_region_histogram``; blocking,
        collective in a multi-process context): the region shape as for ``region_morphology``, ``bins`` equal bins of
        ``u_range`` for U and of ``v_range`` for V."""
        in_u, in_v, _, _ = self.in_out()
        u, v = region_histogram_fields(self._context, [in_u, in_v], region, bins, [u_range, v_range])
        return u, v

    def region_spectrum(self, region, tile: int = 64, window="hann") -> Tuple[RegionSpectrum, RegionSpectrum]:
        """(U, V) tile-averaged power spectra of every region of the current state in one call
        (``gs_fields_region_spectrum``; blocking, collective in a multi-process context): the region shape as for
        ``region_morphology``, tiles of ``tile`` cells a side anchored at every region's first row and column."""
        in_u, in_v, _, _ = self.in_out()
        u, v = region_spectrum_fields(self._context, [in_u, in_v], region, tile, window)
        return u, v

    def snapshot(self) -> Snapshot:
        """The current state copied into planes of its own on the device (``gs_fields_copy``; blocking)."""
        return Snapshot(self)

    def change_since(self, snapshot: Snapshot) -> Tuple[Change, Change]:
        """(U, V): how far the current state is from ``snapshot`` (current minus snapshot), in one call
        (``gs_fields_compare``; blocking, collective in a multi-process context)."""
        in_u, in_v, _, _ = self.in_out()
        u, v = compare_fields(self._context, [in_u, in_v], [snapshot.u, snapshot.v])
        return u, v

    def region_changes_since(self, snapshot: Snapshot, region) -> Tuple[RegionChange, RegionChange]:
        """(U, V): how far every region of the current state is from the same region of ``snapshot`` (current minus
        snapshot), in one call (``gs_fields_region_compare``; blocking, collective in a multi-process context): the region
        shape as for ``region_summaries``."""
        in_u, in_v, _, _ = self.in_out()
        u, v = region_compare_fields(self._context, [in_u, in_v], [snapshot.u, snapshot.v], region)
        return u, v

    def restore(self, snapshot: Snapshot) -> None:
        """Go back to ``snapshot``: its planes are copied into the current in-planes (``gs_fields_copy``; blocking), and
        the next ``perform_steps`` continues from the snapshot's bits."""
        in_u, in_v, _, _ = self.in_out()
        copy_fields(self._context, [in_u, in_v], [snapshot.u, snapshot.v])

    def time_stats(self, groups=("sum", "squares"), v_threshold=None, u_threshold=None, above=True) -> TimeStats:
        """Per-cell statistics over the samples of this species' run, kept on the device (``gs_time_stats``): call
        ``.accumulate(stamp)`` between ``perform_steps`` calls, read ``.mean("v")``, ``.variance("v")``, ``.max()``, ...
        ``groups``: names out of sum, squares, extremes, crossings; crossings need ``v_threshold`` or ``u_threshold``
        (``above``: set above the threshold, one sense or a (U, V) pair).  Works in every context, collective nowhere."""
        return TimeStats(self._context, self, groups, u_threshold=u_threshold, v_threshold=v_threshold, above=above)

    def access_result(self, f: Callable):
        return f(self.v._pair[0], self._context)

    def make_result_view(self, reduce: int = 1) -> np.ndarray:
        """The V plane (``reduce`` > 1: averaged over ``reduce`` x ``reduce`` blocks on the device, gs_hip.h)."""
        return self.access_result(lambda v, ctx: v.make_scalar_view(ctx, reduce))

    def write_result_view(self, target: np.ndarray, reduce: int = 1) -> None:
        self.access_result(lambda v, ctx: v.write_scalar_view(ctx, target, reduce))

    def write_result_view_after(self, target: np.ndarray, reduce: int = 1) -> None:
        """Asynchronous form used by the driver loop (simulate/src/main.rs:99-106)."""
        self.access_result(lambda v, ctx: v.write_scalar_view_after(ctx, target, reduce))


class Ensemble:
    """``members`` independent simulations of one shape on one context (``gs_ensemble``): each member has its own
    ``Parameters`` and its own U and V, the context's math and boundary options apply to all.  Member i evolves bit for
    bit as a lone ``Species`` with member i's parameters would.  The ensemble tracks its current slot itself (no flips).
    Made by ``Simulation.make_ensemble``."""

    def __init__(self, context: HipContext, members: int, shape: Sequence[int]):
        self._ctx = context
        self._h = ctypes.c_void_p()
        rows, cols = int(shape[0]), int(shape[1])
        capi.check(context._lib.gs_ensemble_create(context.handle, ctypes.byref(self._h), int(members), rows, cols))
        self.members, self._shape = int(members), (rows, cols)

    @property
    def handle(self):
        if not self._h:
            raise GsError(capi.GS_ERR_INVALID, "ensemble already destroyed")
        return self._h

    def shape(self) -> Tuple[int, int]:
        return self._shape

    def set_params(self, params) -> None:
        """One ``Parameters`` for every member, or a sequence of one per member."""
        plist = [params] if isinstance(params, Parameters) else list(params)
        arr = (capi.GsParams * len(plist))(*[p.to_c() for p in plist])
        capi.check(self._ctx._lib.gs_ensemble_set_params(self._ctx.handle, self.handle, arr, len(plist)))

    def seed(self) -> None:
        """``Species::new``'s pattern in every member."""
        capi.check(self._ctx._lib.gs_ensemble_seed(self._ctx.handle, self.handle))

    def _range(self, first: int, count: Optional[int]) -> Tuple[int, int]:
        count = self.members - first if count is None else int(count)
        return int(first), count

    def upload(self, u: Optional[np.ndarray], v: Optional[np.ndarray], first: int = 0) -> None:
        """Overwrite members ``[first, first + len)`` from dense float32 ``[count, rows, cols]`` arrays (either may be
        None: that species stays as it is)."""
        arrays = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (u, v)]
        given = [a for a in arrays if a is not None]
        if not given:
            raise ValueError("upload needs u or v")
        count = given[0].shape[0]
        for a in given:
            if a.shape != (count,) + self._shape:
                raise AssertionError(f"upload shape {a.shape} != {(count,) + self._shape}")
        ptr = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in arrays]
        capi.check(self._ctx._lib.gs_ensemble_upload(self._ctx.handle, self.handle, int(first), count, ptr[0], ptr[1]))

    def _download(self, species: int, first: int, count: Optional[int]) -> np.ndarray:
        first, count = self._range(first, count)
        out = np.empty((count,) + self._shape, np.float32)
        capi.check(self._ctx._lib.gs_ensemble_download(self._ctx.handle, self.handle, first, count, species,
                                                       out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def result_views(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """V of members ``[first, first + count)`` as ``[count, rows, cols]`` (blocking)."""
        return self._download(1, first, count)

    def u_views(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """U of members ``[first, first + count)`` as ``[count, rows, cols]`` (blocking)."""
        return self._download(0, first, count)

    def summaries(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Summaries of members ``[first, first + count)`` computed on the device (``gs_members_summarize``, blocking):
        a structured array of ``SUMMARY_DTYPE`` with shape ``(count, 2)``, column 0 = U, 1 = V -- bit for bit what
        ``Species.summary`` gives for a lone Species in the member's state."""
        first, count = self._range(first, count)
        out = np.zeros((max(count, 0), 2), SUMMARY_DTYPE)
        capi.check(self._ctx._lib.gs_members_summarize(self._ctx.handle, self.handle, first, count,
                                                        out.ctypes.data_as(ctypes.POINTER(capi.GsSummary))))
        return out

    def histograms(self, first: int = 0, count: Optional[int] = None, bins: int = 256,
                   u_range: Tuple[float, float] = (0.0, 1.0), v_range: Tuple[float, float] = (0.0, 0.5)) -> np.ndarray:
        """Histograms of members ``[first, first + count)`` counted on the device (``gs_members_histogram``, blocking): a
        ``uint64`` array ``[count, 2, bins + 3]`` -- axis 1: U over ``u_range``, V over ``v_range``; last axis: the
        ``bins`` counts, then below, above, nan -- what ``Species.histogram`` gives for a lone Species in the member's
        state (``Histogram.from_counters`` makes the object)."""
        first, count = self._range(first, count)
        bins = int(bins)
        lo, hi = _f32_pairs([u_range, v_range])
        out = np.zeros((max(count, 0), 2, max(bins, 0) + 3), np.uint64)
        capi.check(self._ctx._lib.gs_members_histogram(self._ctx.handle, self.handle, first, count, lo, hi, bins,
                                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out

    def morphologies(self, first: int = 0, count: Optional[int] = None, v_thresholds=(0.25,), u_thresholds=(0.5,),
                     v_above: bool = True, u_above: bool = False) -> np.ndarray:
        """Bit-quad counts of members ``[first, first + count)`` counted on the device (``gs_members_morphology``, blocking):
        a ``uint64`` array ``[count, 2, nt, 6]`` -- axis 1: U at ``u_thresholds`` with the sense ``u_above``, V at
        ``v_thresholds`` with ``v_above`` (1..4 thresholds, the same number for both); last axis: Q0, Q1, Q2, Q3, Q4, QD -- what
        ``Species.morphology`` gives for a lone Species in the member's state.  ``quad_measures`` turns it into areas,
        perimeters and Euler numbers, ``Morphology.from_quads`` one entry into the object."""
        first, count = self._range(first, count)
        nt, thr, sense = _member_thresholds(u_thresholds, v_thresholds, (u_above, v_above))
        out = np.zeros((max(count, 0), 2, max(nt, 1), 6), np.uint64)
        capi.check(self._ctx._lib.gs_members_morphology(self._ctx.handle, self.handle, first, count, thr, sense, nt,
                                                         out.ctypes.data_as(ctypes.POINTER(capi.GsMorphology))))
        return out

    def components(self, first: int = 0, count: Optional[int] = None, v_thresholds=(0.25,), u_thresholds=(0.5,),
                   connectivity: int = 8) -> np.ndarray:
        """Connected components of members ``[first, first + count)`` labelled on the device (``gs_members_components``,
        blocking): a ``uint64`` array ``[count, 2, nt, 35]`` -- axis 1: U below ``u_thresholds``, V above ``v_thresholds``
        (1..4 thresholds, the same number for both); last axis: components, set_cells, largest, by_size[32] -- what
        ``Species.components`` gives for a lone Species in the member's state.  ``Components.from_counters`` turns one entry
        into the object."""
        first, count = self._range(first, count)
        nt, thr, sense = _member_thresholds(u_thresholds, v_thresholds, (False, True))
        out = np.zeros((max(count, 0), 2, max(nt, 1), 35), np.uint64)
        capi.check(self._ctx._lib.gs_members_components(self._ctx.handle, self.handle, first, count, thr, sense, nt,
                                                         int(connectivity), out.ctypes.data_as(ctypes.POINTER(capi.GsComponents))))
        return out

    def component_lists(self, first: int = 0, count: Optional[int] = None, species: str = "v", threshold: float = 0.25,
                        above: bool = True, connectivity: int = 8, min_size: int = 1) -> List[ComponentList]:
        """Component lists of members ``[first, first + count)`` formed on the device (``gs_members_component_list``,
        blocking): one ``ComponentList`` per member -- what ``Species.component_list`` gives for a lone Species in the
        member's state; rows are the member's own."""
        first, count = self._range(first, count)
        h = ctypes.c_void_p()
        capi.check(self._ctx._lib.gs_members_component_list(self._ctx.handle, self.handle, first, count,
                                                            _species_plane(species, 0, 1), float(threshold), 1 if above else 0,
                                                            int(connectivity), int(min_size), ctypes.byref(h)))
        return _component_lists(self._ctx._lib, h, self._shape, threshold, above, connectivity, min_size)

    def matches_since(self, ref: "Ensemble", first: int = 0, count: Optional[int] = None, species: str = "v",
                      threshold: float = 0.25, above: bool = True, connectivity: int = 8,
                      min_size: int = 1) -> List[ComponentMatch]:
        """What became of the spots of members ``[first, first + count)`` since the same members of ``ref`` -- a
        ``snapshot()``, say -- (``gs_members_match``, blocking): one ``ComponentMatch`` per member, ``ref``'s member the
        ``before`` and this ensemble's the ``after`` -- what ``Species.match_since`` gives for lone Species in the members'
        states."""
        first, count = self._range(first, count)
        h = ctypes.c_void_p()
        capi.check(self._ctx._lib.gs_members_match(self._ctx.handle, ref.handle, self.handle, first, count,
                                                   _species_plane(species, 0, 1), float(threshold), 1 if above else 0,
                                                   int(connectivity), int(min_size), ctypes.byref(h)))
        return _component_matches(self._ctx._lib, h, self._shape, threshold, above, connectivity, min_size)

    def correlations(self, first: int = 0, count: Optional[int] = None, v_thresholds=(0.25,), u_thresholds=(0.5,),
                     max_lag: int = 32, above: Tuple[bool, bool] = (False, True)) -> np.ndarray:
        """Two-point pair counts of members ``[first, first + count)`` counted on the device (``gs_members_correlation``,
        blocking): a ``uint64`` array ``[count, 2, nt, 4, max_lag + 1]`` -- axis 1: U at ``u_thresholds`` with the sense
        ``above[0]``, V at ``v_thresholds`` with ``above[1]`` (1..4 thresholds, the same number for both); axis 3: the unit
        steps of ``CORRELATION_STEPS``; last axis: the lag -- what ``Species.correlation`` gives for a lone Species in the
        member's state.  ``Correlation.from_pairs`` turns one ``[4, max_lag + 1]`` entry into the object."""
        first, count = self._range(first, count)
        nt, thr, sense = _member_thresholds(u_thresholds, v_thresholds, above)
        lags = max_lag + 1 if 1 <= max_lag <= 64 else 1
        out = np.zeros((max(count, 0), 2, max(nt, 1), 4, lags), np.uint64)
        capi.check(self._ctx._lib.gs_members_correlation(self._ctx.handle, self.handle, first, count, thr, sense, nt, max_lag,
                                                          out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out

    def spectra(self, first: int = 0, count: Optional[int] = None, tile: int = 64, window="hann") -> Tuple[np.ndarray, np.ndarray]:
        """Tile-averaged power spectra of members ``[first, first + count)`` summed on the device (``gs_members_spectrum``,
        blocking): (``power``, ``tiles``) -- the raw f64 sums ``[count, 2, tile, tile / 2 + 1]`` and the ``uint64`` tile
        counts ``[count, 2, 2]`` = {used, skipped}; axis 1: U, V -- bit for bit what ``Species.spectrum`` gives for a lone
        Species in the member's state.  ``Spectrum.from_raw(power[m, s], tile, window, tiles[m, s])`` makes the object."""
        first, count = self._range(first, count)
        tile, win = int(tile), _spectrum_window(window)
        power, tiles = _spectrum_outputs(2 * max(count, 0), tile)
        capi.check(self._ctx._lib.gs_members_spectrum(self._ctx.handle, self.handle, first, count, tile, win,
                                                       power.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                       tiles.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return power.reshape((max(count, 0), 2) + power.shape[1:]), tiles.reshape(max(count, 0), 2, 2)

    def snapshot(self) -> "Ensemble":
        """An ensemble of the same shape and member count on the same context whose members hold this one's current states
        (``gs_members_copy``; blocking): what ``changes_since`` compares with and ``copy_from`` brings back.  It carries
        the context's parameters, not this ensemble's: it is a store of states, not something to advance.  All its members
        are active and their step counts start at 0, whatever this ensemble's are."""
        snap = Ensemble(self._ctx, self.members, self._shape)
        snap.copy_from(self)
        return snap

    def copy_from(self, src: "Ensemble", first: int = 0, count: Optional[int] = None) -> None:
        """Members ``[first, first + count)`` of ``src``'s current state into the same members of this ensemble
        (``gs_members_copy``, device to device, blocking); the other members stay as they are."""
        first, count = self._range(first, count)
        capi.check(self._ctx._lib.gs_members_copy(self._ctx.handle, self.handle, src.handle, first, count))

    def changes_since(self, ref: "Ensemble", first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """How far members ``[first, first + count)`` are from the same members of ``ref`` (``gs_members_compare``,
        blocking): a structured array of ``CHANGE_DTYPE`` with shape ``(count, 2)``, column 0 = U, 1 = V -- bit for bit
        what ``Species.change_since`` gives for lone Species in the members' states."""
        first, count = self._range(first, count)
        out = np.zeros((max(count, 0), 2), CHANGE_DTYPE)
        capi.check(self._ctx._lib.gs_members_compare(self._ctx.handle, self.handle, ref.handle, first, count,
                                                     out.ctypes.data_as(ctypes.POINTER(capi.GsChange))))
        return out

    def time_stats(self, groups=("sum", "squares"), v_threshold=None, u_threshold=None, above=True, first: int = 0,
                   count: Optional[int] = None) -> TimeStats:
        """Per-cell statistics over the samples of members ``[first, first + count)``, kept on the device
        (``gs_members_time_stats_create``; ``Species.time_stats`` for the arguments).  Members are sampled whether active
        or retired -- a retired member repeats its state --, and every member's planes are bit for bit those of a lone
        Species sampled in the same states.  The result methods return ``[count, rows, cols]`` numpy arrays."""
        return TimeStats(self._ctx, self, groups, u_threshold=u_threshold, v_threshold=v_threshold, above=above, first=first,
                         count=count)

    BUNDLE_RESULTS = {"mean": capi.GS_TSTAT_MEAN, "variance": capi.GS_TSTAT_VARIANCE, "min": capi.GS_TSTAT_MIN,
                      "max": capi.GS_TSTAT_MAX, "occupancy": capi.GS_TSTAT_OCCUPANCY}

    def bundle_stats(self, span: int, which=("mean", "variance"), v_threshold=None, u_threshold=None, above=True,
                     first: int = 0, count: Optional[int] = None, out: Optional[dict] = None, out_first: int = 0) -> dict:
        """Per-cell statistics ACROSS members, formed on the device in one pass (``gs_members_bundle_stats``, blocking): every
        run of ``span`` consecutive members of ``[first, first + count)`` is a bundle -- the realisations of one parameter
        point, say -- and result ``name`` of bundle ``b`` becomes member ``out_first + b`` of the ensemble ``out[name]``, U
        from the members' U and V from their V.  ``which`` names the results: ``"mean"``, ``"variance"``, ``"min"``,
        ``"max"``, ``"occupancy"`` (the share of the members in which the cell is beyond its species' threshold; a species
        without a threshold is never set).  The accumulators and formulas are those of ``TimeStats`` with member ``j`` in
        the place of sample ``j``: a bundle's planes are bit for bit the time statistics of a lone Species sampled through
        the members' states.  Members are read whether active or retired.  Without ``out`` the result ensembles are made
        here with ``count / span`` members; like ``snapshot()`` they carry the context's parameters.  Returns ``{name:
        Ensemble}``: every ensemble observable applies to a mean field or a probability map without a download."""
        names = [which] if isinstance(which, str) else list(which)
        for name in names:
            if name not in self.BUNDLE_RESULTS:
                raise ValueError(f"unknown result {name!r}: one of {sorted(self.BUNDLE_RESULTS)}")
        first, count = self._range(first, count)
        span = int(span)
        thresholds = above_arr = None
        if u_threshold is not None or v_threshold is not None:
            # (a species whose threshold is not given is never set: nothing is above +inf)
            t = [math.inf if x is None else float(x) for x in (u_threshold, v_threshold)]
            senses = [above, above] if isinstance(above, (bool, int)) else list(above)
            senses = [bool(senses[i]) if x is not None else True for i, x in enumerate((u_threshold, v_threshold))]
            thresholds, above_arr = (ctypes.c_float * 2)(*t), (ctypes.c_int32 * 2)(*[int(a) for a in senses])
        made = []
        if out is None:
            bundles = count // span if span > 0 else 0
            out = {}
            for name in names:
                if name not in out:
                    out[name] = Ensemble(self._ctx, max(int(out_first) + bundles, 1), self._shape)
                    made.append(out[name])
        codes = (ctypes.c_int32 * max(len(names), 1))(*[self.BUNDLE_RESULTS[name] for name in names])
        targets = (ctypes.c_void_p * max(len(names), 1))(*[out[name].handle.value for name in names])
        try:
            capi.check(self._ctx._lib.gs_members_bundle_stats(self._ctx.handle, self.handle, first, count, span, codes, len(names),
                                                              thresholds, above_arr, targets, int(out_first)))
        except GsError:
            for e in made:
                e.destroy()
            raise
        return {name: out[name] for name in names}

    def set_active(self, mask, first: int = 0) -> None:
        """Active flags of members ``[first, first + len(mask))`` from a bool or uint8 array (``gs_members_set_active``;
        blocking): ``prepare_steps`` advances the active members only, an inactive member keeps its state -- every reader
        (``result_views``, ``summaries``, ...) sees it -- and its step count.  The other members keep their flags."""
        m = np.asarray(mask)
        if m.dtype != np.bool_ and m.dtype != np.uint8:
            raise TypeError(f"an active mask is a bool or uint8 array, not {m.dtype}")
        first = int(first)
        if m.ndim != 1 or m.size == 0 or first < 0 or first + m.size > self.members:
            raise ValueError(f"an active mask of shape {m.shape} at member {first} of {self.members}")
        flags = np.ascontiguousarray(m != 0, np.uint8)
        capi.check(self._ctx._lib.gs_members_set_active(self._ctx.handle, self.handle, first, flags.size,
                                                         flags.ctypes.data_as(ctypes.c_void_p)))

    def _flag(self, indices, value: bool) -> None:
        idx = np.unique(np.asarray(indices, np.int64).ravel())
        if idx.size == 0:
            return
        if idx[0] < 0 or idx[-1] >= self.members:
            raise IndexError(f"member {int(idx[0] if idx[0] < 0 else idx[-1])} of {self.members}")
        lo, hi = int(idx[0]), int(idx[-1]) + 1
        mask = self.active(lo, hi - lo)
        mask[idx - lo] = value
        self.set_active(mask, lo)

    def retire(self, indices) -> None:
        """The members ``indices`` stop advancing (``set_active`` with the others' flags as they are)."""
        self._flag(indices, False)

    def reactivate(self, indices) -> None:
        """The members ``indices`` advance again, each from the state it holds."""
        self._flag(indices, True)

    def _get_active(self, first: int, count: Optional[int], flags: bool, steps: bool):
        first, count = self._range(first, count)
        a = np.zeros(max(count, 0), np.uint8) if flags else None
        t = np.zeros(max(count, 0), np.uint64) if steps else None
        total = ctypes.c_uint64()
        capi.check(self._ctx._lib.gs_members_get_active(
            self._ctx.handle, self.handle, first, count, None if a is None else a.ctypes.data_as(ctypes.c_void_p),
            None if t is None else t.ctypes.data_as(ctypes.c_void_p), ctypes.byref(total)))
        return a, t, total.value

    def active(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The active flags of members ``[first, first + count)`` as a bool array."""
        return self._get_active(first, count, True, False)[0].astype(np.bool_)

    def steps_taken(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """The steps each of members ``[first, first + count)`` has been advanced by since the ensemble was made (int64):
        a retired member's count stands still."""
        return self._get_active(first, count, False, True)[1].astype(np.int64)

    def active_count(self) -> int:
        """How many members of the whole ensemble are active."""
        return int(self._get_active(0, 1, False, False)[2])

    def set_noise(self, sigma_u, sigma_v=0.0, seed=0, step=0, first: int = 0, count: Optional[int] = None) -> None:
        """Noise of members ``[first, first + count)`` (``gs_members_set_noise``; blocking): scalars or per-member arrays,
        broadcast against each other.  From now on every step of such a member adds ``sigma * xi`` to each species, drawn
        with the member's own ``seed`` at the member's own step index, which starts at ``step`` and advances with the steps
        that member takes -- member i is bit for bit a lone Species with ``Simulation.set_noise`` of the same values.  The
        first call attaches noise to the ensemble (members never named: sigmas 0, seed 0, step 0); the context's own noise
        never touches an ensemble."""
        first, count = self._range(first, count)
        n = np.zeros(max(count, 0), NOISE_DTYPE)
        n["sigma_u"], n["sigma_v"] = sigma_u, sigma_v
        for name, value in (("seed", seed), ("step", step)):  # any Python or numpy integers, taken modulo 2^64
            words = np.broadcast_to(np.asarray(value, dtype=object), n.shape)
            n[name] = np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in words], np.uint64)
        capi.check(self._ctx._lib.gs_members_set_noise(self._ctx.handle, self.handle, first, count,
                                                        n.ctypes.data_as(ctypes.c_void_p), n.size))

    def noise(self, first: int = 0, count: Optional[int] = None) -> Optional[np.ndarray]:
        """The noise of members ``[first, first + count)`` as a structured array (``NOISE_DTYPE``: sigma_u, sigma_v, seed and
        step -- the member's NEXT step index; a retired member's stands still), or ``None`` when the ensemble has none.
        Saved with a snapshot of the members, the records continue a run exactly."""
        first, count = self._range(first, count)
        n = np.zeros(max(count, 0), NOISE_DTYPE)
        attached = ctypes.c_int32(0)
        capi.check(self._ctx._lib.gs_members_get_noise(self._ctx.handle, self.handle, first, count,
                                                        n.ctypes.data_as(ctypes.c_void_p), ctypes.byref(attached)))
        return n if attached.value else None

    def clear_noise(self) -> None:
        """Detach the ensemble's noise: the next run launches the kernels of an ensemble without noise."""
        capi.check(self._ctx._lib.gs_members_clear_noise(self._ctx.handle, self.handle))

    def prepare_steps(self, steps: int) -> None:
        """Enqueue ``steps`` steps of every active member and return (``gs_ensemble_run``); ``context.sync()`` waits."""
        capi.check(self._ctx._lib.gs_ensemble_run(self._ctx.handle, self.handle, int(steps)))

    def perform_steps(self, steps: int) -> None:
        """``steps`` steps of every active member, done on return."""
        self.prepare_steps(steps)
        self._ctx.sync()

    def destroy(self) -> None:
        if self._h and self._ctx._h:
            self._ctx._lib.gs_ensemble_destroy(self._ctx._h, self._h)
        self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Simulation:
    """The backend: ``SimulateBase + SimulateCreate + Simulate``."""

    CliArgs = HipArgs
    Concentration = HipConcentration
    Error = GsError

    def __init__(self, params: Parameters, args: Optional[HipArgs] = None):
        self.params = params
        self.context = HipContext(params, args)

    @classmethod
    def new(cls, params: Parameters, args: Optional[HipArgs] = None) -> "Simulation":
        """``SimulateCreate::new(params, args)`` (compute/shared/src/lib.rs:42-45)."""
        return cls(params, args)

    def make_species(self, shape: Sequence[int], place_candidates: Optional[int] = None) -> Species:
        """``SimulateBase::make_species`` (lib.rs:33-34).  ``place_candidates``: None = the library's default -- a Species
        of >= 2^26 cells per process on a context with one slab per process is placed by measurement with at most
        ``HipArgs.place_candidates`` extra blocks (``--hip-place-candidates`` / GS_HIP_PLACE_CANDIDATES, default 12; 0 = never)
        --, 0 = no placement, n > 0 = placed whatever its size."""
        if place_candidates is None:
            args = self.context.args
            cells = int(shape[0]) * int(shape[1]) // max(1, args.world)
            place_candidates = args.place_candidates if len(args.devices) == 1 and cells >= PLACE_MIN_CELLS else 0
        return Species.new(self.context, shape, place_candidates)

    def make_ensemble(self, shape: Sequence[int], params, seed: bool = True, members: Optional[int] = None) -> Ensemble:
        """An ``Ensemble`` of grids of ``shape``: ``params`` is a sequence of ``Parameters``, one per member, or one
        ``Parameters`` for all ``members`` (default 1).  ``seed``: ``Species::new``'s pattern in every member, else zeros."""
        plist = [params] if isinstance(params, Parameters) else list(params)
        if not plist:
            raise ValueError("an ensemble needs at least one member")
        n = len(plist) if len(plist) > 1 or members is None else int(members)
        if members is not None and n != int(members):
            raise ValueError(f"{len(plist)} parameter sets for {members} members")
        e = Ensemble(self.context, n, shape)
        e.set_params(plist)
        if seed:
            e.seed()
        return e

    def perform_steps(self, species: Species, steps: int) -> None:
        """``Simulate::perform_steps`` (lib.rs:48-58): ``steps`` steps; on return they are DONE and
        the input slots of ``species`` hold the final state.  Synchronous like every backend of the
        reference -- its GPU backends end ``perform_steps_impl`` with
        ``.then_signal_fence_and_flush()?.wait(None)?`` (compute/shared/src/gpu/mod.rs:77-91)."""
        self.prepare_steps(species, steps)
        self.context.sync()

    def prepare_steps(self, species: Species, steps: int) -> None:
        """The asynchronous form, ``SimulateGpu::prepare_steps`` (compute/shared/src/gpu/mod.rs:
        70-75): enqueue ``steps`` steps and return; whatever is enqueued next on this context (more
        steps, ``write_result_view_after``) runs behind them, a download or ``context.sync()`` waits.
        HIP streams order the work, so there is no future object to pass along."""
        in_u, in_v, out_u, out_v = species.in_out()
        slot = ctypes.c_int32(0)
        lib = self.context._lib
        capi.check(lib.gs_run(self.context.handle, in_u.handle, in_v.handle, out_u.handle,
                              out_v.handle, int(steps), ctypes.byref(slot)))
        if slot.value == 1:  # odd number of steps: the newest state sits in the output slot
            species.u._pair.reverse()
            species.v._pair.reverse()

    def set_param_map(self, feed, kill, shape: Optional[Sequence[int]] = None) -> None:
        """Attach a parameter map (``gs_ctx_set_param_map``): from now on every step takes feed = ``feed[r, c]`` and
        kill = ``kill[r, c]`` at cell (r, c) instead of ``params.feed`` / ``params.kill``.  ``feed`` and ``kill`` are
        global ``[rows, cols]`` arrays or scalars (a scalar is a uniform plane; ``shape`` is needed when both are);
        each process uploads only its own rows.  The library copies them (F + K is formed on the device in the
        context's float mode), so the arrays may change afterwards; a new call replaces the map.  Collective in a
        multi-process run.  The species stepped while it is attached must have its shape."""
        if shape is None:
            arrays = [np.shape(x) for x in (feed, kill) if np.ndim(x) != 0]
            if not arrays:
                raise ValueError("a parameter map of two scalars needs its shape")
            shape = arrays[0]
        rows, cols = int(shape[0]), int(shape[1])
        planes = []
        try:
            for value in (feed, kill):
                c = HipConcentration(self.context, (rows, cols))
                planes.append(c)
                r0, r1 = c.local_rows()
                if np.ndim(value) == 0:
                    capi.check(self.context._lib.gs_field_fill(self.context.handle, c.handle, float(value)))
                else:
                    a = np.asarray(value, np.float32)
                    if a.shape != (rows, cols):
                        raise ValueError(f"parameter map of shape {a.shape}, species of {(rows, cols)}")
                    c.upload(self.context, a[r0:r1])
            capi.check(self.context._lib.gs_ctx_set_param_map(self.context.handle, planes[0].handle, planes[1].handle))
        finally:
            for c in planes:
                c.destroy()

    def clear_param_map(self) -> None:
        """Detach the parameter map: the steps take ``params.feed`` / ``params.kill`` again."""
        capi.check(self.context._lib.gs_ctx_set_param_map(self.context.handle, None, None))

    def set_mask(self, mask, shape: Optional[Sequence[int]] = None) -> None:
        """Attach a domain mask (``gs_ctx_set_mask``): from now on the cells where ``mask`` is nonzero (NaN included) are
        walls -- they keep their values, and a tap of a fluid cell that reads a wall reads the cell's own value instead.
        ``mask`` is a global ``[rows, cols]`` array of any dtype, or a scalar (a uniform plane; ``shape`` is then needed);
        each process uploads only its own rows.  The library copies it, so the array may change afterwards; a new call
        replaces the mask.  Collective in a multi-process run.  The species stepped while it is attached must have its
        shape."""
        if np.ndim(mask) == 0:
            if shape is None:
                raise ValueError("a scalar mask needs its shape")
            rows, cols = int(shape[0]), int(shape[1])
            walls = np.full((rows, cols), 1.0 if mask != 0 else 0.0, np.float32)
        else:
            walls = (np.asarray(mask) != 0).astype(np.float32)
            if walls.ndim != 2 or (shape is not None and walls.shape != (int(shape[0]), int(shape[1]))):
                raise ValueError(f"mask of shape {walls.shape}, species of {tuple(shape) if shape is not None else '?'}")
            rows, cols = walls.shape
        c = HipConcentration(self.context, (rows, cols))
        try:
            r0, r1 = c.local_rows()
            c.upload(self.context, np.ascontiguousarray(walls[r0:r1]))
            capi.check(self.context._lib.gs_ctx_set_mask(self.context.handle, c.handle))
        finally:
            c.destroy()

    def clear_mask(self) -> None:
        """Detach the domain mask: every cell is fluid again."""
        capi.check(self.context._lib.gs_ctx_set_mask(self.context.handle, None))

    def set_noise(self, sigma_u: float, sigma_v: float = 0.0, seed: int = 0, step: int = 0) -> None:
        """Attach a noise term (``gs_ctx_set_noise``): from now on every step adds ``sigma * xi`` to each species, ``xi``
        uniform on [-1, 1) (variance 1/3) and a pure function of (``seed``, step index, global row, global column), so a
        run is bit-reproducible whatever kernel, fusion depth, slab or process count computes it.  ``step`` is the index
        of the next step; it advances with every step enqueued on this context (``noise()`` reports it).  A species whose
        sigma is 0 is not touched.  Collective in a multi-process run (every process passes the same values)."""
        n = capi.GsNoise(float(sigma_u), float(sigma_v), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF)
        capi.check(self.context._lib.gs_ctx_set_noise(self.context.handle, ctypes.byref(n)))

    def clear_noise(self) -> None:
        """Detach the noise term: every step is the deterministic reference step again."""
        capi.check(self.context._lib.gs_ctx_set_noise(self.context.handle, None))

    def noise(self) -> Optional[dict]:
        """The noise term in force as ``{"sigma_u", "sigma_v", "seed", "step"}`` -- ``step``: the index of the next step --
        or ``None`` when none is attached.  Saved with a snapshot, it continues the run exactly (``set_noise(**saved)``)."""
        n = capi.GsNoise()
        attached = ctypes.c_int32(0)
        capi.check(self.context._lib.gs_ctx_get_noise(self.context.handle, ctypes.byref(n), ctypes.byref(attached)))
        if not attached.value:
            return None
        return {"sigma_u": float(n.sigma_u), "sigma_v": float(n.sigma_v), "seed": int(n.seed), "step": int(n.step)}

    def perform_step(self, species: Species) -> None:
        """One ``gs_step`` then ``species.flip()`` -- the ``SimulateStep`` form (cpu.rs:21-42)."""
        in_u, in_v, out_u, out_v = species.in_out()
        capi.check(self.context._lib.gs_step(self.context.handle, in_u.handle, in_v.handle,
                                             out_u.handle, out_v.handle))
        species.flip()
