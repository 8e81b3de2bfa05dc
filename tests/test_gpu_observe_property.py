"""Randomised parity of the on-device observables that threshold or bin a plane -- morphology, two-point correlations,
connected components, component lists, histograms -- against their restatements in tests/ (morph_ref.quads, corr_ref.pairs,
components_ref.counters, component_list_ref.records, hist_ref.histogram), bit for bit: all results are integers.

`cases()` draws

* the shape, each side from the seams of the kernels' units and their neighbours (labelling tiles, quad and pair units,
  words and strips of columns: tests/observe_cases.py), at most CELL_CAP cells in all of a case's planes;
* the pattern (observe_cases.KINDS: planted planes at five densities, the adversarial shapes of components_ref, full and
  empty planes, one set and one unset cell, set lines with gaps on every seam, rows of runs that begin and end in every
  column of a lane) and the values that carry it: set and unset cells on either side of the threshold, and NaN, +-inf, +-0,
  sub-normals and cells equal to the threshold and its f32 neighbours on top;
* thresholds (1 .. 4 distinct ones, +-inf, the largest finite value, a sub-normal and both zeros among them), the sense, the
  connectivity, the largest lag, min_size, the bins and the range (one range ends at a cell's value);
* the call: HipConcentration.<observable> on one field, the *_fields call with 1 .. 4 fields with thresholds and senses of
  their own, or the ensemble's call with a range of members;
* for fields, a chain of 1 .. 5 slabs on one device (one-row slabs occur) and `poison`: the ghost rows of every slab and the
  pitch padding of every row hold values that are set by the widest margin, written through a device view of the field's
  own allocation; for ensembles, members outside the range are set in every cell, `fence` sets the first and last row of
  the members inside it too, and half of the cases retire some members and advance the others by an odd number of steps.

Beyond parity: set cells, area and the pairs at lag 0 agree; a list taken with min_size 1 gives the components' 35 words;
by_size sums to the count; nt thresholds in one call equal nt calls; several slabs equal one; a member equals a lone field
with its plane; a retired member holds the plane it was given; an empty plane counts nothing whatever the poison.  A chain
with a slab shorter than the largest lag must refuse the correlation (GS_ERR_UNSUPPORTED); the case then runs with the lag
the shortest slab allows.  tests/test_observe_property_cpu.py checks without a GPU that the strategy draws legal cases of
every kind, that the new layouts are what they claim, and that the pinned examples would notice each single fault of a
kernel or of the host's seam merge."""
import collections
import os
import time

import numpy as np
import pytest
from hypothesis import HealthCheck, example, given, settings, strategies as st

from grayscott_amd import GsError, HipArgs, HipConcentration, Parameters, Simulation, capi
from grayscott_amd.simulation import (components_fields, correlation_fields, histogram_fields, morphology_fields)

from . import component_list_ref, components_ref, corr_ref, hist_ref, morph_ref
from . import observe_cases as O

pytestmark = pytest.mark.gpu

FAMILIES = ["morphology", "correlation", "components", "component_list", "histogram"]
FORMS = ["field", "fields", "ensemble"]
INF = float("inf")
THRESHOLDS = [0.3, -1.5, 0.0, -0.0, 2.0 ** -130, INF, -INF, 3.4028235e38]
MAX_LAGS = [1, 2, 31, 32, 33, 63, 64]
MIN_SIZES = ["1", "2", "5", "largest", "largest + 1"]
BINS = [1, 2, 255, 256, 1000, 4096]
RANGES = [(0.0, 1.0), (-1.5, 0.3), "a cell's value"]
CELL_CAP, MEMBER_CAP = 530_000, 40_000
GHOST_ROWS = 4                         # above and below every slab (include/gs_hip.h, "Domain decomposition")

ROWS = sorted(set(range(1, 6)) | {m * O.TILE_ROWS + d for m in (1, 2, 3) for d in (-1, 0, 1)}
              | {m * O.QUAD_ROWS + d for m in (1, 2) for d in (-1, 0, 1, 2)})
PAIR_UNIT_ROWS = sorted(m * O.PAIR_ROWS + d for m in (1, 2) for d in (-1, 0, 1))    # correlation draws only
COLS = sorted(set(range(1, 9)) | {m * O.WORD_COLS + d for m in (1, 2) for d in (-1, 0, 1)}
              | {m * O.STRIP_COLS + d for m in (1, 2, 4) for d in range(-3, 4)})
ENSEMBLE_SHAPES = [(13, 21), (37, 53), (45, 61)]

# What ran, for the report of a run (printed when the module is done; shown with pytest -s or -rP)
SEEN = collections.Counter()


def ragged(shape):
    """Does an ensemble of this shape take the load path that is not 16 bytes wide (gs_plane_scan.h: a member's rows lie
    `cols` floats apart, its planes rows * cols)?"""
    return shape[1] % 4 != 0 or shape[0] * shape[1] % 4 != 0


def shortest_slab(rows, slabs):
    return min((i + 1) * rows // slabs - i * rows // slabs for i in range(slabs))


def distinct(thresholds, n):
    """The first n of `thresholds` that differ as f32 values (+0 and -0 do not)."""
    out = []
    for t in thresholds:
        if all(np.float32(t) != np.float32(x) for x in out):
            out.append(t)
    return out[:n]


def pinned_case(family, **kw):
    """A case of `cases` with every field at its plainest value but those given (the @example cases)."""
    base = dict(family=family, form="field", rows=33, cols=259, seed=1, kind="planted", density=0.5, at=None,
                thresholds=[0.3], above=True, conn=8, max_lag=32, min_size=0, bins=256, range=0, slabs=1, poison=False,
                nfields=1, members=1, first=0, count=1, fence=False, retire=False, retired=[False] * 6, steps=1)
    base.update(kw)
    return base


@st.composite
def cases(draw, family=None):
    family = family or draw(st.sampled_from(FAMILIES))
    form = draw(st.sampled_from(FORMS))
    seed = draw(st.integers(0, 2 ** 16))
    all_rows = ROWS + (PAIR_UNIT_ROWS if family == "correlation" else [])
    if form == "ensemble":
        want_ragged = draw(st.booleans())
        if want_ragged and draw(st.integers(0, 3)) == 0:
            rows, cols = draw(st.sampled_from(ENSEMBLE_SHAPES))
        else:
            rows = draw(st.sampled_from(all_rows))
            cols = draw(st.sampled_from([c for c in COLS if rows * c <= MEMBER_CAP and ragged((rows, c)) == want_ragged]))
        cap = MEMBER_CAP
    else:
        rows = draw(st.sampled_from(all_rows))
        cols = draw(st.sampled_from([c for c in COLS if rows * c <= CELL_CAP]))
        cap = CELL_CAP
    cells = rows * cols
    # (planes and thresholds multiply the references' time: a case's planes hold CELL_CAP cells in all, its thresholds see
    # twice that)
    nfields = draw(st.integers(1, max(1, min(4, cap // cells)))) if form == "fields" else 1
    nt = draw(st.integers(1, max(1, min(4, 2 * cap // (cells * nfields)))))
    thresholds = distinct(draw(st.permutations(THRESHOLDS)), 1 if family == "component_list" else nt)
    max_lag = draw(st.sampled_from(MAX_LAGS))
    slabs = min(draw(st.integers(1, 5)), rows)
    if family == "correlation" and form != "ensemble" and slabs > 1 and shortest_slab(rows, slabs) < max_lag:
        # a chain that must refuse this lag: kept as it is one time in four, else given a lag it can do
        if draw(st.integers(0, 3)) != 0:
            fit = [lag for lag in MAX_LAGS if lag <= shortest_slab(rows, slabs)]
            max_lag = draw(st.sampled_from(fit)) if fit else max_lag
            slabs = slabs if fit else 1
    members = draw(st.integers(1, 6))
    first = draw(st.integers(0, members - 1))
    return dict(family=family, form=form, rows=rows, cols=cols, seed=seed, kind=draw(st.sampled_from(O.KINDS)),
                density=draw(st.sampled_from(O.DENSITIES)), at=draw(st.sampled_from([None, None] + O.PLACES)),
                thresholds=thresholds, above=draw(st.booleans()), conn=draw(st.sampled_from([4, 8])), max_lag=max_lag,
                min_size=draw(st.integers(0, len(MIN_SIZES) - 1)), bins=draw(st.sampled_from(BINS)),
                range=draw(st.integers(0, len(RANGES) - 1)), slabs=slabs, poison=draw(st.booleans()), nfields=nfields,
                members=members, first=first, count=draw(st.integers(1, members - first)), fence=draw(st.booleans()),
                retire=draw(st.booleans()), retired=[draw(st.booleans()) for _ in range(6)], steps=draw(st.sampled_from([1, 3, 5])))


def legal(c):
    """What a drawn case runs with: (slabs, the largest lag after the refusal, is the drawn lag refused).  Also the
    strategy's own check (tests/test_observe_property_cpu.py draws cases on the CPU)."""
    rows, cols, form = c["rows"], c["cols"], c["form"]
    assert c["family"] in FAMILIES and form in FORMS and c["kind"] in O.KINDS and c["density"] in O.DENSITIES
    if (rows, cols) not in ENSEMBLE_SHAPES:
        assert (rows in ROWS or (rows in PAIR_UNIT_ROWS and c["family"] == "correlation")) and cols in COLS
    nt = len(c["thresholds"])
    assert 1 <= nt <= 4 and len({np.float32(t).tobytes() for t in c["thresholds"]}) == nt
    assert len(distinct(c["thresholds"], 4)) == nt and all(t in THRESHOLDS for t in c["thresholds"])
    assert c["conn"] in (4, 8) and c["max_lag"] in MAX_LAGS and c["bins"] in BINS and 0 <= c["min_size"] < len(MIN_SIZES)
    assert 1 <= c["slabs"] <= min(5, rows) and 1 <= c["nfields"] <= 4 and (form == "fields" or c["nfields"] == 1)
    assert 1 <= c["members"] <= 6 and 0 <= c["first"] and c["count"] >= 1 and c["first"] + c["count"] <= c["members"]
    assert c["steps"] % 2 == 1
    if form == "ensemble":
        assert rows * cols <= MEMBER_CAP
        return 1, c["max_lag"], False
    assert rows * cols * c["nfields"] <= CELL_CAP
    short = shortest_slab(rows, c["slabs"])
    if c["family"] == "correlation" and c["slabs"] > 1 and short < c["max_lag"]:
        return (c["slabs"], short, True) if short > 0 else (1, c["max_lag"], True)
    return c["slabs"], c["max_lag"], False


def plane_rules(c, i):
    """(thresholds, sense) of plane i of a case: field i of a field list, or species i of an ensemble's members.  Every
    plane has its own: the thresholds rotated, the sense alternating -- but the ensemble's components, whose senses the
    call fixes (U below, V above)."""
    k = i % len(c["thresholds"])
    thresholds = c["thresholds"][k:] + c["thresholds"][:k]
    if c["form"] == "ensemble":
        if c["family"] == "components":
            return thresholds, i == 1
        return thresholds, c["above"] == (i == 1)
    return thresholds, c["above"] == (i % 2 == 0)


def hist_range(c, plane):
    """The (lo, hi) a case's histogram runs over; RANGES' last: hi is the value of a cell of `plane`."""
    r = RANGES[c["range"]]
    if isinstance(r, tuple):
        return r
    lo = -2.0
    with np.errstate(invalid="ignore"):
        inside = plane[(plane > np.float32(lo + 1e-3)) & (plane < np.float32(1e30))]
    return (lo, float(inside.max())) if inside.size else (lo, 1.0)


def make_plane(c, seed, t, above):
    shape = (c["rows"], c["cols"])
    if c["family"] == "histogram" and c["kind"] == "planted":
        lo, hi = RANGES[c["range"]] if isinstance(RANGES[c["range"]], tuple) else (-2.0, 1.0)
        return hist_ref.planted(shape, lo, hi, c["bins"], seed)
    return O.plane(c["kind"], shape, t, above, seed, c["density"], c["at"], c["slabs"])


def field_planes(c):
    """[(plane, thresholds, sense)] of a field case, all drawn from its seed."""
    out = []
    for i in range(c["nfields"]):
        thresholds, above = plane_rules(c, i)
        out.append((make_plane(c, c["seed"] + i, thresholds[0], above), thresholds, above))
    return out


def member_planes(c):
    """(U, V) of an ensemble case as [members, rows, cols] arrays: the members of the range carry the case's pattern -- with
    `fence`, their first and last rows set in every cell --, the members outside it are set in every cell."""
    shape = (c["rows"], c["cols"])
    planes = np.empty((2, c["members"]) + shape, np.float32)
    for s in (0, 1):
        thresholds, above = plane_rules(c, s)
        for m in range(c["members"]):
            if c["first"] <= m < c["first"] + c["count"]:
                planes[s, m] = make_plane(c, c["seed"] + 2 * m + s, thresholds[0], above)
                if c["fence"]:
                    planes[s, m, 0] = planes[s, m, -1] = O.poison_value(above)
            else:
                planes[s, m] = O.poison_value(above)
    return planes[0], planes[1]


def min_size_of(c, plane, t, above):
    full = component_list_ref.records(plane, t, above, c["conn"])
    largest = int(full["size"].max()) if full.shape[0] else 0
    return [1, 2, 5, max(largest, 1), largest + 1][c["min_size"]]


def reference(c, plane, t, above, max_lag, min_size=1, span=None):
    family = c["family"]
    if family == "morphology":
        return morph_ref.quads(plane, t, above)
    if family == "correlation":
        return corr_ref.pairs(plane, t, above, max_lag)
    if family == "components":
        return components_ref.counters(plane, t, above, c["conn"])
    if family == "component_list":
        return component_list_ref.records(plane, t, above, c["conn"], min_size)
    return hist_ref.histogram(plane, span[0], span[1], c["bins"])


# ---- pinned examples ------------------------------------------------------------------------------------------------------
_T, _Q, _P, _S = O.TILE_ROWS, O.QUAD_ROWS, O.PAIR_ROWS, O.STRIP_COLS
_THRESHOLDED = ["morphology", "correlation", "components", "component_list"]
# The cases that must always run, per family (a family's test takes its own):
# - an empty plane under poison in chains of 2 and 3 slabs: every counter 0;
# - set lines with gaps on every seam, and rows of lane runs, over two strips (and a column more) and more than two tiles and
#   quad units, poisoned, in chains of 1, 3 and 5 slabs, both connectivities, both senses;
# - the adversarial shapes across tile and slab seams; one-row slabs (5 rows, 5 slabs); one set cell at a corner;
# - special values around a sub-normal threshold and around -0, four thresholds in one call, four fields in one call;
# - correlation: more than one pair unit, lags 63 and 64 across the strips' edges, a chain that must refuse its lag;
# - ensembles on the ragged path (the three shapes the issue names) and on the 16-byte one, ranges inside the ensemble,
#   fenced, with and without retired members;
# - histograms: every bin count, a range that ends at a cell's value, planted edges, a ragged last block of columns.
EDGE_EXAMPLES = (
    [pinned_case(f, kind="empty", slabs=s, poison=True, rows=2 * _T + 1, cols=_S + 3, conn=n)
     for f in _THRESHOLDED for s, n in ((2, 8), (3, 4))]
    + [pinned_case(f, kind=k, slabs=s, poison=True, rows=r, cols=2 * _S + 1, conn=n, above=a, seed=7 + s, min_size=ms)
       for f in _THRESHOLDED for k in ("seams", "lane_runs")
       for s, n, a, r, ms in ((1, 8, True, 2 * _Q + 1, 0), (3, 4, False, 2 * _Q + 2, 1), (5, 8, True, 3 * _T - 1, 3))]
    + [pinned_case(f, kind=k, slabs=s, rows=r, cols=w, conn=n, poison=True, thresholds=[0.3, -1.5], min_size=ms, form=form,
                   nfields=2 if form == "fields" else 1)
       for f in _THRESHOLDED
       for k, s, r, w, n, ms, form in (("serpentine", 3, 2 * _T + 1, _S + 1, 4, 3, "field"), ("comb", 2, _T + 1, _S + 2, 4, 0, "fields"),
                                       ("rings", 4, 2 * _T, 2 * _S - 1, 8, 2, "field"), ("checkerboard", 5, 5, _S + 3, 8, 0, "fields"),
                                       ("staircase", 3, _Q + 2, _S + 3, 8, 4, "field"), ("u_shape", 2, _T + 1, _S + 1, 4, 1, "field"),
                                       ("column", 5, 5, 7, 4, 3, "field"))]
    + [pinned_case(f, kind="one-set", at=at, rows=_T + 1, cols=_S + 1, slabs=2, poison=True) for f in _THRESHOLDED for at in ("nw", "se")]
    + [pinned_case(f, kind="planted", density=d, thresholds=t, above=a, rows=_Q + 1, cols=_S + 1, form=form, nfields=nf, slabs=s,
                   poison=True, seed=11)
       for f in _THRESHOLDED
       for d, t, a, form, nf, s in ((0.593, [2.0 ** -130, 0.0, 0.3, -1.5], True, "field", 1, 1),
                                    (0.3, [-0.0, 3.4028235e38, INF, -1.5], False, "fields", 4, 2))]
    + [pinned_case("correlation", kind=k, rows=r, cols=w, max_lag=lag, slabs=s, poison=True, above=a, seed=lag)
       for k, r, w, lag, s, a in (("seams", _P + 1, _S + 3, 64, 1, True), ("planted", _P + 1, 2 * _S + 1, 63, 2, False),
                                  ("seams", 2 * _Q + 1, 2 * _S + 2, 64, 3, True), ("lane_runs", 2 * _Q + 2, _S + 1, 33, 2, True),
                                  ("checkerboard", 5, _S + 1, 1, 5, True), ("lane_runs", _P + 1, 7, 31, 1, False),
                                  ("planted", 5, 2 * _S + 1, 64, 1, True), ("lane_runs", _Q + 2, _S + 3, 64, 1, False))]
    + [pinned_case(f, form="ensemble", rows=r, cols=w, kind=k, members=m, first=a, count=n, fence=fence, retire=ret,
                   retired=[False, True, True, False, True, False], steps=3, thresholds=t, seed=r, conn=cn, max_lag=lag, min_size=ms)
       for f in FAMILIES
       for r, w, k, m, a, n, fence, ret, t, cn, lag, ms in (
           (13, 21, "planted", 4, 1, 2, True, False, [0.3, -1.5], 8, 31, 0), (37, 53, "seams", 3, 0, 3, False, True, [0.3], 4, 33, 1),
           (45, 61, "lane_runs", 6, 2, 3, True, True, [0.0, 0.3, 2.0 ** -130], 8, 64, 3),
           (_T + 1, _S, "seams", 3, 1, 1, False, False, [0.3, -1.5], 4, 32, 2), (3, _S + 1, "lane_runs", 2, 1, 1, True, False, [0.3], 8, 2, 0))]
    + [pinned_case("histogram", kind=k, bins=b, range=g, rows=r, cols=w, slabs=s, poison=True, form=form, nfields=nf, seed=b)
       for k, b, g, r, w, s, form, nf in (("planted", 1, 0, 5, _S + 3, 5, "field", 1), ("planted", 2, 1, _T + 1, _S - 1, 2, "fields", 3),
                                          ("planted", 255, 2, _Q, 2 * _S + 1, 3, "field", 1), ("seams", 256, 2, _Q + 1, _S + 1, 2, "field", 1),
                                          ("planted", 1000, 0, 3, 4 * _S + 3, 1, "fields", 2), ("lane_runs", 4096, 2, 2 * _T + 1, 7, 4, "field", 1),
                                          ("planted", 4096, 1, _Q + 1, 2 * _S + 3, 2, "field", 1), ("planted", 1000, 1, 3 * _T, _S + 2, 3, "fields", 2))])


def _with_examples(family):
    def decorate(test):
        for ex in reversed([e for e in EDGE_EXAMPLES if e["family"] == family]):
            test = example(case=ex)(test)
        return test
    return decorate


def counts_of(c):
    """What the run report counts an example under."""
    slabs, _, detour = legal(c)
    out = ["examples", c["family"], "form " + c["form"]]
    if c["form"] == "ensemble":
        out.append("ensemble load path " + ("ragged" if ragged((c["rows"], c["cols"])) else "16 bytes"))
        out += ["retired members"] if c["retire"] else []
    else:
        out.append(f"slabs {slabs}")
        out += ["poisoned"] if c["poison"] else []
        out += ["one-row slabs"] if shortest_slab(c["rows"], slabs) == 1 and slabs > 1 else []
        out += ["refused lags"] if detour else []
    return out


# ---- on the device ----------------------------------------------------------------------------------------------------------
def words(x):
    """A result object as the integers that the reference returns."""
    if hasattr(x, "quads"):
        return x.quads
    if hasattr(x, "pairs"):
        return x.pairs
    if hasattr(x, "by_size"):
        return np.concatenate([np.array([x.count, x.set_cells, x.largest], np.uint64), x.by_size])
    if hasattr(x, "records"):
        return x.records
    return np.concatenate([x.counts, np.array([x.below, x.above, x.nan], np.uint64)])


def observe_fields(ctx, c, fields, rules, max_lag, min_sizes=None, spans=None, one_by_one=False):
    """[field][threshold] results of the case's observable: one call per field (`one_by_one`: HipConcentration's methods)
    or the *_fields call over all of them; lists and the single-field histogram have no other form than the former."""
    family = c["family"]
    thresholds, above = [r[0] for r in rules], [r[1] for r in rules]
    if family == "component_list":
        return [[words(f.component_list(ctx, t[0], a, c["conn"], m))] for f, t, a, m in zip(fields, thresholds, above, min_sizes)]
    if family == "histogram":
        if one_by_one:
            return [[words(f.histogram(ctx, c["bins"], s))] for f, s in zip(fields, spans)]
        return [[words(h)] for h in histogram_fields(ctx, fields, c["bins"], spans)]
    if one_by_one:
        out = []
        for f, t, a in zip(fields, thresholds, above):
            got = {"morphology": lambda: f.morphology(ctx, t, a), "correlation": lambda: f.correlation(ctx, t, max_lag, a),
                   "components": lambda: f.components(ctx, t, a, c["conn"])}[family]()
            out.append([words(x) for x in got])
        return out
    got = {"morphology": lambda: morphology_fields(ctx, fields, thresholds, above),
           "correlation": lambda: correlation_fields(ctx, fields, thresholds, above, max_lag),
           "components": lambda: components_fields(ctx, fields, thresholds, above, c["conn"])}[family]()
    return [[words(x) for x in per_field] for per_field in got]


def poison(field, value):
    """`value` into the ghost rows above and below every slab of `field` and into the pitch padding of all its rows, through
    a device view over rows [-GHOST_ROWS, rows + GHOST_ROWS) and all `pitch` columns of each slab -- the extent raw_shape()
    reports, so every write lies inside the field's own allocation."""
    import torch

    class _DeviceArray:
        def __init__(self, address, rows, pitch):
            self.__cuda_array_interface__ = {"shape": (rows, pitch), "typestr": "<f4", "data": (address, False), "version": 3,
                                             "strides": (pitch * 4, 4)}

    raw_rows, pitch = field.raw_shape()
    slabs = field.device_slabs()
    cols = field.shape()[1]
    assert sum(rows + 2 * GHOST_ROWS for _, _, _, rows, _ in slabs) == raw_rows and all(p == pitch for _, p, _, _, _ in slabs)
    assert pitch >= cols and all(address for address, _, _, _, _ in slabs)
    for address, _, _, rows, device in slabs:
        view = torch.as_tensor(_DeviceArray(address - GHOST_ROWS * pitch * 4, rows + 2 * GHOST_ROWS, pitch), device=f"cuda:{device}")
        assert tuple(view.shape) == (rows + 2 * GHOST_ROWS, pitch)
        view[:GHOST_ROWS] = float(value)
        view[GHOST_ROWS + rows:] = float(value)
        view[:, cols:] = float(value)
    torch.cuda.synchronize()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def counts_nothing(family, got):
    if family == "morphology":
        return not got[1:].any()
    return got.shape[0] == 0 if family == "component_list" else not got.any()


def check_area(ctx, field, thresholds, above, conn, what):
    """components.set_cells == morphology.area == pairs[k][0] for all four k, and by_size sums to the count (all on the
    device; the slab chain is long enough for lag 1)."""
    morph, comp = field.morphology(ctx, thresholds, above), field.components(ctx, thresholds, above, conn)
    corr = field.correlation(ctx, thresholds, 1, above)
    for m, n, p in zip(morph, comp, corr):
        assert n.set_cells == m.area and all(int(p.pairs[k][0]) == m.area for k in range(4)), what
        assert int(n.by_size.sum()) == n.count and (n.count == 0) == (n.set_cells == 0) and n.largest <= n.set_cells, what


def run_field_case(c):
    slabs, max_lag, detour = legal(c)
    family, shape = c["family"], (c["rows"], c["cols"])
    planes = field_planes(c)
    rules = [(t, a) for _, t, a in planes]
    spans = [hist_range(c, p) for p, _, _ in planes]
    min_sizes = [min_size_of(c, p, t[0], a) if family == "component_list" else 1 for p, t, a in planes]
    what = (f"{family} {c['form']} {shape} kind={c['kind']} density={c['density']} at={c['at']} seed={c['seed']} rules={rules} "
            f"conn={c['conn']} max_lag={max_lag} (drawn {c['max_lag']}) min_size={min_sizes} bins={c['bins']} ranges={spans} "
            f"slabs={slabs} (drawn {c['slabs']}) poison={c['poison']}")
    want = [[reference(c, p, t, a, max_lag, m, s) for t in (ts[:1] if family in ("component_list", "histogram") else ts)]
            for (p, ts, a), m, s in zip(planes, min_sizes, spans)]

    def fields_on(sim):
        out = []
        for p, _, a in planes:
            f = HipConcentration(sim.context, shape)
            f.upload(sim.context, p)
            if c["poison"]:
                poison(f, O.poison_value(a))
            out.append(f)
        sim.context.sync()
        return out

    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * c["slabs"]))
    try:
        ctx = sim.context
        fields = fields_on(sim)
        if detour:
            with pytest.raises(GsError) as e:
                observe_fields(ctx, dict(c, family="correlation"), fields, rules, c["max_lag"])
            assert e.value.code == capi.GS_ERR_UNSUPPORTED, what
            if slabs != c["slabs"]:
                ctx.close()
                sim = Simulation.new(Parameters(), HipArgs(devices=[0] * slabs))
                ctx = sim.context
                fields = fields_on(sim)
        got = observe_fields(ctx, c, fields, rules, max_lag, min_sizes, spans, one_by_one=c["form"] == "field")
        for i, (g, w) in enumerate(zip(got, want)):
            assert len(g) == len(w), what
            for k, (x, y) in enumerate(zip(g, w)):
                assert same(x, y), f"field {i} threshold {k}: {x[:8]} ..., not {y[:8]} ...: {what}"
                if c["kind"] == "empty" and family != "histogram" and k == 0:    # (the plane is made for its first threshold)
                    assert counts_nothing(family, x), f"an empty plane: {what}"
        if c["poison"]:                                      # the poison is where it belongs: the cells are the plane's
            assert same(fields[0].make_scalar_view(ctx), planes[0][0]), what
        if family != "histogram":
            check_area(ctx, fields[0], rules[0][0], rules[0][1], c["conn"], what)
        if family == "component_list":
            listed = fields[0].component_list(ctx, rules[0][0][0], rules[0][1], c["conn"], 1)
            counted = fields[0].components(ctx, rules[0][0][:1], rules[0][1], c["conn"])[0]
            assert same(component_list_ref.counters(listed.records), words(counted)), what
        if len(rules[0][0]) > 1 and family not in ("component_list", "histogram"):
            for k, t in enumerate(rules[0][0]):              # nt thresholds in one call: nt calls with one
                alone = observe_fields(ctx, c, fields[:1], [([t], rules[0][1])], max_lag, one_by_one=True)[0][0]
                assert same(alone, got[0][k]), f"threshold {k} alone: {what}"
    finally:
        sim.context.close()
    if slabs > 1:                                            # several slabs: one
        sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
        try:
            field = HipConcentration(sim.context, shape)
            field.upload(sim.context, planes[0][0])
            one = observe_fields(sim.context, c, [field], rules[:1], max_lag, min_sizes[:1], spans[:1], one_by_one=True)[0]
            assert all(same(x, y) for x, y in zip(one, got[0])), f"one slab: {what}"
        finally:
            sim.context.close()


def observe_members(ens, c, rules, max_lag, min_sizes, spans):
    """[member of the range][species][threshold] results of the ensemble's call."""
    family, first, count = c["family"], c["first"], c["count"]
    (tu, au), (tv, av) = rules
    if family == "component_list":
        per = [ens.component_lists(first, count, "uv"[s], rules[s][0][0], rules[s][1], c["conn"], min_sizes[s]) for s in (0, 1)]
        return [[[per[s][m].records] for s in (0, 1)] for m in range(count)]
    if family == "histogram":
        out = ens.histograms(first, count, c["bins"], spans[0], spans[1])
        return [[[out[m, s]] for s in (0, 1)] for m in range(count)]
    if family == "morphology":
        out = ens.morphologies(first, count, tv, tu, av, au)
    elif family == "correlation":
        out = ens.correlations(first, count, tv, tu, max_lag, (au, av))
    else:
        assert (au, av) == (False, True)
        out = ens.components(first, count, tv, tu, c["conn"])
    return [[[out[m, s, k] for k in range(out.shape[2])] for s in (0, 1)] for m in range(count)]


def run_ensemble_case(c):
    _, max_lag, _ = legal(c)
    family, shape, first, count = c["family"], (c["rows"], c["cols"]), c["first"], c["count"]
    u, v = member_planes(c)
    rules = [plane_rules(c, 0), plane_rules(c, 1)]
    retired = [m for m in range(c["members"]) if c["retired"][m]] if c["retire"] else []
    what = (f"{family} ensemble of {c['members']} x {shape}, members [{first}, {first + count}) kind={c['kind']} "
            f"density={c['density']} at={c['at']} seed={c['seed']} rules={rules} conn={c['conn']} max_lag={max_lag} bins={c['bins']} "
            f"fence={c['fence']} retired={retired} steps={c['steps'] if c['retire'] else 0}")
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    lone = Simulation.new(Parameters(), HipArgs(devices=[0]))
    try:
        ens = sim.make_ensemble(shape, Parameters(), seed=False, members=c["members"])
        ens.upload(u, v)
        if c["retire"]:
            ens.retire(retired)
            ens.perform_steps(c["steps"])
            now_u, now_v = ens.u_views(), ens.result_views()
            for m in retired:                                # a retired member holds the planes it was given
                assert same(now_u[m], u[m]) and same(now_v[m], v[m]), f"member {m}: {what}"
            u, v = now_u, now_v
        held = (u, v)
        spans = [hist_range(c, held[s][first]) for s in (0, 1)]
        min_sizes = [min_size_of(c, held[s][first], rules[s][0][0], rules[s][1]) if family == "component_list" else 1 for s in (0, 1)]
        got = observe_members(ens, c, rules, max_lag, min_sizes, spans)
        field = HipConcentration(lone.context, shape)
        for m in range(count):
            for s in (0, 1):
                plane, (thresholds, above) = held[s][first + m], rules[s]
                few = thresholds[:1] if family in ("component_list", "histogram") else thresholds
                assert len(got[m][s]) == len(few), what
                field.upload(lone.context, plane)
                alone = observe_fields(lone.context, c, [field], [rules[s]], max_lag, [min_sizes[s]], [spans[s]], one_by_one=True)[0]
                for k, t in enumerate(few):
                    want = reference(c, plane, t, above, max_lag, min_sizes[s], spans[s])
                    x = np.ascontiguousarray(got[m][s][k])
                    assert same(x, want), f"member {first + m} {'UV'[s]} threshold {k}: {x[:8]} ..., not {want[:8]} ...: {what}"
                    assert same(alone[k], x), f"member {first + m} {'UV'[s]} threshold {k} as a lone field: {what}"
                if family != "histogram" and m == 0:
                    check_area(lone.context, field, thresholds, above, c["conn"], what)
        ens.destroy()
    finally:
        sim.context.close()
        lone.context.close()


def run_case(case, family):
    c = dict(case)
    assert c["family"] == family
    started = time.perf_counter()
    if c["form"] == "ensemble":
        run_ensemble_case(c)
    else:
        run_field_case(c)
    SEEN.update(counts_of(c))
    pinned = case in EDGE_EXAMPLES
    SEEN.update({"pinned examples": 1} if pinned else {})
    took = time.perf_counter() - started
    SEEN["seconds in pinned examples" if pinned else "seconds in drawn examples"] += took
    SEEN["slowest example, seconds"] = max(SEEN["slowest example, seconds"], took)


@pytest.fixture(scope="module", autouse=True)
def report():
    SEEN.clear()
    yield
    print("\nobserve property examples: " + ", ".join(f"{k}: {v:.4g}" for k, v in sorted(SEEN.items())))


# The default keeps the file within the run time of tests/test_gpu_mask_property.py: the pinned examples
# take most of it, a drawn one about 0.01 s
EXAMPLES = int(os.environ.get("GS_PROPERTY_EXAMPLES_OBSERVE", "4"))
_SETTINGS = dict(max_examples=EXAMPLES, deadline=None, suppress_health_check=list(HealthCheck))


@settings(**_SETTINGS)
@given(cases("morphology"))
@_with_examples("morphology")
def test_any_morphology_matches_the_reference(built, case):
    run_case(case, "morphology")


@settings(**_SETTINGS)
@given(cases("correlation"))
@_with_examples("correlation")
def test_any_correlation_matches_the_reference(built, case):
    run_case(case, "correlation")


@settings(**_SETTINGS)
@given(cases("components"))
@_with_examples("components")
def test_any_components_match_the_reference(built, case):
    run_case(case, "components")


@settings(**_SETTINGS)
@given(cases("component_list"))
@_with_examples("component_list")
def test_any_component_list_matches_the_reference(built, case):
    run_case(case, "component_list")


@settings(**_SETTINGS)
@given(cases("histogram"))
@_with_examples("histogram")
def test_any_histogram_matches_the_reference(built, case):
    run_case(case, "histogram")
