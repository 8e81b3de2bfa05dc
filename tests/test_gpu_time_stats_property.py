"""Randomised parity of the time statistics (gs_time_stats_*, gs_members_time_stats_*) against their restatement
(tests/time_stats_ref.py: Accumulators): every raw accumulator and every result plane of every plane of a case, bit for bit
through time_stats_ref.same_bits, which leaves a NaN's sign and payload free and nothing else.

`cases()` draws

* the shape: rows on either side of a workgroup's four waves, of 8 and of 16; columns 1 .. 9, on either side of one and two
  blocks of 256 and of one and two steps of the column loop at every unroll depth (512, 1024, 2048); planes wider than 2053
  columns have at most five rows; half of the fields' shapes have cols % 64 == 0, so that the plane is dense and
  accumulate_slab rescans it, slab by slab, as rows of up to 4096 columns (`scan_shape` restates its rule);
* the groups, by unroll class (one group: 8 blocks per step, two: 4, three or four: 2), 1 .. 6 samples, stamps with 0,
  consecutive values, repeats and 0xFFFFFFFE among them, values from time_stats_ref.sample_planes or from the float
  property's planes with its SALT -- and in every case cells that are set in the last sample alone, cells that are never
  set, and cells where +inf and -inf arrive in different samples (sum is NaN);
* a threshold and a sense per plane (both zeros, a sub-normal, +-inf and the largest finite value among them): the planes of
  a case never all share one rule;
* the call: Species.time_stats with its 2 planes, the C ABI itself with 1, 3 or 4 fields, Ensemble.time_stats with a range of
  1 .. 17 members (half of the shapes ragged; members outside the range hold the poison value; half of the cases retire
  some members and advance the rest by an odd number of steps between samples, and the sample states are read back);
* for fields, a chain of 1 .. 5 slabs on one device (one-row slabs occur), pitch_pad 0 or 3, and `poison`: NaN or 3.0e38 in
  every ghost row and in the pitch padding of every sample field;
* `reset` after the second sample in a third of the cases: the case goes on from a fresh restatement.

Beyond parity, per case: min <= mean <= max and variance >= 0 where all samples are finite; set_count == 0 exactly where
first_stamp == 0xFFFFFFFF; arrival is -1 or one of the stamps; occupancy * samples rounds to set_count; in a quarter of the
cases min, max and first_stamp after every sample follow from those before it by the rule; several slabs equal one; a
member equals a lone Species fed the same planes; 1 .. 4 planes in one object equal one object per plane; the sample fields
download as uploaded with the poison in place; the context's counters stand still; a result plane's summary() is that of a
field uploaded from the restatement's plane.

Parity with a restatement cannot see an error that the restatement shares: in cases of at most EXACT_CELLS cells, sum and
squares of cells with finite samples alone are held to math.fsum over their terms within sum_bound, the bound of any order
of additions, and mean to the exact quotient within that bound over the count plus half an f32 unit in the last place.
(math.fsum rounds the exact sum once more; of six terms that half unit is a good part of the bound, so a cell beyond the
bound from fsum, or within a millionth of the mean's margin, is decided against the exact sum in rationals.)  Pinned
examples alone take more than 6 samples: three of 34 .. 40 on a few cells, where squares / n - mean^2 can fall below zero.
tests/test_time_stats_property_cpu.py checks without a GPU that the strategy draws legal cases of every kind, what
`scan_shape` says of the pinned examples, and that the pinned examples and the exact checks would notice each single fault."""
import collections
import ctypes
import math
import os
import time
from fractions import Fraction

import numpy as np
import pytest
from hypothesis import HealthCheck, example, given, settings, strategies as st

from grayscott_amd import HipArgs, HipConcentration, Parameters, Simulation, capi

from . import summary_ref
from . import time_stats_ref as ref
from . import test_gpu_float_observe_property as F
from .test_gpu_float_observe_property import sum_bound
from .test_gpu_observe_property import CELL_CAP, GHOST_ROWS, MEMBER_CAP, poison, ragged, same, shortest_slab

pytestmark = pytest.mark.gpu

FORMS = ["species", "abi", "ensemble"]
EXACT_CELLS = 20_000
INF = float("inf")
THRESHOLDS = [0.25, 0.5, 0.0, -0.0, 2.0 ** -130, INF, -INF, 3.4028235e38]
STAMPS = [0, 1, 2, 3, 10, 11, 40, 41, 4000000000, 0xFFFFFFFE]
POISONS = F.POISONS
VALUES = ["samples"] + F.KINDS           # time_stats_ref.sample_planes, or a kind of the float property's make_plane

# The kernel's units, restated (grayscott_amd/csrc/gs_time_stats.hip, gs_time_stats.cpp)
BLOCK_COLS = 256                        # a wave's 64 lanes of four columns
SCAN_COLS = 4096                        # the widest row a dense plane is rescanned as
CLASSES = {"one group": [1, 2, 4, 8], "two groups": [3, 5, 6, 9, 10, 12], "three or four groups": [7, 11, 13, 14, 15]}


def unroll(groups):
    """tstat_unroll: blocks of 256 columns whose loads a wave issues ahead -- what a lane holds of them within 96 VGPRs."""
    held = 4 + 8 * bin(groups & 15).count("1")
    return 8 if 96 // held >= 8 else 4 if 96 // held >= 4 else 2


def step_of(groups):
    """Columns the kernel's column loop advances by."""
    return BLOCK_COLS * unroll(groups)


def class_of(groups):
    return next(k for k, v in CLASSES.items() if groups in v)


STEPS = sorted({step_of(g) for g in range(1, 16)})          # 512, 1024, 2048
ROWS = F.ROWS                                               # 1 .. 5, either side of 4, 8, 12 and of 8, 16, 32
COLS = sorted(set(range(1, 10)) | {m * BLOCK_COLS + d for m in (1, 2) for d in range(-5, 6)}
              | {m * s + d for s in STEPS for m in (1, 2) for d in range(-5, 6)})
DENSE_COLS = [64, 128, 192, 256, 512, 1024, 2048, 4096]     # fields: cols % 64 == 0, pitch == cols without pitch_pad
SMALL_COLS = [10, 12, 16, 30, 32, 64]                       # ensembles: members whose cells make short dense rows
ENSEMBLE_SHAPES = F.ENSEMBLE_SHAPES                         # (5, 301), (2, 1031), (1, 2101), (1, 4099): the ragged form
rows_ok = F.rows_ok                                         # wider than 2053 columns: five rows at most

SEEN = collections.Counter()
SLOWEST = [""]                          # which example took longest, for the report


def field_pitch(cols, pitch_pad):
    """A field's pitch: a multiple of 64, plus the pad rounded up to a multiple of 4 (gs_fields.cpp: plane_layout)."""
    return (cols + 63) // 64 * 64 + ((pitch_pad + 3) // 4 * 4 if pitch_pad > 0 else 0)


def scan_shape(rows, cols, pitch):
    """accumulate_slab's rule: (rows, cols, pitch) a slab of `rows` rows is scanned as.  A dense one (pitch == cols) becomes
    rows of the largest power of two w with cols < w <= 4096 that divides its cells, if there is one."""
    if pitch == cols:
        w = SCAN_COLS
        while w > cols:
            if (rows * cols) % w == 0:
                return rows * cols // w, w, w
            w //= 2
    return rows, cols, pitch


def slab_rows(rows, slabs):
    return [(i + 1) * rows // slabs - i * rows // slabs for i in range(slabs)]


def planes_of(c):
    return c["nplanes"] if c["form"] == "abi" else 2


def scans(c):
    """[(rows, cols, pitch, is it the 16-byte form)] of the launches that add one sample of the case."""
    rows, cols = c["rows"], c["cols"]
    if c["form"] == "ensemble":
        r, w, p = scan_shape(c["count"] * rows, cols, cols)
        # the members' planes are allocations of their own: the range begins first * cells floats into them
        return [(r, w, p, p % 4 == 0 and (c["first"] * rows * cols) % 4 == 0)]
    pitch = field_pitch(cols, c["pitch_pad"])
    return [scan_shape(r, cols, pitch) + (True,) for r in slab_rows(rows, c["slabs"])]


def loop_count(cols, groups):
    s = step_of(groups)
    return "once" if cols < s else "exactly once" if cols == s else "more than once"


def rule_of(c, i):
    """(threshold, sense) of plane i."""
    k, above = c["rules"][i]
    return THRESHOLDS[k], above


def same_rule(a, b):
    return np.float32(a[0]) == np.float32(b[0]) and a[1] == b[1]


def pinned_case(**kw):
    """A case of `cases` with every field at its plainest value but those given (the @example cases)."""
    base = dict(form="species", rows=3, cols=261, groups=15, seed=1, values="samples", nsamples=3, stamps=[3, 4, 4, 9, 2, 7],
                rules=[(0, True), (1, False), (4, True), (7, False)], nplanes=2, slabs=1, pitch_pad=0, poison=False, poison_value=0,
                members=1, first=0, count=1, retire=False, retired=[False] * 17, steps=1, reset=False, watch=False)
    base.update(kw)
    return base


@st.composite
def cases(draw, form=None):
    form = form or draw(st.sampled_from(FORMS))
    groups = draw(st.sampled_from(CLASSES[draw(st.sampled_from(sorted(CLASSES)))]))
    rules = [(draw(st.integers(0, len(THRESHOLDS) - 1)), draw(st.booleans())) for _ in range(4)]
    if same_rule((THRESHOLDS[rules[0][0]], rules[0][1]), (THRESHOLDS[rules[1][0]], rules[1][1])):
        rules[1] = (rules[1][0], not rules[1][1])           # no case whose planes all share one rule
    c = pinned_case(form=form, groups=groups, seed=draw(st.integers(0, 2 ** 16)), values=draw(st.sampled_from(VALUES)),
                    nsamples=draw(st.integers(1, 6)), stamps=[draw(st.sampled_from(STAMPS)) for _ in range(6)], rules=rules,
                    poison=draw(st.booleans()), poison_value=draw(st.integers(0, 1)), retire=draw(st.booleans()),
                    retired=[draw(st.booleans()) for _ in range(17)], steps=draw(st.sampled_from([1, 3, 5])),
                    reset=draw(st.integers(0, 2)) == 0, watch=draw(st.integers(0, 3)) == 0)
    rows = draw(st.sampled_from(ROWS))
    if form == "ensemble":
        want_ragged = draw(st.booleans())
        if want_ragged and draw(st.integers(0, 3)) == 0:
            rows, cols = draw(st.sampled_from(ENSEMBLE_SHAPES))
        else:
            cols = draw(st.sampled_from([x for x in sorted(set(COLS) | set(SMALL_COLS))
                                         if rows * x <= MEMBER_CAP and rows_ok(rows, x) and ragged((rows, x)) == want_ragged]))
        members = draw(st.integers(1, max(1, min(17, CELL_CAP // (2 * rows * cols)))))
        first = draw(st.integers(0, members - 1))
        c.update(rows=rows, cols=cols, members=members, first=first, count=draw(st.integers(1, members - first)))
        return c
    if draw(st.booleans()):
        cols = draw(st.sampled_from([x for x in DENSE_COLS if rows_ok(rows, x)]))
    else:
        cols = draw(st.sampled_from([x for x in COLS if rows_ok(rows, x)]))
    nplanes = draw(st.sampled_from([1, 3, 4])) if form == "abi" else 2
    c.update(rows=rows, cols=cols, nplanes=nplanes, slabs=min(draw(st.integers(1, 5)), rows), pitch_pad=draw(st.sampled_from([0, 0, 3])))
    return c


def legal(c):
    """The strategy's own check (tests/test_time_stats_property_cpu.py draws cases on the CPU).  Nothing is refused by the
    time statistics on a chain of one process: every case runs as it is drawn."""
    rows, cols, form = c["rows"], c["cols"], c["form"]
    assert form in FORMS and 1 <= c["groups"] <= 15 and c["values"] in VALUES and 1 <= c["nsamples"] <= len(c["stamps"])
    assert len(c["stamps"]) >= 6 and all(0 <= s < ref.NEVER for s in c["stamps"]) and c["steps"] % 2 == 1
    assert len(c["rules"]) == 4 and all(0 <= k < len(THRESHOLDS) for k, _ in c["rules"]) and c["poison_value"] in (0, 1)
    assert rows >= 1 and cols >= 1 and rows_ok(rows, cols) and c["pitch_pad"] in (0, 3)
    n = planes_of(c)
    assert n == 1 or not all(same_rule(rule_of(c, 0), rule_of(c, i)) for i in range(1, n))
    if form == "ensemble":
        assert 1 <= c["members"] <= 17 and 0 <= c["first"] and c["count"] >= 1 and c["first"] + c["count"] <= c["members"]
        assert rows * cols <= MEMBER_CAP and 2 * c["members"] * rows * cols <= CELL_CAP
    else:
        assert 1 <= c["slabs"] <= min(5, rows) and n * rows * cols <= CELL_CAP and (form == "species" or n in (1, 3, 4))
    for r, w, p, _ in scans(c):
        assert r >= 1 and 1 <= w <= p and w <= max(cols, SCAN_COLS)
    assert sum(r * w for r, w, _, _ in scans(c)) == rows * cols * (c["count"] if form == "ensemble" else 1)


# ---- values ------------------------------------------------------------------------------------------------------------------
def centre(t):
    """Where the samples of a plane with threshold t lie."""
    t = float(np.float32(t))
    return t if math.isfinite(t) and abs(t) < 1e30 else 0.5


def set_value(t, above):
    """The value nearest to threshold t that is set (None: nothing is above +inf or below -inf)."""
    t32 = np.float32(t)
    if np.isinf(t32):
        return None if (t32 > 0) == above else np.float32(0.0)
    with np.errstate(over="ignore"):
        return np.nextafter(t32, np.float32(INF if above else -INF))


def marked_cells(size, seed):
    """Three disjoint sets of flat cell indices: set in the last sample alone, never set, both infinities."""
    k = max(1, size // 16)
    at = np.random.default_rng(seed + 5).permutation(size)
    return at[:k], at[k:2 * k], at[2 * k:3 * k]


def plane_samples(c, i, members=None):
    """The samples of plane i of a case: [nsamples] arrays of the plane's shape ([members, rows, cols] for an ensemble's
    species), all drawn from the case's seed."""
    shape2, n = (c["rows"], c["cols"]), c["nsamples"]
    shape = shape2 if members is None else (members,) + shape2
    t, above = rule_of(c, i)
    seed = c["seed"] + 1000 * i
    if c["values"] == "samples":
        out = ref.sample_planes(shape, seed, centre(t), n)
    else:
        fc = dict(rows=c["rows"], cols=c["cols"], kind=c["values"], salt=2, edges=False, family="summary")
        out = [np.stack([F.make_plane(fc, seed + 10 * k + 100 * m) for m in range(members or 1)]).reshape(shape) for k in range(n)]
    out = [np.ascontiguousarray(x, np.float32).copy() for x in out]
    last_only, never, infs = marked_cells(out[0].size, seed)
    t32, hit = np.float32(t), set_value(t, above)
    for k, x in enumerate(out):
        x.flat[never] = t32                                   # a cell equal to the threshold is not set, under either sense
        x.flat[last_only] = hit if k == n - 1 and hit is not None else t32
    if n > 1:
        out[0].flat[infs] = np.float32(INF)
        out[-1].flat[infs] = np.float32(-INF)
    return out


def fresh_acc(c, shape, i):
    t, above = rule_of(c, i)
    return ref.Accumulators(shape, c["groups"], t if c["groups"] & ref.CROSSINGS else None, above)


# ---- exact arithmetic --------------------------------------------------------------------------------------------------------
def ulp32(q):
    """The f32 unit in the last place at |q| (q: f64 array)."""
    _, e = np.frexp(np.abs(q))
    return np.ldexp(1.0, np.where(q == 0, -149, np.maximum(e - 1, -126) - 23))


def exact_mean_ok(got, terms, n, bound):
    """|got - sum(terms) / n| <= bound / n + ulp32(sum(terms) / n) / 2 in rational arithmetic."""
    if not math.isfinite(got):                               # (the mean of finite f32 samples is no larger than the largest)
        return False
    q = sum(Fraction(float(x)) for x in terms) / n
    if q == 0:
        ulp = Fraction(2) ** -149
    else:
        e = abs(q).numerator.bit_length() - q.denominator.bit_length()
        while Fraction(2) ** e > abs(q):
            e -= 1
        while Fraction(2) ** (e + 1) <= abs(q):
            e += 1
        ulp = Fraction(2) ** (max(e, -126) - 23)
    return abs(Fraction(float(got)) - q) <= Fraction(bound) / n + ulp / 2


def check_exact(samples, raw_sum, raw_squares, mean, what):
    """`raw_sum`, `raw_squares` (f64) and `mean` (f32; any may be None) of one plane against exact arithmetic over `samples`,
    in the cells all of whose samples are finite."""
    x = np.stack([s.astype(np.float64).ravel() for s in samples], axis=1)       # [cells, samples]
    n = x.shape[1]
    fin = np.isfinite(x).all(axis=1)
    cells = np.flatnonzero(fin)
    x = x[fin]
    for got, terms, name in ((raw_sum, x, "sum"), (raw_squares, x * x, "squares")):    # (a 24-bit significand squared is exact)
        if got is None:
            continue
        got = got.ravel()[fin]
        exact = np.array([math.fsum(r) for r in terms.tolist()])
        bound = sum_bound(n, 1.0) * np.array([math.fsum(r) for r in np.abs(terms).tolist()])
        # (math.fsum is the exact sum rounded once: with so few terms that half unit is a good part of the bound, so a cell
        # that is further than the bound from fsum is held to the sum in rationals before it is called wrong)
        bad = [j for j in np.flatnonzero(~(np.abs(got - exact) <= bound))
               if not np.isfinite(got[j]) or abs(Fraction(float(got[j])) - sum(Fraction(t) for t in terms[j].tolist())) > Fraction(float(bound[j]))]
        assert not bad, f"{what}: {name} of cell {cells[bad[0]]}: {got[bad[0]]!r}, exactly {exact[bad[0]]!r}: off by more than {bound[bad[0]]!r}"
    if mean is None:
        return
    got = mean.ravel()[fin].astype(np.float64)
    exact = np.array([math.fsum(r) for r in x.tolist()])
    bound = sum_bound(n, 1.0) * np.array([math.fsum(r) for r in np.abs(x).tolist()])
    q = exact / n
    margin = bound / n + ulp32(q) / 2
    diff = np.abs(got - q)
    # f64 decides wherever it can: its own error is some 2^-52 of the quotient, 2^-28 of the margin; the cells it cannot
    # decide -- a difference within a millionth of the margin, a quotient that close to a power of two -- go to rationals
    m, _ = np.frexp(np.abs(q))
    near = (np.abs(diff - margin) <= 1e-6 * margin) | (np.abs(m - 0.5) < 1e-6) | (m > 1 - 1e-6)
    bad = np.flatnonzero((diff > margin) & ~near)
    assert bad.size == 0, f"{what}: mean of cell {cells[bad[0]]}: {got[bad[0]]!r}, exactly {q[bad[0]]!r}: off by more than {margin[bad[0]]!r}"
    for j in np.flatnonzero(near):
        assert exact_mean_ok(got[j], x[j], n, bound[j]), f"{what}: mean of cell {cells[j]}: {got[j]!r}, not within the bound of {q[j]!r}"


# ---- pinned examples ---------------------------------------------------------------------------------------------------------
def _rules(*pairs):
    return list(pairs) + [(0, True)] * (4 - len(pairs))


_ONE, _TWO, _MANY = CLASSES["one group"], CLASSES["two groups"], CLASSES["three or four groups"]
# The cases that must always run:
# - per unroll class on the 16-byte form, widths S - 1, S, S + 1, S + 5 and 2 S + 5 of the class's column-loop step S (pitch_pad
#   or an odd row count keeps the plane from being rescanned), the group sets of the class in turn;
# - (8, 64) on 4, 2 and 1 slabs and (16, 128): dense rows of 128, 256, 512 and 2048 columns;
# - per unroll class on the ragged form, ensembles of (5, 301), (2, 1031), (1, 2101) and (1, 4099) columns: with the above,
#   every one of the fifteen group sets;
# - dense planes: fields of (16, 256) and (64, 64) on one slab (one row of 4096 each), (24, 128) on three slabs (a row of 1024
#   each), (5, 256) (as it lies), 2 members of (8, 256), 17 members of (3, 10) with the ranges [1, 17) -- 480 cells as 15 rows
#   of 32, begun 120 bytes into the plane: the ragged form on rows of a multiple of 4 columns -- and [0, 16);
# - shapes (1, 1), (1, 4), (4, 1); 1, 3 and 4 planes through the C ABI with four different rules; chains of 5 slabs over 5 rows;
# - both zeros, a sub-normal, both infinities and the largest finite value as thresholds; stamps 0, repeats, 0xFFFFFFFE; reset
#   after the second sample; NaN and 3.0e38 beside the planes; retired members;
# - three cases of 34 .. 40 samples on a few cells, the only pinned ones beyond the 6 that are drawn: squares / n - mean^2 of
#   f32 samples falls below zero through rounding alone, and then only from 33 equal samples of a full significand on (the
#   cells that are never set hold the threshold 3.4028235e38 in every sample), so nothing shorter shows a missing clamp.
EDGE_EXAMPLES = (
    [pinned_case(form=form, rows=r, cols=step_of(cls[0]) * m + d, groups=cls[k % len(cls)], pitch_pad=pad, poison=True, poison_value=k % 2,
                 slabs=s, nplanes=n, seed=20 + k, nsamples=3 + k % 3, stamps=stamps, reset=k % 3 == 1, watch=k % 2 == 0,
                 rules=_rules((k % 8, True), ((k + 3) % 8, False), ((k + 4) % 8, k % 2 == 0), ((k + 6) % 8, True)))
     for cls in (_ONE, _TWO, _MANY)
     for k, (m, d, r, pad, s, form, n, stamps) in enumerate((
         (1, -1, 3, 0, 1, "species", 2, [0, 0, 1, 2, 3, 10]), (1, 0, 3, 3, 2, "abi", 3, [3, 10, 11, 11, 40, 41]),
         (1, 1, 2, 3, 1, "abi", 1, [0xFFFFFFFE, 0, 1, 1, 2, 3]), (1, 5, 5, 0, 5, "species", 2, [10, 10, 10, 0, 1, 2]),
         (2, 5, 2, 3, 2, "abi", 4, [1, 0, 0xFFFFFFFE, 4000000000, 2, 2])))]
    + [pinned_case(form="ensemble", rows=r, cols=w, groups=g, members=m, first=a, count=n, retire=ret,
                   retired=[False, True, True, False, True, False] + [False] * 11, steps=3, poison_value=g % 2, seed=w + g,
                   nsamples=2 + g % 4, stamps=[0, 3, 3, 0xFFFFFFFE, 10, 11][g % 3:] + [1, 2, 40][:g % 3], reset=g % 4 == 1, watch=g % 5 == 0,
                   values=VALUES[g % len(VALUES)], rules=_rules((g % 8, g % 2 == 0), ((g + 5) % 8, g % 3 == 0)))
       for (r, w, m, a, n, ret), gs in (
           ((5, 301, 4, 1, 2, False), (1, 3, 7, 12)), ((2, 1031, 3, 0, 3, True), (2, 5, 11, 9)),
           ((1, 2101, 6, 2, 3, True), (4, 6, 13, 10)), ((1, 4099, 2, 1, 1, False), (8, 14, 15, 3)))
       for g in gs]
    + [pinned_case(form=form, rows=r, cols=w, slabs=s, groups=g, nplanes=n, seed=60 + k, poison=p, poison_value=k % 2, reset=k == 2,
                   watch=k == 0, nsamples=4, values=v, rules=_rules((2, False), (3, True), (5, False), (6, True)))
       for k, (form, r, w, s, g, n, p, v) in enumerate((
           ("species", 16, 256, 1, 15, 2, True, "samples"), ("abi", 64, 64, 1, 6, 3, True, "order"), ("species", 24, 128, 3, 1, 2, True, "special"),
           ("abi", 5, 256, 1, 10, 1, False, "samples"), ("abi", 5, 256, 5, 7, 4, True, "samples"), ("species", 5, 9, 5, 8, 2, True, "stress"),
           ("species", 8, 64, 4, 13, 2, True, "samples"), ("abi", 8, 64, 2, 3, 3, True, "order"), ("abi", 8, 64, 1, 2, 1, False, "special"),
           ("abi", 16, 128, 1, 5, 1, False, "samples")))]
    + [pinned_case(form="ensemble", rows=r, cols=w, members=m, first=a, count=n, groups=g, seed=80 + k, retire=ret, nsamples=3,
                   retired=[k % 2 == 0, True] + [False, True] * 7 + [False], steps=1, reset=k == 1, watch=k == 3,
                   rules=_rules((4, True), (7, False)))
       for k, (r, w, m, a, n, g, ret) in enumerate(((8, 256, 2, 0, 2, 15, False), (3, 10, 17, 1, 16, 15, False), (3, 10, 17, 0, 16, 9, True),
                                                    (3, 10, 17, 1, 16, 4, True), (4, 8, 3, 1, 2, 12, False)))]
    + [pinned_case(form=form, rows=r, cols=w, groups=g, nplanes=n, seed=90 + k, nsamples=ns, poison=True, poison_value=k % 2, reset=ns > 4,
                   stamps=[0, 0, 5, 5, 0xFFFFFFFE, 1], rules=_rules((0, True), (2, False), (4, True), (7, False)), pitch_pad=3 * (k % 2))
       for k, (form, r, w, g, n, ns) in enumerate((("species", 1, 1, 15, 2, 1), ("abi", 1, 4, 13, 3, 2), ("abi", 4, 1, 11, 4, 6),
                                                   ("abi", 1, 1, 8, 1, 3), ("abi", 9, 517, 14, 4, 5)))]
    + [pinned_case(form=form, rows=r, cols=w, groups=g, nplanes=n, seed=95 + k, nsamples=ns, stamps=[s // 2 for s in range(ns)],
                   members=m, first=a, count=m - a, slabs=min(r, 2), poison=True, rules=_rules((7, True), (7, False), (1, True), (1, False)))
       for k, (form, r, w, g, n, ns, m, a) in enumerate((("species", 2, 5, 15, 2, 34, 1, 0), ("abi", 1, 9, 11, 4, 40, 1, 0),
                                                         ("ensemble", 3, 10, 15, 2, 36, 3, 1)))])


def _with_examples(form):
    def decorate(test):
        for ex in reversed([e for e in EDGE_EXAMPLES if e["form"] == form]):
            test = example(case=ex)(test)
        return test
    return decorate


def counts_of(c):
    """What the run report counts an example under."""
    legal(c)
    out = ["examples", "form " + c["form"], f"planes {planes_of(c)}", f"samples {c['nsamples']}"]
    out += ["reset"] if c["reset"] and c["nsamples"] > 2 else []
    out += ["watched"] if c["watch"] else []
    for r, w, p, vec in set(scans(c)):
        form = "16 bytes" if vec else "ragged"
        out.append(f"{class_of(c['groups'])}, {form}, loop {loop_count(w, c['groups'])}")
        out.append("padded rows" if p != w else f"dense, width {w}" if w != c["cols"] else "dense, as it lies")
    if c["form"] == "ensemble":
        out.append("ensemble load path " + ("16 bytes" if scans(c)[0][3] else "ragged"))
        out += ["retired members"] if c["retire"] else []
    else:
        out.append(f"slabs {c['slabs']}")
        out += ["poisoned"] if c["poison"] else []
        out += ["pitch_pad"] if c["pitch_pad"] else []
        out += ["one-row slabs"] if shortest_slab(c["rows"], c["slabs"]) == 1 and c["slabs"] > 1 else []
    return out


# ---- on the device -----------------------------------------------------------------------------------------------------------
COUNTERS = ("launches", "steps", "passes", "ghost_refreshes")
RAW_CODE = {"sum": capi.GS_TSTAT_RAW_SUM, "squares": capi.GS_TSTAT_RAW_SQUARES, "min": capi.GS_TSTAT_RAW_MIN,
            "max": capi.GS_TSTAT_RAW_MAX, "set_count": capi.GS_TSTAT_RAW_SET_COUNT, "first_stamp": capi.GS_TSTAT_RAW_FIRST_STAMP}
RESULT_CODE = {"mean": capi.GS_TSTAT_MEAN, "variance": capi.GS_TSTAT_VARIANCE, "min": capi.GS_TSTAT_MIN, "max": capi.GS_TSTAT_MAX,
               "occupancy": capi.GS_TSTAT_OCCUPANCY, "arrival": capi.GS_TSTAT_ARRIVAL}


class AbiStats:
    """Time statistics of 1 .. 4 fields through the C ABI itself: gs_time_stats_create, _accumulate, _result, _download."""

    def __init__(self, ctx, shape, fields, groups, rules):
        self.ctx, self.lib, self.shape, self.fields, self.h = ctx, capi.load(), tuple(shape), list(fields), ctypes.c_void_p()
        n = len(fields)
        t = (ctypes.c_float * 4)(*([float(r[0]) for r in rules] + [0.0] * (4 - n)))
        a = (ctypes.c_int32 * 4)(*([int(r[1]) for r in rules] + [0] * (4 - n)))
        crossing = bool(groups & ref.CROSSINGS)
        capi.check(self.lib.gs_time_stats_create(ctx.handle, ctypes.byref(self.h), shape[0], shape[1], n, groups,
                                                 t if crossing else None, a if crossing else None))

    def accumulate(self, stamp):
        handles = (ctypes.c_void_p * 4)(*[f.handle for f in self.fields])
        capi.check(self.lib.gs_time_stats_accumulate(self.ctx.handle, self.h, handles, len(self.fields), int(stamp)))

    @property
    def samples(self):
        n = ctypes.c_uint64()
        capi.check(self.lib.gs_time_stats_samples(self.h, ctypes.byref(n)))
        return int(n.value)

    def reset(self):
        capi.check(self.lib.gs_time_stats_reset(self.ctx.handle, self.h))

    def raw(self, name, plane):
        out = np.empty(self.shape, np.float64 if name in ("sum", "squares") else np.float32 if name in ("min", "max") else np.uint32)
        capi.check(self.lib.gs_time_stats_download(self.ctx.handle, self.h, plane, RAW_CODE[name], out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def result(self, name, plane):
        out = HipConcentration(self.ctx, self.shape)
        capi.check(self.lib.gs_time_stats_result(self.ctx.handle, self.h, plane, RESULT_CODE[name], out.handle))
        return out

    def close(self):
        if self.h:
            capi.check(self.lib.gs_time_stats_destroy(self.ctx.handle, self.h))
        self.h = ctypes.c_void_p()


def raw_of(stats, name, i):
    return stats.raw(name, i) if isinstance(stats, AbiStats) else stats.raw(name, "uv"[i])


def result_of(stats, name, i):
    """A result plane as the library hands it out: a field, or for an ensemble an array."""
    return stats.result(name, i) if isinstance(stats, AbiStats) else getattr(stats, name)("uv"[i])


def make_stats(ctx, c, source, fields, rules, first=0, count=None):
    groups, crossing = c["groups"], bool(c["groups"] & ref.CROSSINGS)
    if isinstance(source, list):
        return AbiStats(ctx, (c["rows"], c["cols"]), fields, groups, rules)
    kw = dict(u_threshold=rules[0][0], v_threshold=rules[1][0], above=(rules[0][1], rules[1][1])) if crossing else {}
    if c["form"] == "ensemble" and count is not None:
        kw.update(first=first, count=count)
    return source.time_stats(groups, **kw)


def margins_hold(field, value):
    """Do the ghost rows of every slab of `field` and the pitch padding of its rows still hold `value` (test_gpu_observe_
    property.poison wrote it there)?"""
    import torch

    class _DeviceArray:
        def __init__(self, address, rows, pitch):
            self.__cuda_array_interface__ = {"shape": (rows, pitch), "typestr": "<f4", "data": (address, False), "version": 3,
                                             "strides": (pitch * 4, 4)}

    _, pitch = field.raw_shape()
    cols = field.shape()[1]
    want = np.float32(value)
    for address, _, _, rows, device in field.device_slabs():
        view = torch.as_tensor(_DeviceArray(address - GHOST_ROWS * pitch * 4, rows + 2 * GHOST_ROWS, pitch), device=f"cuda:{device}")
        a = view.cpu().numpy()
        beside = np.concatenate([a[:GHOST_ROWS].ravel(), a[GHOST_ROWS + rows:].ravel(), a[:, cols:].ravel()])
        if not (np.isnan(beside).all() if np.isnan(want) else (beside == want).all()):
            return False
    return True


def check_planes(c, i, raws, results, acc, stamps, what):
    """Plane i of a case against its restatement `acc`, and what holds of the planes themselves."""
    groups = c["groups"]
    for name in ref.raw_names(groups):
        assert ref.same_bits(raws[name], acc.raw(name)), f"{what}: raw {name} of plane {i}: {ref.describe(raws[name], acc.raw(name))}"
    for name in ref.result_names(groups):
        assert ref.same_bits(results[name], acc.result(name)), f"{what}: {name} of plane {i}: {ref.describe(results[name], acc.result(name))}"
    with np.errstate(invalid="ignore"):
        if groups & ref.EXTREMES:                            # every sample of the cell is finite: so are its extremes
            fin = np.isfinite(raws["min"]) & np.isfinite(raws["max"]) & (np.isfinite(raws["sum"]) if groups & ref.SUM else True)
            assert (raws["min"][fin] <= raws["max"][fin]).all(), what
            if groups & ref.SUM:
                assert ((results["min"][fin] <= results["mean"][fin]) & (results["mean"][fin] <= results["max"][fin])).all(), f"{what}: mean of plane {i}"
        if groups & ref.SUM and groups & ref.SQUARES:
            fin = np.isfinite(raws["sum"]) & np.isfinite(raws["squares"])
            assert (results["variance"][fin] >= 0).all(), f"{what}: variance of plane {i}"
    if groups & ref.CROSSINGS:
        assert ((raws["set_count"] == 0) == (raws["first_stamp"] == ref.NEVER)).all(), f"{what}: plane {i}"
        allowed = np.array([-1.0] + [float(np.float32(s)) for s in stamps], np.float32)
        assert np.isin(results["arrival"], allowed).all(), f"{what}: arrival of plane {i}"
        n = acc.samples
        assert (np.rint(results["occupancy"].astype(np.float64) * n) == raws["set_count"]).all(), f"{what}: occupancy of plane {i}"
        assert (raws["set_count"] <= n).all(), what


def check_step(c, before, after, x, rule, stamp, what):
    """min, max, set_count and first_stamp after a sample `x` from those before it (both read from the device)."""
    with np.errstate(invalid="ignore"):
        if c["groups"] & ref.EXTREMES:
            assert ref.same_bits(after["min"], np.where(x < before["min"], x, before["min"])), f"{what}: min after stamp {stamp}"
            assert ref.same_bits(after["max"], np.where(x > before["max"], x, before["max"])), f"{what}: max after stamp {stamp}"
        if c["groups"] & ref.CROSSINGS:
            hit = ref.is_set(x, rule[0], rule[1])
            assert same(after["set_count"], before["set_count"] + hit.astype(np.uint32)), f"{what}: set_count after stamp {stamp}"
            want = np.where(hit & (before["first_stamp"] == ref.NEVER), np.uint32(stamp), before["first_stamp"])
            assert same(after["first_stamp"], want), f"{what}: first_stamp after stamp {stamp}"


def run_fields(c, samples, slabs, pitch_pad, poisoned, accs=None, what=""):
    """The samples of a field case through Species.time_stats or the C ABI on a chain of `slabs` slabs: {(plane, name): raw
    accumulator}.  With `accs` (the restatement's accumulators, fed along) everything is checked on the way."""
    n, shape, groups = len(samples), (c["rows"], c["cols"]), c["groups"]
    rules = [rule_of(c, i) for i in range(n)]
    stamps = c["stamps"][:c["nsamples"]]
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * slabs, pitch_pad=pitch_pad))
    ctx = sim.context
    try:
        if c["form"] == "species":
            from .helpers import species_from_arrays

            source = species_from_arrays(sim, samples[0][0], samples[1][0])
            fields = list(source.in_out()[:2])
        else:
            source = fields = [HipConcentration(ctx, shape) for _ in range(n)]
            for f, s in zip(fields, samples):
                f.upload(ctx, s[0])
        if poisoned:
            for f in fields:
                poison(f, POISONS[c["poison_value"]])
        stats = make_stats(ctx, c, source, fields, rules)
        singles = []
        if accs is not None and c["form"] == "abi" and n > 1:             # one object per plane
            singles = [AbiStats(ctx, shape, [fields[i]], groups, [rules[i]]) for i in range(n)]
        watched = None
        for k, stamp in enumerate(stamps):
            for f, s in zip(fields, samples):
                f.upload(ctx, s[k])
            ctx.sync()
            counters = {key: ctx.stats()[key] for key in COUNTERS}
            if accs is not None and c["watch"]:
                watched = [{name: raw_of(stats, name, i) for name in ref.raw_names(groups)} for i in range(n)]
            for s in [stats] + singles:
                s.accumulate(stamp)
            if accs is not None:
                assert {key: ctx.stats()[key] for key in COUNTERS} == counters, f"{what}: the context's counters"
                for i in range(n):
                    accs[i].accumulate(samples[i][k], stamp)
                if c["watch"]:
                    for i in range(n):
                        now = {name: raw_of(stats, name, i) for name in ref.raw_names(groups)}
                        check_step(c, watched[i], now, samples[i][k], rules[i], stamp, f"{what}: plane {i}")
                assert stats.samples == accs[0].samples, what
            if c["reset"] and k == 1:
                for s in [stats] + singles:
                    s.reset()
                assert stats.samples == 0, what
                if accs is not None:
                    accs[:] = [fresh_acc(c, shape, i) for i in range(n)]
        counters = {key: ctx.stats()[key] for key in COUNTERS}
        raws = {(i, name): raw_of(stats, name, i) for i in range(n) for name in ref.raw_names(groups)}
        if accs is None or accs[0].samples == 0:                 # (reset after the last sample: no result plane to ask for)
            if accs is not None:
                for (i, name), got in raws.items():
                    assert ref.same_bits(got, accs[i].raw(name)), f"{what}: raw {name} of plane {i} after reset"
            return raws
        summarised = False
        for i in range(n):
            results = {}
            for name in ref.result_names(groups):
                plane = result_of(stats, name, i)
                results[name] = plane.make_scalar_view(ctx)
                if not summarised:                                # a result plane is a field like any other
                    twin = HipConcentration(ctx, shape)
                    twin.upload(ctx, accs[i].result(name))
                    assert summary_ref.same(plane.summary(ctx), twin.summary(ctx)), f"{what}: summary of {name}"
                    twin.destroy()
                    summarised = True
                plane.destroy()
            mine = {name: raws[(i, name)] for name in ref.raw_names(groups)}
            check_planes(c, i, mine, results, accs[i], stamps, what)
            for name in ref.raw_names(groups) if singles else []:
                assert ref.same_bits(raw_of(singles[i], name, 0), mine[name]), f"{what}: raw {name} of plane {i} in an object of its own"
            if n * shape[0] * shape[1] <= EXACT_CELLS and groups & (ref.SUM | ref.SQUARES):
                fed = [samples[i][k] for k in range(c["nsamples"])][2 if c["reset"] and c["nsamples"] > 2 else 0:]
                check_exact(fed, mine.get("sum"), mine.get("squares"), results.get("mean"), f"{what}: plane {i}")
        assert {key: ctx.stats()[key] for key in COUNTERS} == counters, f"{what}: the context's counters"
        for f, s in zip(fields, samples):                         # the sample fields are what was uploaded last
            assert same(f.make_scalar_view(ctx), s[c["nsamples"] - 1]), what
            assert not poisoned or margins_hold(f, POISONS[c["poison_value"]]), f"{what}: the poison"
        for s in [stats] + singles:
            s.close()
        return raws
    finally:
        ctx.close()


def run_field_case(c):
    n, shape = planes_of(c), (c["rows"], c["cols"])
    samples = [plane_samples(c, i) for i in range(n)]
    what = (f"time statistics {c['form']} {shape} x {n} groups={c['groups']} samples={c['nsamples']} stamps={c['stamps'][:c['nsamples']]} "
            f"values={c['values']} seed={c['seed']} rules={[rule_of(c, i) for i in range(n)]} slabs={c['slabs']} pitch_pad={c['pitch_pad']} "
            f"poison={POISONS[c['poison_value']] if c['poison'] else None} reset={c['reset']} watch={c['watch']} scans={scans(c)}")
    accs = [fresh_acc(c, shape, i) for i in range(n)]
    got = run_fields(c, samples, c["slabs"], c["pitch_pad"], c["poison"], accs, what)
    if c["slabs"] > 1 or c["pitch_pad"]:                          # several slabs, padded rows: one slab of plain rows
        one = run_fields(dict(c, watch=False), samples, 1, 0, False)
        for key in got:
            assert ref.same_bits(one[key], got[key]), f"{what}: one slab: raw {key[1]} of plane {key[0]}"


def run_ensemble_case(c):
    shape, members, first, count, groups = (c["rows"], c["cols"]), c["members"], c["first"], c["count"], c["groups"]
    rules = [rule_of(c, 0), rule_of(c, 1)]
    stamps = c["stamps"][:c["nsamples"]]
    retired = [m for m in range(members) if c["retired"][m]] if c["retire"] else []
    what = (f"time statistics of an ensemble of {members} x {shape}, members [{first}, {first + count}) groups={groups} "
            f"samples={c['nsamples']} stamps={stamps} values={c['values']} seed={c['seed']} rules={rules} retired={retired} "
            f"steps={c['steps'] if c['retire'] else 0} reset={c['reset']} watch={c['watch']} scans={scans(c)}")
    given = [plane_samples(c, s, members) for s in (0, 1)]       # [species][sample][member]
    outside = np.ones(members, bool)
    outside[first:first + count] = False
    for s in (0, 1):
        for x in given[s]:
            x[outside] = np.float32(POISONS[c["poison_value"]])
    accs = [fresh_acc(c, (count,) + shape, s) for s in (0, 1)]
    fed = [[], []]
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    lone = Simulation.new(Parameters(), HipArgs(devices=[0]))
    try:
        ctx = sim.context
        ens = sim.make_ensemble(shape, Parameters(), seed=False, members=members)
        stats = make_stats(ctx, c, ens, None, rules, first, count)
        for k, stamp in enumerate(stamps):
            ens.upload(given[0][k], given[1][k])
            if c["retire"]:
                if k == 0:
                    ens.retire(retired)
                ens.perform_steps(c["steps"])
            u, v = ens.u_views(), ens.result_views()
            for m in retired:                                     # a retired member holds the planes it was given
                assert same(u[m], given[0][k][m]) and same(v[m], given[1][k][m]), f"member {m}: {what}"
            x = [np.ascontiguousarray(u[first:first + count]), np.ascontiguousarray(v[first:first + count])]
            counters = {key: ctx.stats()[key] for key in COUNTERS}
            watched = [{name: raw_of(stats, name, s) for name in ref.raw_names(groups)} for s in (0, 1)] if c["watch"] else None
            stats.accumulate(stamp)
            assert {key: ctx.stats()[key] for key in COUNTERS} == counters, f"{what}: the context's counters"
            for s in (0, 1):
                accs[s].accumulate(x[s], stamp)
                fed[s].append(x[s])
                if c["watch"]:
                    now = {name: raw_of(stats, name, s) for name in ref.raw_names(groups)}
                    check_step(c, watched[s], now, x[s], rules[s], stamp, f"{what}: species {s}")
            assert stats.samples == accs[0].samples, what
            if c["reset"] and k == 1:
                stats.reset()
                assert stats.samples == 0, what
                accs = [fresh_acc(c, (count,) + shape, s) for s in (0, 1)]
                fed = [[], []]
            now_u, now_v = ens.u_views(), ens.result_views()      # the members are what they were
            assert same(now_u, u) and same(now_v, v), what
        raws = {(s, name): raw_of(stats, name, s) for s in (0, 1) for name in ref.raw_names(groups)}
        if accs[0].samples == 0:
            for (s, name), got in raws.items():
                assert ref.same_bits(got, accs[s].raw(name)), f"{what}: raw {name} of species {s} after reset"
        else:
            for s in (0, 1):
                results = {name: result_of(stats, name, s) for name in ref.result_names(groups)}
                mine = {name: raws[(s, name)] for name in ref.raw_names(groups)}
                check_planes(c, s, mine, results, accs[s], stamps, what)
                if 2 * count * shape[0] * shape[1] <= EXACT_CELLS and groups & (ref.SUM | ref.SQUARES):
                    check_exact(fed[s], mine.get("sum"), mine.get("squares"), results.get("mean"), f"{what}: species {s}")
            # the first and the last member of the range: a lone Species fed the same planes
            from .helpers import species_from_arrays

            species = species_from_arrays(lone, fed[0][0][0], fed[1][0][0])
            for j in sorted({0, count - 1}):
                alone = make_stats(lone.context, dict(c, form="species"), species, None, rules)
                for k, stamp in enumerate(stamps[len(stamps) - len(fed[0]):]):
                    in_u, in_v, _, _ = species.in_out()
                    in_u.upload(lone.context, fed[0][k][j])
                    in_v.upload(lone.context, fed[1][k][j])
                    alone.accumulate(stamp)
                for (s, name), got in raws.items():
                    assert ref.same_bits(raw_of(alone, name, s), got[j]), f"{what}: member {first + j} as a lone Species: raw {name} of species {s}"
                alone.close()
        stats.close()
        ens.destroy()
    finally:
        sim.context.close()
        lone.context.close()


def run_case(case, form):
    c = dict(case)
    assert c["form"] == form
    started = time.perf_counter()
    if form == "ensemble":
        run_ensemble_case(c)
    else:
        run_field_case(c)
    SEEN.update(counts_of(c))
    pinned = case in EDGE_EXAMPLES
    SEEN.update({"pinned examples": 1} if pinned else {"drawn examples": 1})
    took = time.perf_counter() - started
    SEEN["seconds in pinned examples" if pinned else "seconds in drawn examples"] += took
    if took > SEEN["slowest example, seconds"]:
        SEEN["slowest example, seconds"] = took
        SLOWEST[:] = [f'{c["form"]} {c["rows"]} x {c["cols"]} x {planes_of(c)}, {c["nsamples"]} samples, {c["members"]} members']


@pytest.fixture(scope="module", autouse=True)
def report():
    SEEN.clear()
    yield
    print("\ntime statistics property examples: " + ", ".join(f"{k}: {v:.4g}" for k, v in sorted(SEEN.items())) + f" ({SLOWEST[0]})")


# The default keeps the file within 1.25 times the run time of tests/test_gpu_observe_property.py
EXAMPLES = int(os.environ.get("GS_PROPERTY_EXAMPLES_TIME_STATS", "4"))
_SETTINGS = dict(max_examples=EXAMPLES, deadline=None, suppress_health_check=list(HealthCheck))


@settings(**_SETTINGS)
@given(cases("species"))
@_with_examples("species")
def test_any_species_time_statistics_match_the_reference(built, case):
    run_case(case, "species")


@settings(**_SETTINGS)
@given(cases("abi"))
@_with_examples("abi")
def test_any_time_statistics_through_the_c_abi_match_the_reference(built, case):
    run_case(case, "abi")


@settings(**_SETTINGS)
@given(cases("ensemble"))
@_with_examples("ensemble")
def test_any_ensemble_time_statistics_match_the_reference(built, case):
    run_case(case, "ensemble")
