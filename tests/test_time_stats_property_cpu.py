"""The randomised GPU parity test of the time statistics (tests/test_gpu_time_stats_property.py) without a GPU: its strategy
draws legal cases of every kind within the caps; `scan_shape` says of the pinned examples what the issue says of them; and
the pinned examples discriminate: a model of the launches -- the memory a slab's sample lies in, the rows it is scanned as,
the column loop's steps and blocks, the kernel form, the accumulators' rule, reset, the result formulas, the download -- is
held to time_stats_ref.Accumulators without a fault, and with exactly one fault each it gives other planes than the
reference on at least three pinned examples, while every pinned example tells at least one fault.  (An ensemble whose
members are retired and advanced is modelled with the planes it was given: what the steps make of them is the device's.)
The exact checks notice a sample added twice and a mean one f32 unit off."""
import collections
import functools

import numpy as np
import pytest

from . import time_stats_ref as ref
from . import test_gpu_time_stats_property as P
from .test_observe_property_cpu import flushed


# ---- the strategy ------------------------------------------------------------------------------------------------------------
def test_the_strategy_draws_legal_cases_of_every_kind():
    from hypothesis import HealthCheck, given, seed, settings

    seen = collections.Counter()

    @seed(20240611)
    @settings(max_examples=2000, deadline=None, database=None, suppress_health_check=list(HealthCheck))
    @given(P.cases())
    def draw(c):
        P.legal(c)
        seen["draws"] += 1
        seen.update(set(P.counts_of(c)) - {"examples"})
        seen.update({("values", c["values"]), ("groups", c["groups"]), ("samples", c["nsamples"]), ("poison value", c["poison_value"])})
        seen.update(("stamp", s) for s in set(c["stamps"][:c["nsamples"]]))
        seen.update(("rule", k, above) for k, above in set(c["rules"][:P.planes_of(c)]))
        if c["form"] == "ensemble":
            seen.update({("members", c["members"]), ("ragged shape", P.ragged((c["rows"], c["cols"])))})
            seen.update({("range inside",)} if c["first"] > 0 and c["first"] + c["count"] < c["members"] else {})
            assert c["rows"] * c["cols"] <= P.MEMBER_CAP
        else:
            assert P.planes_of(c) * c["rows"] * c["cols"] <= P.CELL_CAP
        if len(set(c["stamps"][:c["nsamples"]])) < c["nsamples"]:
            seen[("repeated stamp",)] += 1

    draw()
    assert seen["draws"] >= 1900, seen["draws"]
    want = (["form " + f for f in P.FORMS] + [f"planes {n}" for n in (1, 2, 3, 4)] + [f"samples {n}" for n in range(1, 7)]
            + [f"slabs {s}" for s in range(1, 6)] + ["one-row slabs", "poisoned", "pitch_pad", "padded rows", "dense, as it lies",
                                                     "reset", "watched", "retired members", "ensemble load path ragged",
                                                     "ensemble load path 16 bytes", ("repeated stamp",), ("range inside",)]
            + [f"dense, width {w}" for w in (32, 64, 128, 256, 512, 1024, 2048, 4096)]
            # (the ragged form never runs its loop exactly once: its rows either have a column count that is no multiple
            # of 4, or begin a member range whose cells per member are none -- then 17 members at most hold no multiple
            # of 512 cells, so no row is 512, 1024 or 2048 columns wide)
            + [f"{k}, {form}, loop {n}" for k in P.CLASSES for form in ("16 bytes", "ragged") for n in ("once", "exactly once", "more than once")
               if (form, n) != ("ragged", "exactly once")]
            + [("values", v) for v in P.VALUES] + [("groups", g) for g in range(1, 16)] + [("members", m) for m in range(1, 18)]
            + [("stamp", s) for s in P.STAMPS] + [("rule", k, a) for k in range(len(P.THRESHOLDS)) for a in (False, True)]
            + [("ragged shape", r) for r in (False, True)] + [("poison value", v) for v in (0, 1)])
    rare = {k: seen[k] for k in want if seen[k] < 5}
    assert not rare, rare


def test_the_kernel_units_are_what_the_source_says():
    assert [P.unroll(g) for g in (1, 2, 4, 8)] == [8] * 4 and [P.unroll(g) for g in (3, 5, 6, 9, 10, 12)] == [4] * 6
    assert [P.unroll(g) for g in (7, 11, 13, 14, 15)] == [2] * 5 and P.STEPS == [512, 1024, 2048]
    assert sorted(g for v in P.CLASSES.values() for g in v) == list(range(1, 16))
    assert P.field_pitch(300, 0) == 320 and P.field_pitch(256, 0) == 256 and P.field_pitch(256, 3) == 260 and P.field_pitch(1, 1) == 68
    assert P.slab_rows(5, 5) == [1] * 5 and P.slab_rows(24, 3) == [8] * 3 and P.slab_rows(7, 3) == [2, 2, 3]


def test_the_pinned_examples_are_scanned_as_the_issue_says():
    def find(**kw):
        found = [c for c in P.EDGE_EXAMPLES if all(c[k] == v for k, v in kw.items())]
        assert found, kw
        return found

    assert P.scan_shape(16, 256, 256) == (1, 4096, 4096) and P.scan_shape(64, 64, 64) == (1, 4096, 4096)
    assert P.scan_shape(8, 128, 128) == (1, 1024, 1024) and P.scan_shape(5, 256, 256) == (5, 256, 256)
    assert P.scan_shape(16, 256, 260) == (16, 256, 260) and P.scan_shape(3 * 8, 64, 64) == (3, 512, 512)
    assert P.scan_shape(2 * 8, 256, 256) == (1, 4096, 4096) and P.scan_shape(16 * 3, 10, 10) == (15, 32, 32)
    assert P.scan_shape(2, 1, 1) == (1, 2, 2) and P.scan_shape(1, 2048, 2048) == (1, 2048, 2048)
    for c in find(form="species", rows=16, cols=256, slabs=1) + find(form="abi", rows=64, cols=64, slabs=1):
        assert P.scans(c) == [(1, 4096, 4096, True)]
    assert P.scans(find(rows=24, cols=128, slabs=3)[0]) == [(1, 1024, 1024, True)] * 3
    assert P.scans(find(rows=5, cols=256, slabs=1)[0]) == [(5, 256, 256, True)]
    assert P.scans(find(rows=5, cols=256, slabs=5)[0]) == [(1, 256, 256, True)] * 5
    assert P.scans(find(form="ensemble", rows=8, cols=256, members=2)[0]) == [(1, 4096, 4096, True)]
    # 17 members of (3, 10): the range [1, 17) begins 120 bytes into the plane -- the ragged form on rows of 32 columns --,
    # the range [0, 16) on 16 bytes
    assert {P.scans(c)[0] for c in find(form="ensemble", cols=10, members=17, first=1)} == {(15, 32, 32, False)}
    assert P.scans(find(form="ensemble", cols=10, members=17, first=0)[0]) == [(15, 32, 32, True)]
    assert (1 * 3 * 10 * 4) % 16 == 8
    for shape in P.ENSEMBLE_SHAPES:                       # scanned as they lie, on the ragged form, at every unroll class
        found = find(form="ensemble", rows=shape[0], cols=shape[1])
        assert {P.class_of(c["groups"]) for c in found} == set(P.CLASSES)
        assert all(P.scans(c) == [(c["count"] * shape[0], shape[1], shape[1], False)] for c in found)
    for cls in P.CLASSES.values():                        # S - 1, S, S + 1, S + 5, 2 S + 5 as they lie on the 16-byte form
        s = P.step_of(cls[0])
        for w in (s - 1, s, s + 1, s + 5, 2 * s + 5):
            assert any(c["groups"] in cls and (r, x, vec) == (r, w, True) and x == c["cols"]
                       for c in P.EDGE_EXAMPLES if c["form"] != "ensemble" for r, x, _, vec in P.scans(c)), (cls, w)
    assert {c["groups"] for c in P.EDGE_EXAMPLES} == set(range(1, 16))
    assert {(c["rows"], c["cols"]) for c in P.EDGE_EXAMPLES} >= {(1, 1), (1, 4), (4, 1)}
    assert {c["nplanes"] for c in P.EDGE_EXAMPLES if c["form"] == "abi"} == {1, 3, 4}
    assert any(c["slabs"] == 5 and c["rows"] == 5 for c in P.EDGE_EXAMPLES)
    for c in P.EDGE_EXAMPLES:
        if c["form"] == "abi" and c["nplanes"] == 4 and c["groups"] & ref.CROSSINGS:
            rules = [P.rule_of(c, i) for i in range(4)]
            assert all(not P.same_rule(rules[i], rules[j]) for i in range(4) for j in range(i)), c


def test_the_pinned_examples_are_legal_and_cover_the_forms():
    counts = collections.Counter()
    for c in P.EDGE_EXAMPLES:
        counts.update(P.counts_of(c))
    need = (["form " + f for f in P.FORMS] + [f"slabs {s}" for s in (1, 2, 3, 4, 5)] + [f"planes {n}" for n in (1, 2, 3, 4)]
            + ["poisoned", "pitch_pad", "one-row slabs", "retired members", "reset", "watched", "dense, as it lies", "padded rows"]
            + [f"dense, width {w}" for w in (32, 64, 128, 256, 512, 1024, 2048, 4096)]
            + [f"{k}, {form}, loop {n}" for k in P.CLASSES for form in ("16 bytes", "ragged") for n in ("once", "more than once")]
            + [f"{k}, 16 bytes, loop exactly once" for k in P.CLASSES])
    assert all(counts[k] > 0 for k in need), {k: counts[k] for k in need if not counts[k]}


def test_every_case_holds_the_three_kinds_of_cell():
    for c in P.EDGE_EXAMPLES[::3]:
        for i in range(P.planes_of(c)):
            t, above = P.rule_of(c, i)
            x = np.stack(P.plane_samples(c, i, c["members"] if c["form"] == "ensemble" else None))
            hits = ref.is_set(x, t, above).reshape(x.shape[0], -1)
            last_only, never, infs = P.marked_cells(x[0].size, c["seed"] + 1000 * i)
            assert not hits[:, never].any() and not hits[:-1, last_only].any()
            assert hits[-1, last_only].all() or P.set_value(t, above) is None
            if c["nsamples"] > 1 and infs.size:
                with np.errstate(invalid="ignore"):
                    assert np.isnan(x.astype(np.float64).sum(axis=0).ravel()[infs]).all()


# ---- the pinned examples discriminate ----------------------------------------------------------------------------------------
STEP_FAULTS = ["step 256 (U - 1), " + k for k in P.CLASSES]       # the column loop advances by one block too few
LAYOUT_FAULTS = ["last-block-skipped",      # the last block of every unrolled group is skipped
                 "behind-group-dropped",    # the column loop runs once: the columns behind a full group are dropped
                 "tail-takes-last",         # ragged form: the columns of the last, partial quad take the last column's sample
                 "tail-not-stored",         # ... are not stored
                 "row-above-read",          # the sample is read a pitch early: a ghost row for a slab's first row
                 "pad-read",                # a row's last column reads the cell right of it: the pitch padding
                 "slab-row-off",            # a slab's accumulators are placed one row off in the download
                 "first-member-ignored",    # the member range's first member is ignored: the planes begin at member 0
                 "scan-width"]              # the dense rescanning takes a width that does not divide the cells
RULE_FAULTS = ["threshold-0", "sense-0",    # plane 0's threshold, plane 0's sense for every plane
               ">=", "nan-below", "non-strict-extremes", "nan-extreme", "last-stamp", "stamp-0-never", "squares-f32", "sum-f32", "ftz"]
RESULT_FAULTS = ["variance-unclamped", "n-1", "occupancy-f32", "reset-extremes-zero", "reset-keeps-count"]
FAULTS = STEP_FAULTS + LAYOUT_FAULTS + RULE_FAULTS + RESULT_FAULTS
GUARD = P.SCAN_COLS + 8                                            # cells in front of and behind a slab's memory


class Model:
    """The accumulators of one plane of one slab as flat arrays of rows x pitch cells, and the launch that adds a sample."""

    def __init__(self, cells, fault=None, after_reset=False):
        zero = fault == "reset-extremes-zero" and after_reset
        self.sum, self.squares = np.zeros(cells, np.float64), np.zeros(cells, np.float64)
        self.min = np.full(cells, 0 if zero else np.inf, np.float32)
        self.max = np.full(cells, 0 if zero else -np.inf, np.float32)
        self.set_count, self.first_stamp = np.zeros(cells, np.uint32), np.full(cells, ref.NEVER, np.uint32)

    def add(self, x, at, stamp, rule, rule0, fault):
        """Sample values `x` into the cells `at` (index arrays of one shape)."""
        t, above = rule
        if fault == "threshold-0":
            t = rule0[0]
        if fault == "sense-0":
            above = rule0[1]
        if fault == "ftz":
            x = flushed(x)
        with np.errstate(all="ignore"):
            x64 = x.astype(np.float64)
            if fault == "sum-f32":
                self.sum[at] = (self.sum[at].astype(np.float32) + x).astype(np.float64)
            else:
                self.sum[at] = self.sum[at] + x64
            if fault == "squares-f32":
                self.squares[at] = (self.squares[at].astype(np.float32) + x * x).astype(np.float64)
            else:
                self.squares[at] = self.squares[at] + x64 * x64
            mn, mx = self.min[at], self.max[at]
            if fault == "non-strict-extremes":
                lower, higher = x <= mn, x >= mx
            elif fault == "nan-extreme":
                lower, higher = ~(x >= mn), ~(x <= mx)
            else:
                lower, higher = x < mn, x > mx
            self.min[at], self.max[at] = np.where(lower, x, mn), np.where(higher, x, mx)
            t32 = np.float32(t)
            if fault == ">=":
                hit = x >= t32 if above else x <= t32
            else:
                hit = x > t32 if above else x < t32
            if fault == "nan-below" and not above:
                hit = hit | np.isnan(x)
        first = self.first_stamp[at]
        never = (first == ref.NEVER) | ((first == 0) if fault == "stamp-0-never" else False)
        self.set_count[at] = self.set_count[at] + hit.astype(np.uint32)
        self.first_stamp[at] = np.where(hit & (never | (fault == "last-stamp")), np.uint32(stamp), first)


def visits(cols, groups, vec, fault):
    """The launch's column loop over a row of `cols` columns: [(columns stored, columns their samples are read from)], one
    entry per time a column is added to."""
    u, cls = P.unroll(groups), P.class_of(groups)
    step = P.BLOCK_COLS * (u - 1 if fault == "step 256 (U - 1), " + cls else u)
    times = np.zeros(cols, np.int64)
    for c0 in range(0, cols, step):
        for block in range(u - 1 if fault == "last-block-skipped" else u):
            times[c0 + P.BLOCK_COLS * block:c0 + P.BLOCK_COLS * (block + 1)] += 1
        if fault == "behind-group-dropped":
            break
    src = np.arange(cols)
    tail = np.arange(cols - cols % 4, cols)                 # the last, partial quad
    if not vec and fault == "tail-takes-last":
        src[tail] = cols - 1
    if not vec and fault == "tail-not-stored":
        times[tail] = 0
    if fault == "pad-read":
        src[cols - 1] = cols
    return [(np.flatnonzero(times >= k), src[times >= k]) for k in range(1, int(times.max()) + 1 if cols else 1)]


def faulty_scan(rows, cols, pitch, fault):
    if fault == "scan-width" and pitch == cols:
        w = P.SCAN_COLS
        while w > cols:
            if w <= rows * cols:
                return rows * cols // w, w, w                # (the last, partial row is dropped)
            w //= 2
    return P.scan_shape(rows, cols, pitch)


def slab_memories(c, planes, fault):
    """Per slab of the case: (its first row in the download, rows, pitch, the memory each sample lies in, where the slab's
    first cell lies in it).  `planes`: the samples of one plane, [rows, cols] each ([members, rows, cols] for an ensemble)."""
    rows, cols = c["rows"], c["cols"]
    if c["form"] == "ensemble":                               # the members' planes, one behind the other, in one allocation
        base = GUARD + (0 if fault == "first-member-ignored" else c["first"] * rows * cols)
        mems = [np.concatenate([np.zeros(GUARD, np.float32), x.ravel(), np.zeros(GUARD, np.float32)]) for x in planes]
        return [(0, c["count"] * rows, cols, mems, base)]
    pitch = P.field_pitch(cols, c["pitch_pad"])
    beyond = np.float32(P.POISONS[c["poison_value"]] if c["poison"] else 0)          # fields are created zero-filled
    out, r0 = [], 0
    for n in P.slab_rows(rows, c["slabs"]):
        mems = []
        for x in planes:
            block = np.full((n + 2 * P.GHOST_ROWS, pitch), beyond, np.float32)
            block[P.GHOST_ROWS:P.GHOST_ROWS + n, :cols] = x[r0:r0 + n]
            mems.append(np.concatenate([np.full(GUARD, beyond, np.float32), block.ravel(), np.full(GUARD, beyond, np.float32)]))
        out.append((r0, n, pitch, mems, GUARD + P.GHOST_ROWS * pitch))
        r0 += n
    return out


def modelled(c, i, fault=None):
    """{name: array} of plane i of pinned example `c`: the raw accumulators and, under "result:<name>", the result planes,
    as the model gives them with `fault`; None without a sample since the last reset."""
    members = c["members"] if c["form"] == "ensemble" else None
    planes = P.plane_samples(c, i, members)
    if members is not None:
        outside = np.ones(members, bool)
        outside[c["first"]:c["first"] + c["count"]] = False
        for x in planes:
            x[outside] = np.float32(P.POISONS[c["poison_value"]])
    groups, cols = c["groups"], c["cols"]
    rule, rule0 = P.rule_of(c, i), P.rule_of(c, 0)
    out_rows = c["count"] * c["rows"] if members is not None else c["rows"]
    slabs = slab_memories(c, planes, fault)
    models = [Model(n * pitch, fault) for _, n, pitch, _, _ in slabs]
    samples = 0
    for k, stamp in enumerate(c["stamps"][:c["nsamples"]]):
        for m, (s, (_, n, pitch, mems, base)) in zip(models, enumerate(slabs)):
            r, w, p = faulty_scan(n, cols, pitch, fault)
            vec = P.scans(c)[s][3]
            row_at = np.arange(r)[:, None] * p
            for stored, src in visits(w, groups, vec, fault):
                read = base + row_at + src[None, :] - (p if fault == "row-above-read" else 0)
                m.add(mems[k][read], row_at + stored[None, :], stamp, rule, rule0, fault)
        samples += 1
        if c["reset"] and k == 1:
            models = [Model(n * pitch, fault, after_reset=True) for _, n, pitch, _, _ in slabs]
            samples = samples if fault == "reset-keeps-count" else 0
    out = {}
    for name in ref.raw_names(groups):
        full = np.zeros((out_rows, cols), getattr(models[0], name).dtype)
        for s, (m, (r0, n, pitch, _, _)) in enumerate(zip(models, slabs)):
            at = r0 - 1 if fault == "slab-row-off" and s > 0 else r0
            full[at:at + n] = getattr(m, name).reshape(n, pitch)[:, :cols]
        out[name] = full
    if samples == 0:
        return out
    n = np.float64(samples)
    with np.errstate(all="ignore"):
        if groups & ref.SUM:
            out["result:mean"] = (out["sum"] / n).astype(np.float32)
        if groups & ref.SUM and groups & ref.SQUARES:
            mean = out["sum"] / n
            d = out["squares"] / (n - 1 if fault == "n-1" else n) - mean * mean
            out["result:variance"] = (d if fault == "variance-unclamped" else np.where(d <= 0.0, 0.0, d)).astype(np.float32)
        if groups & ref.EXTREMES:
            out["result:min"], out["result:max"] = out["min"], out["max"]
        if groups & ref.CROSSINGS:
            count = out["set_count"]
            # (an IEEE f32 division of counts this small gives the bits of the f64 one; what a kernel that stays in f32
            # does is multiply by the reciprocal)
            occupancy = count.astype(np.float32) * (np.float32(1) / np.float32(n)) if fault == "occupancy-f32" else count.astype(np.float64) / n
            out["result:occupancy"] = occupancy.astype(np.float32)
            out["result:arrival"] = np.where(out["first_stamp"] == ref.NEVER, np.float32(-1.0), out["first_stamp"].astype(np.float32))
    return out


def referenced(c, i):
    """The same planes from time_stats_ref.Accumulators."""
    members = c["members"] if c["form"] == "ensemble" else None
    planes = P.plane_samples(c, i, members)
    if members is not None:
        planes = [x[c["first"]:c["first"] + c["count"]].reshape(-1, c["cols"]) for x in planes]
    acc = P.fresh_acc(c, planes[0].shape, i)
    for k, stamp in enumerate(c["stamps"][:c["nsamples"]]):
        acc.accumulate(planes[k], stamp)
        if c["reset"] and k == 1:
            acc = P.fresh_acc(c, planes[0].shape, i)
    out = {name: acc.raw(name) for name in ref.raw_names(c["groups"])}
    if acc.samples:
        out.update({"result:" + name: acc.result(name) for name in ref.result_names(c["groups"])})
    return out


def same_planes(a, b):
    return a.keys() == b.keys() and all(ref.same_bits(a[k], b[k]) for k in a)


@functools.lru_cache(maxsize=None)
def discrimination(n):
    """{fault: does pinned example `n` give other planes with it than the reference}; the model without a fault is held to
    the reference first."""
    c = P.EDGE_EXAMPLES[n]
    caught = {f: False for f in FAULTS}
    for i in range(P.planes_of(c)):
        true = referenced(c, i)
        got = modelled(c, i)
        assert same_planes(got, true), (n, i, [k for k in true if not ref.same_bits(got[k], true[k])])
        for fault in FAULTS:
            caught[fault] = caught[fault] or not same_planes(modelled(c, i, fault), true)
    return caught


@pytest.mark.parametrize("n", range(len(P.EDGE_EXAMPLES)))
def test_pinned_example_discriminates(n):
    caught = discrimination(n)
    assert any(caught.values()), P.EDGE_EXAMPLES[n]


def test_every_fault_is_caught_by_three_pinned_examples():
    catches = {f: [n for n in range(len(P.EDGE_EXAMPLES)) if discrimination(n)[f]] for f in FAULTS}
    assert all(len(v) >= 3 for v in catches.values()), {f: v for f, v in catches.items() if len(v) < 3}


# ---- the exact checks notice faults ------------------------------------------------------------------------------------------
def _finite_samples(shape, n, seed):
    rng = np.random.default_rng(seed)
    out = [(rng.standard_normal(shape) * 10.0 ** rng.integers(-30, 30, size=shape)).astype(np.float32) for _ in range(n)]
    out[0].flat[:3] = [0.3, 2.0 ** -130, 3.4028235e38]     # (one unit below a power of two is half a unit of it away)
    return out


@pytest.mark.parametrize("n", [1, 2, 5, 6])
def test_the_exact_checks_hold_the_restatement_and_notice_faults(n):
    samples = _finite_samples((7, 33), n, n)
    acc = ref.Accumulators((7, 33))
    for k, x in enumerate(samples):
        acc.accumulate(x, k)
    P.check_exact(samples, acc.sum, acc.squares, acc.result("mean"), "the restatement")
    twice = ref.Accumulators((7, 33))                      # one sample added twice
    for k, x in enumerate(samples + samples[-1:]):
        twice.accumulate(x, k)
    with pytest.raises(AssertionError, match="sum of cell"):
        P.check_exact(samples, twice.sum, None, None, "a sample added twice")
    with pytest.raises(AssertionError, match="squares of cell"):
        P.check_exact(samples, None, twice.squares, None, "a sample added twice")
    mean = acc.result("mean")
    for direction in (np.inf, -np.inf):                    # a mean one f32 unit off, in every cell in turn
        for cell in (0, 1, 2, 5, 230):
            off = mean.copy()
            with np.errstate(over="ignore"):
                off.flat[cell] = np.nextafter(mean.flat[cell], np.float32(direction))
            with pytest.raises(AssertionError, match="mean of cell"):
                P.check_exact(samples, None, None, off, "a mean one unit off")
    with np.errstate(all="ignore"):
        low = (acc.sum.astype(np.float32).astype(np.float64) / n).astype(np.float32)    # a sum kept in f32: caught where it differs
    if n > 1 and not ref.same_bits(low, mean):
        with pytest.raises(AssertionError):
            P.check_exact(samples, acc.sum.astype(np.float32).astype(np.float64), None, low, "a sum kept in f32")
