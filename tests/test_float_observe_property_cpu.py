"""The randomised GPU parity test of the float-valued observables (tests/test_gpu_float_observe_property.py) without a GPU:
its strategy draws legal cases of every family, form, factor class, region form, slab count and load path within the caps,
with at most a quarter of the drawn chains refusing; the vectorised references equal their literal twins on the small pinned
examples; the exact checks accept the references and notice a wrong sum; and the pinned examples discriminate: restatements
of the kernels with exactly one fault -- of a fold order, of an index, of what lies beside the plane in memory, of a rule --
each give another result than the reference on at least three pinned examples, and every pinned example tells at least one
of them from the reference."""
import collections
import functools

import numpy as np
import pytest

from . import change_ref, reduce_ref, regions_ref, summary_ref
from . import test_gpu_float_observe_property as P


# ---- the strategy ------------------------------------------------------------------------------------------------------------
def test_the_strategy_draws_legal_cases_of_every_kind():
    from hypothesis import HealthCheck, given, seed, settings

    seen = collections.Counter()
    chains = collections.Counter()

    def draw(c):
        slabs, refused = P.legal(c)
        family = c["family"]
        seen["draws"] += 1
        seen.update({("family", family), ("form", family, c["form"]), ("kind", c["kind"]), ("salt", c["salt"]), ("edges", c["edges"])})
        seen.update({("b", c["b_kind"])} if family == "change" else {})
        seen.update({("tail", c["cols"] > P.GROUP_COLS and c["cols"] % P.GROUP_COLS != 0, c["form"] == "ensemble")})
        if c["form"] == "ensemble":
            seen.update({("ragged", P.ragged((c["rows"], c["cols"]))), ("retire", c["retire"]), ("members", c["members"])})
            assert c["rows"] * c["cols"] <= P.MEMBER_CAP
            return
        seen.update({("slabs", slabs), ("poison", c["poison"]), ("poison value", c["poison_value"])})
        seen.update({("one-row slabs", True)} if slabs > 1 and P.shortest_slab(c["rows"], slabs) == 1 else {})
        assert c["rows"] * c["cols"] * c["nfields"] * (2 if family == "change" else 1) <= P.CELL_CAP
        if c["form"] == "fields":
            seen[("nfields", c["nfields"])] += 1
        if family == "reduce":
            seen.update({("factor class", P.factor_class(c["f"])), ("factor", c["f"])})
            seen.update({("tile columns", c["cols"] - P.tile_cols(c["f"]))} if abs(c["cols"] - P.tile_cols(c["f"])) <= 1 else {})
        if family == "regions":
            seen.update({("region form", P.region_form(c)), ("rh", c["rh"]), ("rw", c["rw"])})
        if family in ("reduce", "regions") and c["slabs"] > 1:
            chains[refused] += 1

    for family in P.FAMILIES:                                 # 2000 draws in all, as many of every family
        seed(20250301)(settings(max_examples=500, deadline=None, database=None, suppress_health_check=list(HealthCheck))(
            given(P.cases(family))(draw)))()
    assert seen["draws"] >= 1900, seen["draws"]
    want = ([("family", f) for f in P.FAMILIES] + [("form", f, form) for f in P.FAMILIES for form in P.FORMS[f]]
            + [("kind", k) for k in P.KINDS] + [("salt", s) for s in (0, 1, 2)] + [("edges", e) for e in (False, True)]
            + [("b", b) for b in P.B_KINDS] + [("tail", True, e) for e in (False, True)] + [("ragged", r) for r in (False, True)]
            + [("retire", r) for r in (False, True)] + [("members", m) for m in range(1, 7)] + [("slabs", s) for s in range(1, 6)]
            + [("poison", p) for p in (False, True)] + [("poison value", v) for v in (0, 1)] + [("one-row slabs", True)]
            + [("nfields", n) for n in (1, 2, 3, 4)] + [("factor class", k) for k in P.FACTOR_CLASSES]
            + [("tile columns", d) for d in (-1, 0, 1)]
            + [("region form", r) for r in ("narrow", "exactly 256", "wide", "wider than 2048")]
            + [("rh", h) for h in P.REGION_HEIGHTS] + [("rw", w) for w in P.REGION_WIDTHS])
    rare = {k: seen[k] for k in want if seen[k] < 10}
    assert not rare, rare
    # every factor 2 .. 64 can be drawn (the classes hold them all), and the small ones and ten of the others were
    assert sorted(f for fs in P.FACTOR_CLASSES.values() for f in fs) == list(range(2, 65))
    assert all(seen[("factor", f)] > 0 for f in range(2, 9)) and sum(1 for f in range(9, 65) if seen[("factor", f)]) >= 10
    # a chain that must refuse: at most a quarter of the reduce and region draws with more than one slab
    assert chains[True] >= 20 and chains[True] + chains[False] >= 200 and chains[True] * 4 <= chains[True] + chains[False], chains


def test_the_kernels_units_are_restated():
    assert (P.WAVES, P.LANE_COLS, P.BLOCK_COLS, P.SUM_UNROLL, P.GROUP_COLS, P.RED_ROWS) == (4, 4, 256, 8, 2048, 8)
    # W(f) = npix(f) * f of gs_launch_reduce: the widths its comments name
    assert [P.tile_cols(f) for f in (3, 5, 6, 7, 8, 10, 16, 64)] == [1020, 1020, 1008, 1008, 1024, 1000, 1024, 1024]
    assert all(P.npix(f) % 4 == 0 and P.npix(f) * (f | 1) <= 1200 for f in range(2, 65) if f not in (2, 4))
    assert 4101 in P.COLS and 2053 in P.COLS and {4 * m + d for m in (1, 2) for d in (-1, 0, 1)} <= set(P.ROWS)
    assert {7, 8, 9, 15, 16, 17, 31, 32, 33} <= set(P.ROWS)


def test_the_pinned_examples_are_legal_and_cover_the_forms():
    counts = collections.Counter()
    for c in P.EDGE_EXAMPLES:
        P.legal(c)
        counts.update(P.counts_of(c))
    need = ([f"{f} form {form}" for f in P.FAMILIES for form in P.FORMS[f]] + [f"slabs {s}" for s in range(1, 6)] + P.FAMILIES
            + ["ensemble load path ragged", "ensemble load path 16 bytes", "poisoned", "one-row slabs", "refused chains",
               "retired members", "beyond 2048 with a ragged tail, ragged", "beyond 2048 with a ragged tail, 16 bytes",
               "region form wider than 2048", "region form narrow", "region form exactly 256", "region form wide"]
            + [f"factor {f}" for f in (2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 17, 33, 63, 64)]
            + ["factor class " + k for k in P.FACTOR_CLASSES])
    assert all(counts[k] > 0 for k in need), [k for k in need if not counts[k]]
    for shape in P.ENSEMBLE_SHAPES:
        assert P.ragged(shape) and any((c["rows"], c["cols"]) == shape for c in P.EDGE_EXAMPLES if c["family"] == "summary")
        assert any((c["rows"], c["cols"]) == shape for c in P.EDGE_EXAMPLES if c["family"] == "change")


# ---- the references ----------------------------------------------------------------------------------------------------------
def first_planes(c):
    """(a, b) of a pinned example's first plane (an ensemble: species 0 of its first member of the range; b: comparisons)."""
    if c["form"] == "ensemble":
        if c["family"] == "change":
            a, b = P.member_pairs(c)
            return a[0, c["first"]], b[0, c["first"]]
        return P.member_planes(c)[0, c["first"]], None
    planes, others = P.field_inputs(c)
    return planes[0], (None if others is None else (planes[0] if others[0] is None else others[0]))


@pytest.mark.parametrize("n", [n for n, c in enumerate(P.EDGE_EXAMPLES) if c["rows"] * c["cols"] <= 3000])
def test_references_equal_their_literal_twins(n):
    c = P.EDGE_EXAMPLES[n]
    a, b = first_planes(c)
    if c["family"] == "summary":
        assert summary_ref.same(summary_ref.summary(a), summary_ref.literal(a))
    elif c["family"] == "change":
        assert change_ref.same(change_ref.change(a, b), change_ref.literal(a, b))
    elif c["family"] == "reduce":
        assert reduce_ref.same_bits(reduce_ref.reduce(a, c["f"]), reduce_ref.literal(a, c["f"]))
    else:
        want = regions_ref.summaries(a, P.region_of(c))
        for at, crop in regions_ref.crops(a, P.region_of(c)):
            assert summary_ref.same(want[at], summary_ref.literal(crop)), at


def test_the_exact_checks_accept_the_references_and_notice_a_wrong_sum():
    a, b = change_ref.order_sensitive((9, 261), 3)
    s, d = summary_ref.summary(a), change_ref.change(a, b)
    P.assert_summary_exact(s, a, "summary")
    P.assert_change_exact(d, a, b, "change")
    with pytest.raises(AssertionError):
        P.assert_summary_exact(dict(s, sum=s["sum"] + float(a[0, 0])), a, "a cell twice")
    with pytest.raises(AssertionError):
        P.assert_change_exact(dict(d, sum_abs=d["sum_abs"] - abs(float(a[8, 260]) - float(b[8, 260]))), a, b, "a cell dropped")
    assert P.sum_bound(1, 5.0) == 0.0 and P.sum_bound(3, 1.0) == 2 * 2.0 ** -53 / (1 - 2 * 2.0 ** -53)
    for f, shape, seed in ((3, (10, 31), 1), (12, (25, 40), 2), (2, (5, 9), 3)):
        plane = reduce_ref.special_plane(shape, seed)
        image = reduce_ref.reduce(plane, f)
        P.assert_reduce_exact(image, plane, f, f"f = {f}")
        plain = P.stress_fields(shape, seed)[0]               # (nothing cancels: the bound is far below a unit of f32)
        wrong = reduce_ref.reduce(plain, f)
        P.assert_reduce_exact(wrong, plain, f, f"f = {f}")
        wrong[-1, -1] = np.nextafter(wrong[-1, -1], np.float32(np.inf))
        with pytest.raises(AssertionError):
            P.assert_reduce_exact(wrong, plain, f, f"f = {f}, one pixel one unit off")
    tiny = np.full((4, 4), 1e-45, np.float32)                 # sub-normal means: the unit in the last place is 2^-149
    P.assert_reduce_exact(reduce_ref.reduce(tiny, 2), tiny, 2, "sub-normal pixels")
    ints = P.scaled_ints(np.array([1e-45, -1e-45, 1.0, 3.4028235e38, 0.0, 1.1754944e-38], np.float32))
    assert ints == [1, -1, 1 << 149, (2 ** 24 - 1) << (104 + 149), 0, 1 << 23]


# ---- the pinned examples discriminate -------------------------------------------------------------------------------------
# A single fault is a restatement of an observable with exactly one defect.  It sees what the device sees: the plane, what
# lies right of every row's last cell (`right`: pitch padding; in an ensemble, or where the pitch is the width, the next
# row's first cell) and what lies below the last row (`below`: a ghost row; the next member's first row).
FOLD_FAULTS = ["ascending",             # plain ascending column order in a row
               "adjacent-pairs",        # the lane combine done as adjacent pairs instead of halves
               "rows-pairwise",         # rows folded pairwise
               "no-last-column",        # the last column dropped when cols % 4 != 0
               "no-last-block",         # the last block of 256 dropped
               "no-group-tail",         # the columns after a full 2048 group dropped
               "pad-read",              # one pad column read
               "ghost-read",            # one ghost row read
               "nonfinite-uncounted",   # a non-finite cell added as 0 but not counted
               "ftz"]                   # sub-normals flushed
CHANGE_FAULTS = ["abs-f32",             # |d| taken in f32
                 "differing-by-value"]  # differing by value instead of by bits
REGION_FAULTS = ["border-lane", "border-row",   # a region border moved by one lane (4 columns) or by one row
                 "ragged-as-full"]      # a ragged last region sized as a full one
REDUCE_FAULTS = ["f2-divisor",          # an edge block divided by f * f instead of nr * nc
                 "rows-descending",     # a block's row partials added in descending order
                 "second-batch-skipped",  # the second batch of rows of a block with f > 8 skipped
                 "next-tile-pixel",     # a tile's last pixel taken from the next tile
                 "pad-read", "ghost-read", "ftz"]
FAULTS = {"summary": FOLD_FAULTS, "change": FOLD_FAULTS + CHANGE_FAULTS, "regions": FOLD_FAULTS + REGION_FAULTS, "reduce": REDUCE_FAULTS}


def flushed(a):
    tiny = (a.view(np.uint32) & np.uint32(0x7f800000)) == 0
    return np.where(tiny, np.copysign(np.float32(0), a), a).astype(np.float32)


def beside(fault, a, right, below):
    """Plane `a` with what lies beside it taken for cells of its own."""
    if fault == "pad-read" and right is not None:
        return np.concatenate([a, right[:, None]], axis=1)
    if fault == "ghost-read" and below is not None:
        return np.concatenate([a, below[None, :]], axis=0)
    return a


def cut(a, fault):
    cols = a.shape[1]
    if fault == "no-last-column" and cols % P.LANE_COLS:
        return a[:, :cols - 1]
    if fault == "no-last-block":
        return a[:, :(cols - 1) // P.BLOCK_COLS * P.BLOCK_COLS]
    if fault == "no-group-tail" and cols > P.GROUP_COLS:
        return a[:, :cols // P.GROUP_COLS * P.GROUP_COLS]
    return a


def fold(d, fault):
    """The sum of the f64 terms d[rows, cols] in the definition's order, but for `fault`."""
    rows, cols = d.shape
    if fault == "ascending":
        parts = np.cumsum(np.concatenate([np.zeros((rows, 1)), d], axis=1), axis=1)[:, -1]
    else:
        blocks = max(1, -(-cols // P.BLOCK_COLS))
        x = np.zeros((rows, blocks * P.BLOCK_COLS))
        x[:, :cols] = d
        x = x.reshape(rows, blocks, 64, P.LANE_COLS)
        s = np.zeros((rows, 64))
        for k in range(blocks):
            for j in range(P.LANE_COLS):
                s = s + x[:, k, :, j]
        while s.shape[1] > 1:
            h = s.shape[1] // 2
            s = (s[:, 0::2] + s[:, 1::2]) if fault == "adjacent-pairs" else (s[:, :h] + s[:, h:])
        parts = s[:, 0]
    if fault == "rows-pairwise":
        p = parts
        while p.size > 1:
            even = p.size // 2 * 2
            p = np.concatenate([p[0:even:2] + p[1:even:2], p[even:]])
        return float(p[0])
    return float(np.cumsum(np.concatenate([[0.0], parts]))[-1])


def summary_with(a, fault=None, right=None, below=None):
    a = cut(beside(fault, np.asarray(a, np.float32), right, below), fault)
    a = flushed(a) if fault == "ftz" else a
    fin = np.isfinite(a)
    d = np.where(fin, a.astype(np.float64), 0.0)
    finite = a[fin]
    return {"sum": fold(d, fault), "sum_sq": fold(d * d, fault), "min": float(finite.min()) if finite.size else np.inf,
            "max": float(finite.max()) if finite.size else -np.inf,
            "nonfinite": 0 if fault == "nonfinite-uncounted" else int(a.size - np.count_nonzero(fin))}


def change_with(a, b, fault=None, right=(None, None), below=(None, None)):
    a = cut(beside(fault, np.asarray(a, np.float32), right[0], below[0]), fault)
    b = cut(beside(fault, np.asarray(b, np.float32), right[1], below[1]), fault)
    if fault == "ftz":
        a, b = flushed(a), flushed(b)
    fin = np.isfinite(a) & np.isfinite(b)
    with np.errstate(all="ignore"):
        d = np.where(fin, a.astype(np.float64) - b.astype(np.float64), 0.0)
        mag = np.where(fin, np.abs(a - b).astype(np.float64), 0.0) if fault == "abs-f32" else np.abs(d)
        unlike = (a != b) if fault == "differing-by-value" else (a.view(np.uint32) != b.view(np.uint32))
    return {"sum_abs": fold(mag, fault), "sum_sq": fold(d * d, fault), "max_abs": float(mag.max()) if mag.size else 0.0,
            "differing": int(np.count_nonzero(unlike)),
            "nonfinite": 0 if fault == "nonfinite-uncounted" else int(a.size - np.count_nonzero(fin))}


def regions_with(a, region, fault=None, right=None, below=None):
    """((RR, RC) records, sizes) of the regional summaries with `fault`."""
    a = beside(fault, np.asarray(a, np.float32), right, below)
    rows, cols = a.shape
    rh, rw = region
    rr, rc = regions_ref.grid(a.shape, region)
    row_edges = [min(i * rh + (1 if fault == "border-row" and 0 < i < rr else 0), rows) for i in range(rr)] + [rows]
    col_edges = [min(j * rw + (P.LANE_COLS if fault == "border-lane" and 0 < j < rc else 0), cols) for j in range(rc)] + [cols]
    out = np.zeros((rr, rc), regions_ref.SUMMARY_DTYPE)
    for i in range(rr):
        for j in range(rc):
            s = summary_with(a[row_edges[i]:row_edges[i + 1], col_edges[j]:col_edges[j + 1]],
                             fault if fault in FOLD_FAULTS and fault not in ("pad-read", "ghost-read") else None)
            out[i, j] = tuple(s[f] for f in summary_ref.FIELDS)
    sizes = np.full((rr, rc), rh * rw, np.int64) if fault == "ragged-as-full" else regions_ref.sizes(a.shape, region)
    return out, sizes


def reduce_with(a, f, fault=None, right=None, below=None):
    a = np.asarray(a, np.float32)
    a = flushed(a) if fault == "ftz" else a
    rows, cols = a.shape
    orows, ocols = reduce_ref.shape(rows, cols, f)
    x = np.zeros((orows * f + 1, ocols * f + 1), np.float64)
    x[:rows, :cols] = a
    if fault == "pad-read" and right is not None and cols % f:       # the ragged last block reads on
        x[:rows, cols] = right
    if fault == "ghost-read" and below is not None and rows % f:
        x[rows, :cols] = below
    x = x[:orows * f, :ocols * f].reshape(orows, f, ocols, f)
    nr = np.minimum(f, rows - np.arange(orows) * f)
    nc = np.minimum(f, cols - np.arange(ocols) * f)
    order = range(f - 1, -1, -1) if fault == "rows-descending" else range(f)
    with np.errstate(all="ignore"):
        total = np.zeros((orows, ocols), np.float64)
        for i in order:
            if fault == "second-batch-skipped" and P.RED_ROWS <= i < 2 * P.RED_ROWS:
                continue
            p = np.zeros((orows, ocols), np.float64)
            for j in range(f):
                p = p + x[:, i, :, j]
            total = total + p
        count = np.full((orows, ocols), float(f * f)) if fault == "f2-divisor" else (nr[:, None] * nc[None, :]).astype(np.float64)
        out = (total / count).astype(np.float32)
    if fault == "next-tile-pixel":
        for C in range(P.npix(f) - 1, ocols - 1, P.npix(f)):
            out[:, C] = out[:, C + 1]
    return out


def views_of(c):
    """What pinned example `c` shows of its first plane: (a, b, (right of a, of b), (below a, below b))."""
    rows, cols = c["rows"], c["cols"]
    if c["form"] == "ensemble":
        planes = P.member_pairs(c) if c["family"] == "change" else (P.member_planes(c), None)
        inside = range(c["first"], c["first"] + c["count"])
        m = next((i for i in inside if c["retire"] and c["retired"][i]), c["first"])
        out = []
        for x in planes:
            if x is None:
                out.append((None, None, None))
                continue
            a = x[0, m]
            # a member's rows lie `cols` floats apart: right of a row's last cell lies the next row's first, below the last
            # row the next member -- unknown here where that member advances
            known = m + 1 < c["members"] and (m + 1 not in inside or not c["retire"] or c["retired"][m + 1])
            below = x[0, m + 1][0] if known else None
            right = np.concatenate([a[1:, 0], below[:1] if known else a[:1, 0]])
            out.append((a, right, below))
        return out[0][0], out[1][0], (out[0][1], out[1][1]), (out[0][2], out[1][2])
    a, b = first_planes(c)
    pitch = -(-cols // 64) * 64                                       # a field's pitch is a multiple of 64
    sides = []
    for plane, sign in ((a, 1.0), (b, -1.0)):
        if plane is None:
            sides.append((None, None))
            continue
        beyond = np.float32(sign * P.POISONS[c["poison_value"]]) if c["poison"] else np.float32(0)   # planes are created zero-filled
        below = np.full(cols, beyond, np.float32)
        sides.append((np.full(rows, beyond, np.float32) if pitch > cols else np.concatenate([plane[1:, 0], below[:1]]), below))
    if c["family"] == "change" and c["b_kind"] == "same":             # one field on both sides
        sides[1] = sides[0]
    return a, b, (sides[0][0], sides[1][0]), (sides[0][1], sides[1][1])


def observable(c, fault, a, b, right, below):
    family = c["family"]
    if family == "summary":
        return summary_with(a, fault, right[0], below[0])
    if family == "change":
        return change_with(a, b, fault, right, below)
    if family == "reduce":
        return reduce_with(a, c["f"], fault, right[0], below[0])
    return regions_with(a, P.region_of(c), fault, right[0], below[0])


def same_as_reference(c, got, a, b):
    family = c["family"]
    if family == "summary":
        return summary_ref.same(got, summary_ref.summary(a))
    if family == "change":
        return change_ref.same(got, change_ref.change(a, b))
    if family == "reduce":
        return reduce_ref.same_bits(got, reduce_ref.reduce(a, c["f"]))
    region = P.region_of(c)
    want = regions_ref.summaries(a, region)
    return got[0].shape == want.shape and regions_ref.same_summaries(got[0], want) and np.array_equal(got[1], regions_ref.sizes(a.shape, region))


@functools.lru_cache(maxsize=None)
def discrimination(n):
    """{fault: does pinned example `n` give another result with it than without} for the faults of its family; the
    restatement without a fault is held to the reference first."""
    c = P.EDGE_EXAMPLES[n]
    a, b, right, below = views_of(c)
    assert same_as_reference(c, observable(c, None, a, b, right, below), a, b), n
    return {fault: not same_as_reference(c, observable(c, fault, a, b, right, below), a, b) for fault in FAULTS[c["family"]]}


@pytest.mark.parametrize("n", range(len(P.EDGE_EXAMPLES)))
def test_pinned_example_discriminates(n):
    caught = discrimination(n)
    assert any(caught.values()), P.EDGE_EXAMPLES[n]


@pytest.mark.parametrize("family", P.FAMILIES)
def test_every_fault_is_caught_by_three_pinned_examples(family):
    examples = [n for n, c in enumerate(P.EDGE_EXAMPLES) if c["family"] == family]
    catches = {f: [n for n in examples if discrimination(n)[f]] for f in FAULTS[family]}
    assert all(len(v) >= 3 for v in catches.values()), {f: v for f, v in catches.items() if len(v) < 3}
