"""The randomised GPU parity test of the observables (tests/test_gpu_observe_property.py) without a GPU: its strategy draws
legal cases of every kind within the caps; the `seams` and `lane_runs` layouts (tests/observe_cases.py) are what they claim,
and the references agree with scipy and with their literal loops on them; and the pinned examples discriminate: for every
observable, restatements with exactly one defect -- of a kernel's index arithmetic, of the host's seam merge, of the set
rule, of what lies beside the plane in memory -- each give another result than the reference on at least three pinned
examples, and every pinned example tells at least one of them from the reference."""
import collections
import functools

import numpy as np
import pytest

from . import component_list_ref, components_ref, corr_ref, hist_ref, morph_ref
from . import observe_cases as O
from . import test_gpu_observe_property as P


# ---- the strategy ------------------------------------------------------------------------------------------------------------
def test_the_strategy_draws_legal_cases_of_every_kind():
    from hypothesis import HealthCheck, given, seed, settings

    seen = collections.Counter()
    detours = collections.Counter()

    @seed(20240229)
    @settings(max_examples=2000, deadline=None, database=None, suppress_health_check=list(HealthCheck))
    @given(P.cases())
    def draw(c):
        slabs, max_lag, detour = P.legal(c)
        seen["draws"] += 1
        seen.update({("family", c["family"]), ("kind", c["kind"]), ("form", c["form"]), ("conn", c["conn"]),
                     ("nt", len(c["thresholds"])), ("lag", c["max_lag"]), ("above", c["above"]), ("min_size", c["min_size"]),
                     ("bins", c["bins"]), ("range", c["range"])})
        seen.update(("threshold", repr(t)) for t in c["thresholds"])
        if c["form"] == "ensemble":
            seen.update({("ragged", P.ragged((c["rows"], c["cols"]))), ("retire", c["retire"]), ("fence", c["fence"]),
                         ("members", c["members"])})
            assert c["rows"] * c["cols"] <= P.MEMBER_CAP
        else:
            seen.update({("slabs", slabs), ("poison", c["poison"])})
            seen.update({("one-row slabs", True)} if slabs > 1 and P.shortest_slab(c["rows"], slabs) == 1 else {})
            assert c["rows"] * c["cols"] * c["nfields"] <= P.CELL_CAP
            if c["form"] == "fields":
                seen[("nfields", c["nfields"])] += 1
            if c["family"] == "correlation" and c["slabs"] > 1:
                detours[detour] += 1
                assert not detour or 1 <= max_lag < c["max_lag"]

    draw()
    assert seen["draws"] >= 1900, seen["draws"]
    want = ([("family", f) for f in P.FAMILIES] + [("kind", k) for k in O.KINDS] + [("form", f) for f in P.FORMS]
            + [("conn", 4), ("conn", 8)] + [("nt", n) for n in (1, 2, 3, 4)] + [("lag", lag) for lag in P.MAX_LAGS]
            + [("above", a) for a in (False, True)] + [("min_size", m) for m in range(len(P.MIN_SIZES))]
            + [("bins", b) for b in P.BINS] + [("range", r) for r in range(len(P.RANGES))]
            + [("threshold", repr(t)) for t in P.THRESHOLDS] + [("ragged", r) for r in (False, True)]
            + [("retire", r) for r in (False, True)] + [("fence", r) for r in (False, True)] + [("members", m) for m in range(1, 7)]
            + [("slabs", s) for s in range(1, 6)] + [("poison", p) for p in (False, True)] + [("one-row slabs", True)]
            + [("nfields", n) for n in (1, 2, 3, 4)])
    rare = {k: seen[k] for k in want if seen[k] < 20}
    assert not rare, rare
    # a chain that must refuse its lag: at most a quarter of the correlation draws with more than one slab
    assert detours[True] + detours[False] >= 100 and detours[True] * 4 <= detours[True] + detours[False], detours


def test_the_pinned_examples_are_legal_and_cover_the_forms():
    counts = collections.Counter()
    for c in P.EDGE_EXAMPLES:
        P.legal(c)
        counts.update(P.counts_of(c))
    need = (["form " + f for f in P.FORMS] + [f"slabs {s}" for s in range(1, 6)] + P.FAMILIES
            + ["ensemble load path ragged", "ensemble load path 16 bytes", "poisoned", "one-row slabs", "refused lags", "retired members"])
    assert all(counts[k] > 0 for k in need), counts
    for shape in P.ENSEMBLE_SHAPES:
        assert P.ragged(shape) and any((c["rows"], c["cols"]) == shape for c in P.EDGE_EXAMPLES)
    empties = [c for c in P.EDGE_EXAMPLES if c["kind"] == "empty" and c["poison"]]
    assert {(c["family"], c["slabs"]) for c in empties} >= {(f, s) for f in P.FAMILIES[:4] for s in (2, 3)}


def test_the_seam_helper():
    assert O.seam_rows(5, 5) == [1, 2, 3, 4] and O.seam_rows(50, 3) == [16, 33] and O.seam_rows(7, 1) == []
    assert O.seam_rows(2, 5) == [1]                      # more slabs than rows: row 0 is no seam
    assert (O.TILE_ROWS, O.TILE_COLS, O.QUAD_ROWS, O.PAIR_ROWS, O.STRIP_COLS, O.WORD_COLS, O.LANE_COLS) == (16, 256, 32, 512, 256, 64, 4)


# ---- the new layouts ---------------------------------------------------------------------------------------------------------
LAYOUT_SHAPES = [(8, 8), (17, 65), (33, 259), (66, 515), (5, 1027)]


@pytest.mark.parametrize("shape", LAYOUT_SHAPES + [(513, 9), (1026, 8)])
@pytest.mark.parametrize("slabs", [1, 3, 5])
def test_seams_have_a_set_cell_and_a_gap_on_every_line(shape, slabs):
    rows, cols = shape
    bits = O.seams(shape, np.random.default_rng(rows + slabs), slabs)
    assert bits.dtype == np.bool_ and bits.shape == shape
    line_rows, line_cols = O.seam_lines(shape, slabs)
    for m in range(1, rows // O.TILE_ROWS + 1):
        assert all(r in line_rows for r in (m * O.TILE_ROWS - 1, m * O.TILE_ROWS) if r < rows)
    for m in range(1, rows // O.QUAD_ROWS + 1):
        assert all(r in line_rows for r in (m * O.QUAD_ROWS - 1, m * O.QUAD_ROWS, m * O.QUAD_ROWS + 1) if r < rows)
    for m in range(1, rows // O.PAIR_ROWS + 1):
        assert all(r in line_rows for r in (m * O.PAIR_ROWS - 1, m * O.PAIR_ROWS) if r < rows)
    for i in range(1, min(slabs, rows)):
        assert i * rows // min(slabs, rows) in line_rows and i * rows // min(slabs, rows) - 1 in line_rows
    for m in range(1, cols // O.WORD_COLS + 1):
        assert all(x in line_cols for x in (m * O.WORD_COLS - 1, m * O.WORD_COLS) if x < cols)
    for m in range(1, cols // O.STRIP_COLS + 1):
        assert all(x in line_cols for x in (m * O.STRIP_COLS - 1, m * O.STRIP_COLS, m * O.STRIP_COLS + 1) if x < cols)
    assert O.seams_are_mixed(bits, line_rows, line_cols)
    for r in line_rows:
        assert cols < 8 or (bits[r].any() and not bits[r].all())
    for x in line_cols:
        assert rows < 8 or (bits[:, x].any() and not bits[:, x].all())


@pytest.mark.parametrize("shape", [(33, 515), (48, 259)])
def test_lane_runs_hold_every_pattern_beside_full_lanes(shape):
    bits = O.lane_runs(shape, np.random.default_rng(shape[1]))
    assert bits.dtype == np.bool_ and bits.shape == shape
    p = O.lane_patterns(bits[0::4])                       # the rows drawn per lane
    assert set(p.ravel().tolist()) == set(range(16))
    after_full = p[:, 1:][p[:, :-1] == 15]
    # a run that comes out of a full lane and ends in column j of the next: patterns 1, 3, 7, and a full lane before a gap
    assert {1, 3, 7} <= set(after_full.tolist()) and any(int(x) % 2 == 0 for x in after_full.tolist())
    before_full = p[:, :-1][p[:, 1:] == 15]
    assert {8, 12, 14} <= set(before_full.tolist())      # ... and one that begins in column j and runs into a full lane
    assert (p == 15).mean() > 0.4                         # long stretches of full lanes
    # the rows between: the row above moved one column right, then one left
    assert (bits[1, 1:] == bits[0, :-1]).all() and (bits[3, :-1] == bits[2, 1:]).all()
    eight, four = components_ref.sizes(bits, 0.5, True, 8), components_ref.sizes(bits, 0.5, True, 4)
    assert len(eight) < len(four)                         # some runs meet the row above across a corner only


def _scipy_counters(bits, conn):
    from scipy import ndimage

    lab, n = ndimage.label(bits, ndimage.generate_binary_structure(2, 1 if conn == 4 else 2))
    sizes = np.bincount(lab.ravel())[1:]
    out = np.zeros(35, np.uint64)
    if n:
        out[0], out[1], out[2] = n, sizes.sum(), sizes.max()
        for x in sizes:
            out[3 + min(int(x).bit_length() - 1, 31)] += np.uint64(1)
    return out


@pytest.mark.parametrize("kind", ["seams", "lane_runs"])
@pytest.mark.parametrize("shape", [(1, 1), (2, 9), (17, 65), (33, 259)])
def test_references_agree_on_the_new_layouts(kind, shape):
    for seed, (t, above) in enumerate(((0.3, True), (2.0 ** -130, False), (0.0, True))):
        a = O.plane(kind, shape, t, above, seed, slabs=3)
        bits = morph_ref.set_cells(a, t, above)
        for conn in (4, 8):
            assert np.array_equal(components_ref.counters(a, t, above, conn), _scipy_counters(bits, conn))
            rec = component_list_ref.records(a, t, above, conn)
            assert np.array_equal(component_list_ref.counters(rec), _scipy_counters(bits, conn))
        if shape[0] * shape[1] <= 17 * 65:
            assert np.array_equal(corr_ref.pairs(a, t, above, 5), corr_ref.literal(a, t, above, 5))
            assert np.array_equal(morph_ref.quads(a, t, above), morph_ref.literal(a, t, above))
            assert np.array_equal(component_list_ref.records(a, t, above, 8, 2), component_list_ref.literal(a, t, above, 8, 2))
        span = (-2.0, 1.0)
        if a.size <= 17 * 65:
            assert np.array_equal(hist_ref.histogram(a, *span, 255), hist_ref.literal(a, *span, 255))


def test_values_carry_the_pattern():
    rng = np.random.default_rng(3)
    bits = rng.random((9, 31)) < 0.5
    for t in P.THRESHOLDS:
        for above in (False, True):
            a = O.values_of(bits, t, above, np.random.default_rng(1), special=False)
            possible = not (np.isinf(t) and (t > 0) == above)     # nothing is above +inf or below -inf
            assert (morph_ref.set_cells(a, t, above) == (bits if possible else np.zeros_like(bits))).all(), (t, above)
            odd = O.values_of(bits, t, above, np.random.default_rng(1))
            assert np.isnan(odd).any() and (odd == np.float32(t)).any() and int((odd.view(np.uint32) != a.view(np.uint32)).sum()) <= 17
    for kind in ("full", "empty", "one-set", "one-unset"):
        a = O.plane(kind, (6, 7), 0.3, True, 5, at="se")
        want = {"full": 42, "empty": 0, "one-set": 1, "one-unset": 41}[kind]
        assert int(morph_ref.set_cells(a, 0.3, True).sum()) == want
    assert morph_ref.set_cells(O.plane("one-set", (6, 7), 0.3, False, 5, at="se"), 0.3, False)[5, 6]


# ---- the pinned examples discriminate -------------------------------------------------------------------------------------
# A single fault is a restatement of an observable with exactly one defect.  It sees what the device sees: the plane, what
# lies right of every row's last cell (`right`: pitch padding; in an ensemble the next row's first cell), what lies below the
# last row (`below`: a ghost row; the next member's first row), and the slabs' first rows.
RULE_FAULTS = [">=",              # a cell equal to the threshold is set
               "nan-below",       # NaN is set under the "below" sense
               "ftz"]             # sub-normal cells are flushed to zero before the comparison
BESIDE_FAULTS = ["right-seen",    # the cell right of a row's last one (column `cols`) is taken for a cell of the plane
                 "below-seen"]    # the row below the last one is
COMPONENT_FAULTS = ["no-tile-column",     # no union across a tile's first column (c % 256 == 0)
                    "no-tile-row",        # no union across a tile's first row (r % 16 == 0)
                    "no-border-diagonal",  # under 8-connectivity, the diagonal unions across a tile border dropped
                    "diagonal-under-4",   # a diagonal union made under 4-connectivity
                    "row-wrap",           # (r, cols - 1) and (r + 1, 0) treated as neighbours
                    "no-seam-merge",      # no merge across a slab seam
                    "no-seam-diagonal"]   # the seam merge blind to diagonals under 8-connectivity
LIST_FAULTS = ["last-piece-first-cell",   # a merged record keeps one slab's first cell (the last piece's), not the smallest
               "first-piece-box",         # a merged record keeps its first slab's box
               "local-rows",              # a merged record's rows are local to the slab
               "min-size-before-merge",   # min_size applied before the seam merge
               "merged-last"]             # the merged list left unsorted: merged records follow the others
PAIR_FAULTS = ["row-wrap",                # pairs along a row wrap from its end to the next row's start
               "lag+1",                   # lag d counted as d + 1
               "no-unit-row",             # pairs across a unit's first row (r % 512 == 0) dropped in directions 1..3
               "no-strip",                # pairs whose cells lie in different 256-column strips dropped
               "no-word-carry",           # ... in different 64-column words, at lags of a word or more
               "no-slab-row"]             # pairs across a slab's first row dropped
QUAD_FAULTS = ["shared-row-twice",        # the quad row shared by two units (q % 32 == 0) counted twice
               "shared-row-never",        # ... not counted at all
               "no-right-ring", "no-bottom-ring",   # the padding ring missing on one side
               "qd-q2"]                   # QD and Q2 exchanged
BIN_FAULTS = ["hi-above",                 # x == hi counted above
              "nan-below-range",          # NaN counted below
              "last-block",               # the last partial block of 256 columns skipped
              "f64-bin",                  # the bin formed in f64
              "ftz", "right-seen"]
FAULTS = {"morphology": RULE_FAULTS + BESIDE_FAULTS + QUAD_FAULTS,
          "correlation": RULE_FAULTS + BESIDE_FAULTS + PAIR_FAULTS,
          "components": RULE_FAULTS + BESIDE_FAULTS + COMPONENT_FAULTS,
          "component_list": RULE_FAULTS + BESIDE_FAULTS + COMPONENT_FAULTS + LIST_FAULTS,
          "histogram": BIN_FAULTS}


def flushed(a):
    tiny = (a.view(np.uint32) & np.uint32(0x7f800000)) == 0
    return np.where(tiny, np.copysign(np.float32(0), a), a).astype(np.float32)


def faulty_bits(fault, a, t, above):
    """The set cells of plane `a` under the set rule with `fault` (any other: the rule itself)."""
    a, t = np.asarray(a, np.float32), np.float32(t)
    if fault == "ftz":
        a = flushed(a)
    with np.errstate(invalid="ignore"):
        if fault == ">=":
            return (a >= t) if above else (a <= t)
        bits = (a > t) if above else (a < t)
    if fault == "nan-below" and not above:
        bits = bits | np.isnan(a)
    return bits


def edges_of(bits, conn):
    """The unions of a labelling as {name: (keep, r, c, r2, c2)}: every pair of set neighbours, by direction."""
    rows, cols = bits.shape
    rr, cc = np.mgrid[0:rows, 0:cols]
    out = {}
    for name, (dr, dc) in (("h", (0, 1)), ("v", (1, 0)), ("d", (1, 1)), ("a", (1, -1))):
        if name in "da" and conn == 4:
            continue
        top = (slice(0, rows - dr), slice(max(0, -dc), cols - max(0, dc)))
        low = (slice(dr, rows), slice(max(0, dc), cols + min(0, dc)))
        both = bits[top] & bits[low]
        out[name] = (rr[top][both], cc[top][both], rr[low][both], cc[low][both])
    return out


def components_of(bits, conn, fault=None, seams=()):
    """(flat indices of the set cells, their component numbers) under the unions that `fault` leaves or adds."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    rows, cols = bits.shape
    seams = np.asarray(sorted(seams), np.int64)
    e = edges_of(bits, 8 if fault == "diagonal-under-4" else conn)
    if fault == "diagonal-under-4" and conn == 4:
        e.pop("a")
    elif fault == "diagonal-under-4":
        return components_of(bits, conn, None, seams)
    pa, pb = [], []
    for name, (r, c, r2, c2) in e.items():
        tile_row = (r // O.TILE_ROWS) != (r2 // O.TILE_ROWS)
        tile_col = (c // O.TILE_COLS) != (c2 // O.TILE_COLS)
        seam = np.searchsorted(seams, r, side="right") != np.searchsorted(seams, r2, side="right")
        keep = np.ones(r.shape, bool)
        if fault == "no-tile-column":
            keep = ~(tile_col & ~tile_row)
        elif fault == "no-tile-row":
            keep = ~(tile_row & ~tile_col)
        elif fault == "no-border-diagonal" and name in "da":
            keep = ~(tile_row | tile_col)
        elif fault == "no-seam-merge":
            keep = ~seam
        elif fault == "no-seam-diagonal" and name in "da":
            keep = ~seam
        pa.append((r * cols + c)[keep])
        pb.append((r2 * cols + c2)[keep])
    if fault == "row-wrap" and rows > 1:
        wrap = bits[:-1, cols - 1] & bits[1:, 0]
        r = np.flatnonzero(wrap)
        pa.append(r * cols + cols - 1)
        pb.append((r + 1) * cols)
    pa, pb = np.concatenate(pa), np.concatenate(pb)
    n = rows * cols
    _, lab = connected_components(coo_matrix((np.ones(pa.size, np.int8), (pa, pb)), shape=(n, n)), directed=False)
    cells = np.flatnonzero(bits.ravel())
    return cells, lab[cells]


def records_of(cells, lab, cols, row0=0):
    """One record (component_list_ref.DTYPE) per component number in `lab`, in the order of their first cells."""
    out = np.zeros(0, component_list_ref.DTYPE)
    if cells.size == 0:
        return out
    _, first, inv = np.unique(lab, return_index=True, return_inverse=True)
    rank = np.empty(first.size, np.int64)
    rank[np.argsort(first)] = np.arange(first.size)
    k = rank[inv]
    n = first.size
    r, c = np.divmod(cells, cols)
    r = r + row0
    out = np.zeros(n, component_list_ref.DTYPE)
    out["size"] = np.bincount(k, minlength=n)
    for name, x in (("sum_row", r), ("sum_col", c)):
        s = np.zeros(n, np.int64)
        np.add.at(s, k, x)
        out[name] = s
    f = np.sort(cells[first])
    out["first_row"], out["first_col"] = f // cols + row0, f % cols
    for name, x, op, start in (("row_min", r, np.minimum, 1 << 40), ("row_max", r, np.maximum, -1), ("col_min", c, np.minimum, 1 << 40),
                               ("col_max", c, np.maximum, -1)):
        m = np.full(n, start, np.int64)
        op.at(m, k, x)
        out[name] = m
    return out


def counters_of(rec):
    return component_list_ref.counters(rec)


def merged_list(bits, conn, min_size, seams, fault):
    """The list as the host forms it from the slabs' own lists, with one of LIST_FAULTS in the merge."""
    rows, cols = bits.shape
    bounds = [0] + list(seams) + [rows]
    cells, lab = components_of(bits, conn)
    owner = np.full(rows * cols, -1, np.int64)
    owner[cells] = lab
    pieces = []                                           # (component of the whole plane, slab, record with global rows)
    for s in range(len(bounds) - 1):
        r0, r1 = bounds[s], bounds[s + 1]
        pc, pl = components_of(bits[r0:r1], conn)
        rec = records_of(pc, pl, cols, r0)
        for x in rec:
            pieces.append((int(owner[int(x["first_row"]) * cols + int(x["first_col"])]), s, x))
    by_whole = collections.defaultdict(list)
    for w, s, x in pieces:
        by_whole[w].append((s, x))
    single, merged = [], []
    for w, group in by_whole.items():
        if fault == "min-size-before-merge":
            group = [(s, x) for s, x in group if int(x["size"]) >= min_size]
            if not group:
                continue
        out = np.zeros(1, component_list_ref.DTYPE)[0]
        local = fault == "local-rows" and len(group) > 1
        shift = [bounds[s] if local else 0 for s, _ in group]
        out["size"] = sum(int(x["size"]) for _, x in group)
        out["sum_row"] = sum(int(x["sum_row"]) - int(x["size"]) * d for (_, x), d in zip(group, shift))
        out["sum_col"] = sum(int(x["sum_col"]) for _, x in group)
        firsts = [(int(x["first_row"]) - d, int(x["first_col"])) for (_, x), d in zip(group, shift)]
        out["first_row"], out["first_col"] = firsts[-1] if fault == "last-piece-first-cell" else min(firsts)
        boxed = group[:1] if fault == "first-piece-box" else group
        out["row_min"] = min(int(x["row_min"]) - d for (_, x), d in zip(boxed, shift))
        out["row_max"] = max(int(x["row_max"]) - d for (_, x), d in zip(boxed, shift))
        out["col_min"], out["col_max"] = min(int(x["col_min"]) for _, x in boxed), max(int(x["col_max"]) for _, x in boxed)
        if int(out["size"]) >= min_size:
            (merged if len(group) > 1 else single).append(out)
    key = lambda x: (int(x["first_row"]), int(x["first_col"]))
    if fault == "merged-last":
        ordered = sorted(single, key=key) + sorted(merged, key=key)
    else:
        ordered = sorted(single + merged, key=key)
    return np.array(ordered, component_list_ref.DTYPE) if ordered else np.zeros(0, component_list_ref.DTYPE)


def pairs_of(bits, max_lag, fault=None, seams=()):
    rows, cols = bits.shape
    seams = np.asarray(sorted(seams), np.int64)
    out = np.zeros((4, max_lag + 1), np.uint64)
    flat = bits.ravel()
    shift = 1 if fault == "lag+1" else 0
    for k, (dr, dc) in enumerate(corr_ref.STEPS):
        for lag in range(max_lag + 1):
            d = lag + shift if lag > 0 else 0
            if fault == "row-wrap" and k == 0:
                out[k, lag] = np.count_nonzero(flat[:flat.size - d] & flat[d:]) if d < flat.size else 0
                continue
            if d * dr >= rows or d * abs(dc) >= cols:
                continue
            r, c = np.mgrid[0:rows - d * dr, (d if dc < 0 else 0):(cols - d if dc > 0 else cols)]
            r2, c2 = r + d * dr, c + d * dc
            both = bits[r, c] & bits[r2, c2]
            if fault == "no-unit-row" and k > 0:
                both &= (r // O.PAIR_ROWS) == (r2 // O.PAIR_ROWS)
            elif fault == "no-strip":
                both &= (c // O.STRIP_COLS) == (c2 // O.STRIP_COLS)
            elif fault == "no-word-carry" and d >= O.WORD_COLS:
                both &= (c // O.WORD_COLS) == (c2 // O.WORD_COLS)
            elif fault == "no-slab-row":
                both &= np.searchsorted(seams, r, side="right") == np.searchsorted(seams, r2, side="right")
            out[k, lag] = np.count_nonzero(both)
    return out


def quads_of(bits, fault=None):
    rows, cols = bits.shape
    b = np.pad(bits, 1).astype(np.int64)
    if fault == "no-right-ring":
        b = b[:, :-1]
    if fault == "no-bottom-ring":
        b = b[:-1]
    tl, tr, bl, br = b[:-1, :-1], b[:-1, 1:], b[1:, :-1], b[1:, 1:]
    n = tl + tr + bl + br
    kind = np.where((n == 2) & (tl == br), 5, n)                 # Q0 .. Q4 by their number of set cells, QD = 5
    weight = np.ones(kind.shape[0], np.int64)
    shared = np.arange(kind.shape[0]) % O.QUAD_ROWS == 0
    shared[0] = False                                            # (quad row 0 has no unit above it)
    if fault == "shared-row-twice":
        weight[shared] = 2
    if fault == "shared-row-never":
        weight[shared] = 0
    out = np.bincount(kind.ravel(), weights=np.repeat(weight, kind.shape[1]), minlength=6).astype(np.uint64)
    if fault == "qd-q2":
        out[[2, 5]] = out[[5, 2]]
    return out


def histogram_of(a, lo, hi, bins, fault=None):
    a = np.asarray(a, np.float32)
    if fault == "ftz":
        a = flushed(a)
    if fault == "last-block" and a.shape[1] % O.STRIP_COLS:
        a = a[:, :a.shape[1] // O.STRIP_COLS * O.STRIP_COLS]
    slots = hist_ref.slots(a, lo, hi, bins)
    lo32, hi32 = np.float32(lo), np.float32(hi)
    if fault == "hi-above":
        slots = np.where(a == hi32, bins + 1, slots)
    if fault == "nan-below-range":
        slots = np.where(np.isnan(a), bins, slots)
    if fault == "f64-bin":
        with np.errstate(all="ignore"):
            inside = ~(np.isnan(a) | (a < lo32) | (a > hi32))
            t = (np.where(inside, a, lo32).astype(np.float64) - float(lo32)) * (bins / (float(hi32) - float(lo32)))
        slots = np.where(inside, np.minimum(t.astype(np.int64), bins - 1), slots)
    return np.bincount(slots.ravel(), minlength=bins + 3).astype(np.uint64)


def beside(fault, a, right, below):
    """Plane `a` with what lies beside it taken for cells of its own."""
    if fault == "right-seen":
        return np.concatenate([a, right[:, None]], axis=1)
    if fault == "below-seen":
        return np.concatenate([a, below[None, :]], axis=0)
    return a


def observable(family, fault, a, t, above, conn, max_lag, min_size, span, bins, seams, right, below):
    """What the observable gives with `fault` (None: what it gives)."""
    if family == "histogram":
        return histogram_of(beside(fault, a, right, below), span[0], span[1], bins, fault)
    a = beside(fault, a, right, below)
    bits = faulty_bits(fault, a, t, above)
    if family == "morphology":
        return quads_of(bits, fault)
    if family == "correlation":
        return pairs_of(bits, max_lag, fault, seams)
    if fault in LIST_FAULTS:
        return merged_list(bits, conn, min_size, seams, fault)
    cells, lab = components_of(bits, conn, fault, seams)
    rec = records_of(cells, lab, bits.shape[1])
    return counters_of(rec) if family == "components" else rec[rec["size"] >= np.uint64(min_size)]


def views_of(c):
    """What pinned example `c` shows of its first plane (an ensemble: both species of one member of the range -- a retired
    one where members are retired, whose planes stay what they were): (plane, threshold list, sense, right, below, slabs'
    first rows, min_size, range) each."""
    slabs, max_lag, _ = P.legal(c)
    rows, cols = c["rows"], c["cols"]
    out = []
    if c["form"] == "ensemble":
        u, v = P.member_planes(c)
        inside = range(c["first"], c["first"] + c["count"])
        m = next((i for i in inside if c["retire"] and c["retired"][i]), c["first"])
        for s, planes in ((0, u), (1, v)):
            thresholds, above = P.plane_rules(c, s)
            a = planes[m]
            # a member's rows lie `cols` floats apart: right of a row's last cell lies the next row's first, below the
            # last row the next plane -- set in every cell where it is outside the range or fenced, else unknown here
            follows_set = m + 1 < c["members"] and (m + 1 not in inside or c["fence"])
            below = np.full(cols, O.poison_value(above) if follows_set else a[0, 0], np.float32)
            right = np.concatenate([a[1:, 0], below[:1]])
            out.append((a, thresholds, above, right, below if follows_set else None, [], P.min_size_of(c, a, thresholds[0], above),
                        P.hist_range(c, a)))
        return out, max_lag
    a, thresholds, above = P.field_planes(c)[0]
    pitch = -(-cols // 64) * 64                                       # a field's pitch is a multiple of 64
    beyond = O.poison_value(above) if c["poison"] else np.float32(0)   # planes are created zero-filled
    below = np.full(cols, beyond, np.float32)
    right = np.full(rows, beyond, np.float32) if pitch > cols else np.concatenate([a[1:, 0], below[:1]])
    return [(a, thresholds, above, right, below, O.seam_rows(rows, slabs), P.min_size_of(c, a, thresholds[0], above), P.hist_range(c, a))], max_lag


@functools.lru_cache(maxsize=None)
def discrimination(n):
    """{fault: does pinned example `n` give another result with it than without} for the faults of its family; the
    restatement without a fault is held to the reference first."""
    c = P.EDGE_EXAMPLES[n]
    family = c["family"]
    views, max_lag = views_of(c)
    caught = {f: False for f in FAULTS[family]}
    for a, thresholds, above, right, below, seams, min_size, span in views:
        for t in (thresholds[:1] if family in ("component_list", "histogram") else thresholds):
            args = (a, t, above, c["conn"], max_lag, min_size, span, c["bins"], seams, right, below)
            true = P.reference(c, a, t, above, max_lag, min_size, span)
            assert P.same(observable(family, None, *args), true), (n, t)
            if family == "component_list":
                assert P.same(merged_list(morph_ref.set_cells(a, t, above), c["conn"], min_size, seams, None), true), (n, t)
            for fault in FAULTS[family]:
                if caught[fault] or (fault == "below-seen" and below is None):
                    continue
                caught[fault] = not P.same(observable(family, fault, *args), true)
    return caught


@pytest.mark.parametrize("n", range(len(P.EDGE_EXAMPLES)))
def test_pinned_example_discriminates(n):
    caught = discrimination(n)
    assert any(caught.values()), P.EDGE_EXAMPLES[n]


@pytest.mark.parametrize("family", P.FAMILIES)
def test_every_fault_is_caught_by_three_pinned_examples(family):
    examples = [n for n, c in enumerate(P.EDGE_EXAMPLES) if c["family"] == family]
    catches = {f: [n for n in examples if discrimination(n)[f]] for f in FAULTS[family]}
    assert all(len(v) >= 3 for v in catches.values()), {f: v for f, v in catches.items() if len(v) < 3}
