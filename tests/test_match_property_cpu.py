"""The randomised GPU parity test of the component matches (tests/test_gpu_match_property.py) without a GPU: its strategy
draws legal cases of every kind within the caps, and cases in which something is matched -- over 2000 draws at most a third
without an overlap, each of the five events in a fifth of them at least, an overlap made of several pieces in a sixth --;
and the pinned examples discriminate: a model of the match -- both planes labelled and listed (components_of, merged_list and
their labelling and seam faults from tests/test_observe_property_cpu.py), the pieces of every slab in first-cell order, the
slot a piece's root takes among the roots of its workgroup's waves, the records a piece names, the host's mapping, cutting
and folding -- is held to match_ref.match without a fault, and with exactly one fault each it gives another match than the
reference on at least three pinned examples, while every pinned example tells at least one fault.  (An ensemble whose
members are retired and advanced is modelled with the planes it was given: what the steps make of the others is the
device's.)"""
import collections
import functools

import numpy as np
import pytest

from . import component_list_ref, match_ref, morph_ref
from . import observe_cases as O
from . import test_gpu_match_property as P
from . import test_observe_property_cpu as C


# ---- the strategy ------------------------------------------------------------------------------------------------------------
def test_the_strategy_draws_legal_cases_in_which_something_is_matched():
    from hypothesis import HealthCheck, given, seed, settings

    seen = collections.Counter()

    @seed(20240612)
    @settings(max_examples=2000, deadline=None, database=None, suppress_health_check=list(HealthCheck))
    @given(P.cases())
    def draw(c):
        P.legal(c)
        seen["draws"] += 1
        seen.update(set(P.counts_of(c)) - {"examples"})
        seen.update({("kind", c["kind"]), ("threshold", repr(c["threshold"])), ("species", c["species"])})
        if c["form"] == "ensemble":
            seen.update({("members", c["members"])})
            seen.update({("empty", P.EMPTY[e], place) for place, e in enumerate(c["empties"]) if e})
            before, after = P.member_planes(c)
            before, after = before[P.plain_member(c)], after[P.plain_member(c)]
        else:
            before, after = P.pair_of_planes(c, c["seed"])
        t, above, conn = c["threshold"], c["above"], c["conn"]
        min_size = P.min_size_of(c, before, after)
        rb, ra, ov = match_ref.match(before, after, t, above, conn, min_size)
        seen["no overlap"] += ov.shape[0] == 0
        seen.update(k for k, n in match_ref.events(rb, ra, ov).items() if n)
        seen["several pieces"] += bool(ov.shape[0]) and bool((match_ref.pieces(before, after, t, above, conn, min_size) > 1).any())

    draw()
    n = seen["draws"]
    assert n >= 1900, n
    want = (["form " + f for f in P.FORMS] + [f"slabs {s}" for s in range(1, 6)] + ["one-row slabs", "poisoned", "retired members", "fenced",
                                                                                     "a member with an empty list", "ensemble load path ragged",
                                                                                     "ensemble load path 16 bytes", "nothing can be set"]
            + ["connectivity 4", "connectivity 8", "sense above", "sense below"] + ["min_size " + w for w in P.MIN_SIZES]
            + ["after " + a for a in P.AFTERS] + [("kind", k) for k in O.KINDS] + [("threshold", repr(t)) for t in P.THRESHOLDS]
            + [("species", s) for s in "uv"] + [("members", m) for m in range(1, 7)]
            + [("empty", e, place) for e in ("before", "after") for place in range(3)])
    rare = {k: seen[k] for k in want if seen[k] < 5}
    assert not rare, rare
    assert seen["nothing can be set"] * 8 <= n, seen["nothing can be set"]
    # a green run must mean something: what the reference alone finds in the draws
    assert seen["no overlap"] * 3 <= n, seen["no overlap"]
    for event in ("continued", "split", "merged", "born", "died"):
        assert seen[event] * 5 >= n, (event, seen[event])
    assert seen["several pieces"] * 6 >= n, seen["several pieces"]


def test_the_pinned_examples_are_legal_and_cover_the_forms():
    counts = collections.Counter()
    for c in P.EDGE_EXAMPLES:
        counts.update(P.counts_of(c))
    need = (["form " + f for f in P.FORMS] + [f"slabs {s}" for s in range(1, 6)] + ["min_size " + w for w in P.MIN_SIZES]
            + ["after " + a for a in P.AFTERS + P.LAYOUTS] + ["connectivity 4", "connectivity 8", "sense above", "sense below",
                                                             "poisoned", "one-row slabs", "retired members", "fenced", "nothing can be set",
                                                             "a member with an empty list", "ensemble load path ragged", "ensemble load path 16 bytes"])
    assert all(counts[k] > 0 for k in need), {k: counts[k] for k in need if not counts[k]}
    for shape in P.ENSEMBLE_SHAPES:                        # ragged, with an empty member at each place
        found = [c for c in P.EDGE_EXAMPLES if (c["rows"], c["cols"]) == shape and c["form"] == "ensemble"]
        assert P.ragged(shape) and found, shape
        assert all(any(c["empties"][place] for c in found) for place in range(3)), shape
    moved = {(c["kind"], c["conn"], c["slabs"]) for c in P.EDGE_EXAMPLES if c["after"] == "moved" and max(map(abs, c["move"])) == 1}
    assert moved >= {(k, n, s) for k in P._ADVERSARIAL for n in (4, 8) for s in (2, 5)}


def test_the_layouts_are_what_they_claim():
    for c in P.EDGE_EXAMPLES:
        if c["kind"] not in P.LAYOUTS:
            continue
        before, after = P.pair_of_planes(c, c["seed"])
        t, above = c["threshold"], c["above"]
        pieces = match_ref.pieces(before, after, t, above, c["conn"])
        b, a = morph_ref.set_cells(before, t, above), morph_ref.set_cells(after, t, above)
        roots = np.flatnonzero((b & a).ravel())
        if c["kind"] == "u against bars":
            assert sorted(pieces) == [1, 1] and c["at"] in O.seam_rows(c["rows"], c["slabs"])      # two pairs, each piece cut by the seam
            assert all((b & a)[r, x] for r in (c["at"] - 1, c["at"]) for x in (1, c["cols"] - 2))
        elif c["kind"] == "u against z":
            assert list(pieces) == [2]                            # one overlap, a piece on either side of the seam
            assert (b & a)[:c["at"]].any() and (b & a)[c["at"]:].any()
        elif c["kind"] == "wave roots":
            assert sorted({(e // P.ENTRIES, e % P.ENTRIES // 64) for e in roots}) == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (1, 3)]
        else:
            assert c["at"] in roots and len(roots) == 3 and roots[0] < 255


# ---- the pinned examples discriminate ----------------------------------------------------------------------------------------
MATCH_FAULTS = ["pieces-not-added",         # two pieces of one pair are left as two overlaps
                "seam-pieces-not-added",    # pieces cut by a seam are not added: one overlap per slab
                "min-size-per-slab",        # min_size is applied to a slab's part of a component, before the seam merge
                "drop-by-before-alone",     # a pair is dropped only when its before-record is not listed
                "first-cell-order",         # the overlaps come in first-cell order, not sorted
                "cells-after-size",         # an overlap's cells are taken as the after-record's size
                "pair-right-of-root",       # a piece's pair is read one cell to the right of its root
                "first-wave-slots",         # the roots of a workgroup's later waves take the first wave's slots
                "last-prefix-short",        # the prefix of the last workgroup is one short
                "batch-not-shifted",        # a batch's indices are not shifted by the planes before
                "empty-before-previous",    # a member's pieces go to the previous member when that one's before-list is empty
                "after-other-sense"]        # the after plane is thresholded with the other sense
FAULTS = C.RULE_FAULTS[:2] + C.COMPONENT_FAULTS + C.LIST_FAULTS + MATCH_FAULTS
UNSET = 0xFFFFFFFF
MARK = (UNSET, UNSET, 0)


def structure(conn):
    from scipy import ndimage

    return ndimage.generate_binary_structure(2, 1 if conn == 4 else 2)


def labelled(bits, conn, min_size, seams, fault):
    """(component number per cell in first-cell order, -1 where unset; record index per number, -1 where not listed; the
    list) of one plane, the labelling with `fault` where it is one of the labelling's or of the list's."""
    cells, lab = C.components_of(bits, conn, fault if fault in C.COMPONENT_FAULTS else None, seams)
    plane = np.full(bits.size, -1, np.int64)
    sizes = np.zeros(0, np.int64)
    if cells.size:
        _, first, inv = np.unique(lab, return_index=True, return_inverse=True)
        rank = np.empty(first.size, np.int64)
        rank[np.argsort(first)] = np.arange(first.size)
        plane[cells] = rank[inv]
        sizes = np.bincount(rank[inv])
    keep = sizes >= min_size
    index = np.where(keep, np.cumsum(keep) - 1, -1)
    records = C.records_of(cells, lab, bits.shape[1])
    records = records[records["size"] >= np.uint64(min_size)]
    if fault in C.LIST_FAULTS:
        records = C.merged_list(bits, conn, min_size, seams, fault)
    return plane.reshape(bits.shape), index, records


def raw_overlaps(bits_b, bits_a, lab_b, idx_b, lab_a, idx_a, conn, min_size, fault):
    """The raw overlaps of one launch over a dense block of rows: one per piece, in the slot its root takes."""
    from scipy import ndimage

    both = bits_b & bits_a
    lab_p, n = ndimage.label(both, structure(conn))
    if n == 0:
        return []
    at = np.flatnonzero(lab_p.ravel())
    _, first, cells = np.unique(lab_p.ravel()[at], return_index=True, return_counts=True)
    order = np.argsort(at[first])
    roots, cells = at[first][order], cells[order]
    local = [ndimage.label(b, structure(conn))[0].ravel() for b in (bits_b, bits_a)]
    local_sizes = [np.bincount(x) for x in local]
    fb, fa = lab_b.ravel(), lab_a.ravel()
    raw = []
    for root, count in zip(roots.tolist(), cells.tolist()):
        read = root + 1 if fault == "pair-right-of-root" else root
        if read >= fb.size or fb[read] < 0 or fa[read] < 0:
            raw.append(MARK)
            continue
        b, a = int(idx_b[fb[read]]), int(idx_a[fa[read]])
        if fault == "min-size-per-slab" and (local_sizes[0][local[0][root]] < min_size or local_sizes[1][local[1][root]] < min_size):
            b = -1
        if fault == "drop-by-before-alone" and b >= 0 and a < 0:
            a = UNSET
        raw.append((b, a, count) if b >= 0 and a >= 0 else MARK)
    if fault in ("first-wave-slots", "last-prefix-short"):
        group = roots // P.ENTRIES
        prefix = np.searchsorted(group, np.arange(group.max() + 1))        # pieces before each workgroup
        groups_in_grid = -(-fb.size // P.ENTRIES)
        slots = [MARK] * len(raw)
        for k, (root, g) in enumerate(zip(roots.tolist(), group.tolist())):
            rank = k - int(prefix[g])
            if fault == "first-wave-slots":
                wave = root % P.ENTRIES // 64
                rank = int(np.count_nonzero((group == g) & (roots % P.ENTRIES // 64 == wave) & (roots < root)))
            start = int(prefix[g]) - (1 if fault == "last-prefix-short" and g == groups_in_grid - 1 and prefix[g] > 0 else 0)
            slots[start + rank] = raw[k]
        raw = slots
    return raw


def folded(raw, rec_a, fault):
    """[(slab, (before, after, cells))] as the host folds them."""
    kept = [(s, o) for s, o in raw if o[0] != UNSET]
    if fault != "first-cell-order":
        kept.sort(key=lambda x: (x[1][0], x[1][1]))
    out, owner = [], {}
    for s, (b, a, n) in kept:
        key = (b, a, s) if fault == "seam-pieces-not-added" else (b, a)
        if fault != "pieces-not-added" and key in owner:
            out[owner[key]][2] += n
        else:
            owner[key] = len(out)
            out.append([b, a, n])
    overlaps = np.zeros(len(out), match_ref.OVERLAP)
    for k, (b, a, n) in enumerate(out):
        overlaps[k] = (b, a, int(rec_a["size"][a]) if fault == "cells-after-size" and a < len(rec_a) else n)
    return overlaps


def sets_of(c, plane, fault, after=False):
    above = c["above"] != (fault == "after-other-sense" and after)
    return C.faulty_bits(fault, plane, c["threshold"], above)


def plane_match(c, before, after, min_size, seams, fault):
    """(before's records, after's records, overlaps) of one pair of planes in a chain whose slabs begin at `seams`."""
    conn = c["conn"]
    bits_b, bits_a = sets_of(c, before, fault), sets_of(c, after, fault, after=True)
    lab_b, idx_b, rec_b = labelled(bits_b, conn, min_size, seams, fault)
    lab_a, idx_a, rec_a = labelled(bits_a, conn, min_size, seams, fault)
    raw = []
    bounds = [0] + list(seams) + [before.shape[0]]
    for s in range(len(bounds) - 1):
        rows = slice(bounds[s], bounds[s + 1])
        raw += [(s, o) for o in raw_overlaps(bits_b[rows], bits_a[rows], lab_b[rows], idx_b, lab_a[rows], idx_a, conn, min_size, fault)]
    return rec_b, rec_a, folded(raw, rec_a, fault)


def modelled(c, fault=None):
    """[(records, records, overlaps)] of pinned example `c`, one per plane matched, as the model gives them with `fault`."""
    if c["form"] != "ensemble":
        before, after = P.pair_of_planes(c, c["seed"])
        return [plane_match(c, before, after, P.min_size_of(c, before, after), O.seam_rows(c["rows"], c["slabs"]), fault)]
    before, after = P.member_planes(c)
    for m in range(c["members"]):
        if c["retire"] and c["retired"][m]:
            after[m] = before[m]
    first, count = c["first"], c["count"]
    min_size = P.min_size_of(c, before[P.plain_member(c)], after[P.plain_member(c)])
    out = [plane_match(c, before[m], after[m], min_size, [], fault) for m in range(first, first + count)]
    nb, na = np.cumsum([0] + [len(x[0]) for x in out]), np.cumsum([0] + [len(x[1]) for x in out])
    if fault == "batch-not-shifted":                       # the indices stay those of the batch's records
        for p, (_, _, ov) in enumerate(out):
            ov["before"] += np.uint32(nb[p])
            ov["after"] += np.uint32(na[p])
    if fault == "empty-before-previous":
        for p in range(1, count):
            if len(out[p - 1][0]) == 0 and len(out[p][2]):   # cut into the plane before, whose after-records come first
                moved = out[p][2].copy()
                moved["after"] += np.uint32(na[p] - na[p - 1])
                out[p - 1] = (out[p - 1][0], out[p - 1][1], moved)
                out[p] = (out[p][0], out[p][1], out[p][2][:0])
    return out


def referenced(c):
    if c["form"] != "ensemble":
        before, after = P.pair_of_planes(c, c["seed"])
        return [match_ref.match(before, after, c["threshold"], c["above"], c["conn"], P.min_size_of(c, before, after))]
    before, after = P.member_planes(c)
    for m in range(c["members"]):
        if c["retire"] and c["retired"][m]:
            after[m] = before[m]
    min_size = P.min_size_of(c, before[P.plain_member(c)], after[P.plain_member(c)])
    return [match_ref.match(before[m], after[m], c["threshold"], c["above"], c["conn"], min_size)
            for m in range(c["first"], c["first"] + c["count"])]


def same_matches(x, y):
    return len(x) == len(y) and all(P.same(np.ascontiguousarray(p), np.ascontiguousarray(q)) for a, b in zip(x, y) for p, q in zip(a, b))


@functools.lru_cache(maxsize=None)
def discrimination(n):
    """{fault: does pinned example `n` give another match with it than the reference}; the model without a fault is held to
    the reference first."""
    c = P.EDGE_EXAMPLES[n]
    true = referenced(c)
    assert same_matches(modelled(c), true), n
    return {fault: not same_matches(modelled(c, fault), true) for fault in FAULTS}


@pytest.mark.parametrize("n", range(len(P.EDGE_EXAMPLES)))
def test_pinned_example_discriminates(n):
    caught = discrimination(n)
    assert any(caught.values()), P.EDGE_EXAMPLES[n]


def test_every_fault_is_caught_by_three_pinned_examples():
    catches = {f: [n for n in range(len(P.EDGE_EXAMPLES)) if discrimination(n)[f]] for f in FAULTS}
    assert all(len(v) >= 3 for v in catches.values()), {f: v for f, v in catches.items() if len(v) < 3}
