"""Randomised parity of the component matches (gs_fields_match, gs_members_match) -- HipConcentration.match,
Species.match_since, Ensemble.matches_since -- against their restatement, tests/match_ref.py: both lists record for record,
the overlaps equal in the same order, counts() equal to match_ref.events.  All integers, no tolerance.

`cases()` draws

* the shape from tests/test_gpu_observe_property.py's ROWS and COLS (the labelling tile of 16 x 256, the lanes' words, the
  strips: cells on both sides of every multiple of 256 entries), at most MEMBER_CAP cells a plane -- the reference labels
  both planes and their pieces;
* the `before` pattern from observe_cases.KINDS with its densities and places, and what `after` is to it: another draw of
  the kind, a draw of another kind, `before` itself (the same handle, or a copy), `before` moved by up to two cells without
  wrapping, `before` with one cell in twelve flipped, `before` with the rows on either side of every seam drawn again; the
  values carry the patterns through observe_cases.values_of with its special cells;
* the rule: a threshold of the observables' THRESHOLDS (one that nothing can satisfy under the sense in one draw of eight at
  most), either sense, connectivity 4 or 8, min_size 1, 2, 5, the largest component's size, one more, or the row count;
* the call: two fields, a Species with a snapshot, or a member range of an ensemble and its snapshot;
* for fields, a chain of 1 .. 5 slabs (one-row slabs occur) and `poison`: the ghost rows and the pitch padding of both planes
  set by the widest margin; for ensembles 1 .. 6 members, half of the shapes ragged, the members outside the range set in
  every cell, `fence` setting the first and last row of those inside, members with nothing set before or nothing set after
  at the first, a middle and the last place of the range, and half of the cases retiring some members and advancing the
  others by an odd number of steps.

Beyond parity, on the device: with min_size 1 the overlaps' cells sum to the cells set in both planes; the overlaps of a
record sum to its size at most; match(a, a) is (i, i, size_i); match(b, a) is match(a, b) with the columns exchanged and
sorted again; both lists are the planes' component_list under the rule; several slabs equal one and poison changes nothing;
a member equals a lone pair of fields, a range the same members of the whole; a retired member's components all continue as
themselves; the context's counters and the planes are what they were.  tests/test_match_property_cpu.py checks without a
GPU that the strategy draws legal cases of every kind in which something is matched, and that the pinned examples would
notice each single fault of the kernels or of the host's folding."""
import collections
import os
import time

import numpy as np
import pytest
from hypothesis import HealthCheck, example, given, settings, strategies as st

from grayscott_amd import HipArgs, HipConcentration, Parameters, Simulation

from . import component_list_ref, components_ref, match_ref, morph_ref
from . import observe_cases as O
from .test_gpu_observe_property import COLS, ENSEMBLE_SHAPES, MEMBER_CAP, ROWS, THRESHOLDS, poison, ragged, same, shortest_slab

pytestmark = pytest.mark.gpu

FORMS = ["field", "species", "ensemble"]
INF = float("inf")
MIN_SIZES = ["1", "2", "5", "largest", "largest + 1", "rows"]
AFTERS = ["again", "other", "same handle", "copy", "moved", "flipped", "seams redrawn"]
# Pairs of planes that only pinned examples use (`at`: the seam, or the column, they are about)
LAYOUTS = ["u against bars", "u against z", "wave roots", "row roots"]
EMPTY = [None, "before", "after"]                      # a member with nothing set before, or after
ENTRIES = 256                                          # entries of a workgroup of gs_match_pairs_k; 64 to a wave
# What is drawn more often than the rest, so that something is matched in most draws (tests/test_match_property_cpu.py holds
# 2000 draws to it: an overlap in two thirds, every event in a fifth, an overlap of several pieces in a sixth): the kinds in
# which many components of both planes meet, the relations that break and join them, and the small values of min_size --
# with "largest" the largest component is listed on one side alone, with "largest + 1" nothing is
KIND_DRAWS = O.KINDS + ["planted"] * 9 + ["seams"] * 5 + ["lane_runs"] * 5 + ["rings", "comb"]
AFTER_DRAWS = AFTERS + ["again", "again", "flipped", "flipped", "flipped", "other", "seams redrawn", "moved"]
MIN_SIZE_DRAWS = [0] * 12 + [1, 1, 2, 2, 3, 4, 5]

SEEN = collections.Counter()
SLOWEST = [""]                          # which example took longest, for the report


def pinned_case(**kw):
    """A case of `cases` with every field at its plainest value but those given (the @example cases)."""
    base = dict(form="field", rows=17, cols=259, seed=1, kind="planted", density=0.5, at=None, after="again", other="planted",
                move=(0, 1), threshold=0.3, above=True, conn=8, min_size=0, slabs=1, poison=False, species="v", members=1, first=0,
                count=1, fence=False, empties=(0, 0, 0), retire=False, retired=[False] * 6, steps=1)
    base.update(kw)
    return base


def impossible(t, above):
    """Can no cell be set under this rule (nothing is above +inf or below -inf)?"""
    return np.isinf(np.float32(t)) and (t > 0) == above


@st.composite
def cases(draw, form=None):
    form = form or draw(st.sampled_from(FORMS))
    t, above = draw(st.sampled_from(THRESHOLDS)), draw(st.booleans())
    if impossible(t, above) and draw(st.integers(0, 3)) != 0:      # two rules of sixteen are: a quarter of them go on
        above = not above
    c = pinned_case(form=form, seed=draw(st.integers(0, 2 ** 16)), kind=draw(st.sampled_from(KIND_DRAWS)),
                    density=draw(st.sampled_from(O.DENSITIES)), at=draw(st.sampled_from([None, None] + O.PLACES)),
                    after=draw(st.sampled_from(AFTER_DRAWS)), other=draw(st.sampled_from(KIND_DRAWS)),
                    move=(draw(st.integers(-2, 2)), draw(st.integers(-2, 2))), threshold=t, above=above, conn=draw(st.sampled_from([4, 8])),
                    min_size=draw(st.sampled_from(MIN_SIZE_DRAWS)), poison=draw(st.booleans()), species=draw(st.sampled_from("uv")),
                    fence=draw(st.booleans()), empties=tuple(draw(st.integers(0, 2)) for _ in range(3)) if draw(st.booleans()) else (0, 0, 0),
                    retire=draw(st.booleans()), retired=[draw(st.booleans()) for _ in range(6)], steps=draw(st.sampled_from([1, 3, 5])))
    if form == "ensemble":
        want_ragged = draw(st.booleans())
        if want_ragged and draw(st.integers(0, 3)) == 0:
            rows, cols = draw(st.sampled_from(ENSEMBLE_SHAPES))
        else:
            rows = draw(st.sampled_from(ROWS))
            cols = draw(st.sampled_from([x for x in COLS if rows * x <= MEMBER_CAP and ragged((rows, x)) == want_ragged]))
        members = draw(st.integers(1, 6))
        first = draw(st.integers(0, members - 1))
        c.update(rows=rows, cols=cols, members=members, first=first, count=draw(st.integers(1, members - first)))
        return c
    rows = draw(st.sampled_from(ROWS))
    cols = draw(st.sampled_from([x for x in COLS if rows * x <= MEMBER_CAP]))
    c.update(rows=rows, cols=cols, slabs=min(draw(st.integers(1, 5)), rows))
    return c


def legal(c):
    """The strategy's own check (tests/test_match_property_cpu.py draws cases on the CPU).  Neither a field chain in one
    process nor an ensemble refuses a match: every case runs as it is drawn."""
    rows, cols, form = c["rows"], c["cols"], c["form"]
    assert form in FORMS and (c["kind"] in O.KINDS or c["kind"] in LAYOUTS) and c["other"] in O.KINDS and c["density"] in O.DENSITIES
    assert c["after"] in AFTERS and c["conn"] in (4, 8) and 0 <= c["min_size"] < len(MIN_SIZES) and c["species"] in "uv"
    assert c["threshold"] in THRESHOLDS and all(-2 <= d <= 2 for d in c["move"]) and c["steps"] % 2 == 1
    assert rows * cols <= MEMBER_CAP and all(e in (0, 1, 2) for e in c["empties"])
    if (rows, cols) not in ENSEMBLE_SHAPES and c["kind"] not in LAYOUTS:
        assert rows in ROWS and cols in COLS
    if form == "ensemble":
        assert 1 <= c["members"] <= 6 and 0 <= c["first"] and c["count"] >= 1 and c["first"] + c["count"] <= c["members"]
        assert c["slabs"] == 1
    else:
        assert 1 <= c["slabs"] <= min(5, rows)


# ---- planes ------------------------------------------------------------------------------------------------------------------
def empty_places(c):
    """The first, a middle and the last place of the range; a range of one member has none (what is emptied is one member
    among others: a lone member with an empty list is the `empty` kind's business)."""
    return [c["first"], c["first"] + c["count"] // 2, c["first"] + c["count"] - 1] if c["count"] > 1 else []


def bits_of(c, kind, seed):
    """The set cells of a plane of pattern `kind` under the case's rule."""
    shape, t, above = (c["rows"], c["cols"]), c["threshold"], c["above"]
    if kind == "planted":
        return morph_ref.set_cells(O.plane("planted", shape, t, above, seed, c["density"]), t, above)
    return O.pattern(kind, shape, np.random.default_rng(seed), c["density"], c["at"], c["slabs"])


def layout_bits(c):
    """(before, after) of the pairs of planes that only pinned examples use."""
    shape = rows, cols = c["rows"], c["cols"]
    kind, at = c["kind"], c["at"]
    b, a = np.zeros(shape, bool), np.zeros(shape, bool)
    if kind in ("u against bars", "u against z"):
        # a U across seam `at` against two bars through its arms -- two pieces of two pairs, each cut by the seam -- or against
        # a Z that meets one arm above the seam and the other below it: ONE overlap of two pieces in different slabs
        b = components_ref.u_shape(shape, at) != 0
        if kind == "u against bars":
            a[at - 1] = a[at] = True
            a[at - 1, cols // 2] = a[at, cols // 2] = False
        else:
            a[at - 1, :cols // 2 + 1] = a[at, cols // 2:] = True
    elif kind == "wave roots":
        # one piece root in each of the four waves of the workgroup of entries [256, 512), two in the workgroup before it
        assert cols == ENTRIES and rows >= 3
        b[1, [10, 74, 138, 202]] = b[0, [5, 100]] = True
        a = b.copy()
        a[2, 10] = a[2, 202] = True
    else:
        # a root on entry `at` of row 0 (255, 256, 257: the last of a workgroup, the first and second of the next), one
        # before it and one in a later row
        assert cols > ENTRIES + 1 and rows >= 3 and at in (255, 256, 257)
        b[0, [3, at]] = b[2, 7] = True
        a = b.copy()
        a[1, at] = True
    return b, a


def pair_bits(c, seed):
    """(before, after) as boolean planes: `before` of the case's kind, `after` what the case says it is to it."""
    if c["kind"] in LAYOUTS:
        return layout_bits(c)
    rows, cols = shape = (c["rows"], c["cols"])
    rng = np.random.default_rng(seed + 7)
    b = bits_of(c, c["kind"], seed)
    after = c["after"]
    if after == "again":
        return b, bits_of(c, c["kind"], seed + 500)
    if after == "other":
        return b, bits_of(c, c["other"], seed + 500)
    if after in ("same handle", "copy"):
        return b, b
    a = np.zeros(shape, bool)
    if after == "moved":
        dr, dc = c["move"]
        if abs(dr) < rows and abs(dc) < cols:
            a[max(dr, 0):rows + min(dr, 0), max(dc, 0):cols + min(dc, 0)] = b[max(-dr, 0):rows + min(-dr, 0), max(-dc, 0):cols + min(-dc, 0)]
        return b, a
    if after == "flipped":
        return b, b ^ (rng.random(shape) < 1.0 / 12.0)
    a = b.copy()                                              # the rows on either side of every seam drawn again
    for seam in O.seam_rows(rows, c["slabs"]) or ([rows // 2] if rows > 1 else []):
        a[seam - 1:seam + 1] = rng.random((2, cols)) < 0.5
    return b, a


def pair_of_planes(c, seed):
    """(before, after) as f32 planes; `after` is `before` itself (the same array) where the case says so."""
    t, above = c["threshold"], c["above"]
    b, a = pair_bits(c, seed)
    plain = c["kind"] in ("full", "empty", "one-set", "one-unset") or c["kind"] in LAYOUTS     # planes that stay what they are called
    before = O.values_of(b, t, above, np.random.default_rng(seed + 1), special=not plain)
    if c["after"] in ("same handle", "copy") and c["kind"] not in LAYOUTS:
        return before, before
    plain = plain or (c["after"] == "other" and c["other"] in ("full", "empty", "one-set", "one-unset"))
    return before, O.values_of(a, t, above, np.random.default_rng(seed + 2), special=not plain)


def member_planes(c):
    """(before, after) of the case's species as [members, rows, cols] arrays: the members of the range carry the case's
    pair -- with `fence`, their first and last rows set in every cell of both --, a member at the first, a middle or the
    last place of the range has nothing set before, or after, where `empties` says so, and the members outside the range
    are set in every cell of both."""
    shape, above = (c["rows"], c["cols"]), c["above"]
    before, after = np.empty((c["members"],) + shape, np.float32), np.empty((c["members"],) + shape, np.float32)
    unset = O.values_of(np.zeros(shape, bool), c["threshold"], above, np.random.default_rng(c["seed"]), special=False)
    places = empty_places(c)
    for m in range(c["members"]):
        if not c["first"] <= m < c["first"] + c["count"]:
            before[m] = after[m] = O.poison_value(above)
            continue
        before[m], after[m] = pair_of_planes(c, c["seed"] + 10 * m)
        if c["fence"]:
            before[m, 0] = before[m, -1] = after[m, 0] = after[m, -1] = O.poison_value(above)
        for place, e in zip(places, c["empties"]):
            if m == place and EMPTY[e] == "before":
                before[m] = unset
            if m == place and EMPTY[e] == "after":
                after[m] = unset
    return before, after


def plain_member(c):
    """A member of the range that `empties` leaves as it was drawn (the first one, if there is none)."""
    places = empty_places(c)
    emptied = {place for place, e in zip(places, c["empties"]) if e}
    return next((m for m in range(c["first"], c["first"] + c["count"]) if m not in emptied), c["first"])


def min_size_of(c, before, after):
    t, above, conn = c["threshold"], c["above"], c["conn"]
    sizes = [component_list_ref.records(p, t, above, conn)["size"] for p in (before, after)]
    largest = max([int(s.max()) for s in sizes if s.shape[0]] or [0])
    return [1, 2, 5, max(largest, 1), largest + 1, c["rows"]][c["min_size"]]


# ---- pinned examples ---------------------------------------------------------------------------------------------------------
_T, _S = O.TILE_ROWS, O.STRIP_COLS
_ADVERSARIAL = sorted(O.ADVERSARIAL) + ["seams", "lane_runs"]
# The cases that must always run:
# - every adversarial kind (serpentine, comb, rings, checkerboard, staircase, column, seam lines, lane runs) against itself
#   moved by one cell, under both connectivities, on 2 and on 5 slabs, poisoned;
# - a U against bars and a U against a Z at every seam of a chain of 5 slabs: an overlap made of two pieces, and one made of
#   pieces in different slabs; a column against itself with min_size = rows on 5 slabs (every slab's part is smaller);
# - one piece root in each of the four waves of a workgroup of 256 entries; a root on entry 255, 256 and 257 of a row wider
#   than 256; both planes full; either plane empty; one set cell at each of the eight places against a full plane;
# - min_size = largest + 1: both lists empty, no overlap left; a threshold of +inf above: empty whatever the poison;
# - planted planes and their flipped, moved and redrawn selves over more than one tile, with every min_size word, both senses,
#   thresholds 0, -0, a sub-normal and the largest finite value, as fields and as a Species with a snapshot;
# - ensembles: ragged (13, 21), (37, 53), (45, 61) and 16-byte shapes, ranges inside the ensemble, fenced, with a member that
#   has nothing set before or after at the first, a middle and the last place, with and without retired members.
EDGE_EXAMPLES = (
    [pinned_case(kind=k, after="moved", move=mv, conn=n, slabs=s, poison=True, rows=r, cols=w, seed=3 + i, form=form, min_size=ms)
     for i, k in enumerate(_ADVERSARIAL)
     for n, s, mv, r, w, form, ms in ((4, 2, (0, 1), _T + 1, _S + 3, "field", 0), (8, 5, (1, 0) if i % 2 else (1, 1), 2 * _T + 1, _S + 1, "field" if i % 3 else "species", 1),
                                      (8, 2, (1, 0), _T + 1, _S + 1, "species" if i % 3 == 1 else "field", 0), (4, 5, (0, -1) if i % 2 else (-1, 0), 5, _S + 3, "field", 1 if i % 2 else 0))]
    + [pinned_case(kind=k, at=seam, rows=10, cols=12, slabs=5, conn=n, poison=True, after="other", min_size=ms)
       for seam in (2, 4, 6, 8) for k, n, ms in (("u against bars", 4 if seam % 4 else 8, 0), ("u against z", 4, 1 if seam == 4 else 0))]
    + [pinned_case(kind="column", after=a, rows=r, cols=w, slabs=5, min_size=5, conn=n, poison=True)
       for a, r, w, n in (("copy", 5, 7, 4), ("same handle", 2 * _T + 1, _S + 1, 8))]
    + [pinned_case(kind="wave roots", rows=3, cols=ENTRIES, after="other", conn=n, slabs=s) for n, s in ((8, 1), (4, 3))]
    + [pinned_case(kind="row roots", at=at, rows=3, cols=300, after="other", conn=4 + 4 * (at % 2), slabs=1 + at % 2, poison=True)
       for at in (255, 256, 257)]
    + [pinned_case(kind="full", after="again", rows=_T + 1, cols=_S + 1, slabs=2, poison=True, conn=4),
       pinned_case(kind="empty", after="other", other="planted", rows=_T, cols=_S + 1, slabs=3, poison=True),
       pinned_case(kind="planted", after="other", other="empty", rows=5, cols=2 * _S + 1, slabs=5, poison=True, above=False),
       pinned_case(kind="empty", after="again", rows=5, cols=7, slabs=2, poison=True, conn=4)]
    + [pinned_case(kind="one-set", at=at, after="other", other="full", rows=_T + 1, cols=_S + 1, slabs=1 + i % 3, poison=i % 2 == 0,
                   conn=4 + 4 * (i % 2), above=i % 4 < 2)
       for i, at in enumerate(O.PLACES)]
    + [pinned_case(kind="planted", density=0.3, after="flipped", min_size=4, rows=_T + 1, cols=_S + 3, slabs=2, poison=True, seed=41),
       pinned_case(kind="seams", after="again", min_size=4, rows=_T, cols=_S, slabs=1, conn=4, seed=42, form="species", species="u"),
       pinned_case(kind="planted", threshold=INF, above=True, after="again", rows=_T + 1, cols=_S + 1, slabs=3, poison=True, seed=43),
       pinned_case(kind="lane_runs", threshold=-INF, above=False, after="flipped", rows=5, cols=_S + 1, slabs=5, poison=True, seed=44)]
    + [pinned_case(kind="planted", density=d, after=a, move=mv, threshold=t, above=ab, conn=n, min_size=ms, rows=r, cols=w, slabs=s,
                   poison=True, seed=50 + ms, form=form, species=sp)
       for d, a, mv, t, ab, n, ms, r, w, s, form, sp in (
           (0.5, "flipped", (0, 0), 0.3, True, 8, 0, 2 * _T + 1, _S + 3, 3, "field", "v"),
           (0.593, "moved", (1, -1), 0.0, False, 4, 1, 2 * _T, 2 * _S + 1, 2, "species", "u"),
           (0.5, "seams redrawn", (0, 0), -0.0, True, 8, 2, 2 * _T + 1, _S + 1, 5, "field", "v"),
           (0.3, "again", (0, 0), 2.0 ** -130, True, 4, 3, _T + 1, 2 * _S + 3, 4, "species", "v"),
           (0.5, "seams redrawn", (0, 0), 3.4028235e38, False, 8, 5, 5, _S + 2, 5, "field", "v"),
           (0.593, "flipped", (0, 0), -1.5, False, 8, 5, 3 * _T + 1, 8, 3, "species", "v"),
           (0.5, "moved", (-2, 2), 0.3, True, 4, 2, 4, 4 * _S + 3, 1, "field", "v"))]
    + [pinned_case(form="ensemble", rows=r, cols=w, kind=k, density=0.5, after=a, members=m, first=f, count=n, fence=fence, empties=e,
                   retire=ret, retired=[False, True, True, False, True, False], steps=3, conn=cn, min_size=ms, seed=r + w, species=sp,
                   threshold=t, above=ab)
       for r, w, k, a, m, f, n, fence, e, ret, cn, ms, sp, t, ab in (
           (13, 21, "planted", "flipped", 4, 1, 3, True, (1, 0, 2), False, 8, 0, "v", 0.3, True),
           (37, 53, "seams", "again", 3, 0, 3, False, (1, 0, 2), False, 4, 1, "u", 0.3, False),
           (45, 61, "lane_runs", "moved", 6, 2, 3, True, (0, 1, 0), True, 8, 2, "v", 0.0, True),
           (13, 21, "checkerboard", "seams redrawn", 6, 0, 6, False, (0, 1, 2), True, 4, 0, "v", 0.3, True),
           (_T + 1, _S, "planted", "flipped", 3, 1, 2, False, (2, 0, 1), False, 8, 4, "u", 0.3, True),
           (3, _S + 1, "lane_runs", "copy", 2, 1, 1, True, (0, 0, 0), False, 8, 0, "v", 2.0 ** -130, False),
           (_T, 2 * _S, "rings", "moved", 5, 1, 4, False, (0, 2, 0), True, 4, 5, "v", 0.3, True),
           (37, 53, "planted", "other", 5, 1, 3, True, (1, 1, 1), False, 8, 0, "v", 0.3, True),
           (45, 61, "planted", "again", 2, 0, 2, False, (2, 0, 2), False, 4, 3, "u", -1.5, True),
           (5, 7, "empty", "other", 3, 1, 1, False, (0, 0, 0), False, 8, 0, "v", 0.3, True),
           (_T, _S, "planted", "other", 2, 1, 1, True, (0, 0, 0), False, 4, 0, "u", 0.3, False))])


def _with_examples(form):
    def decorate(test):
        for ex in reversed([e for e in EDGE_EXAMPLES if e["form"] == form]):
            test = example(case=ex)(test)
        return test
    return decorate


def counts_of(c):
    """What the run report counts an example under."""
    legal(c)
    out = ["examples", "form " + c["form"], f"connectivity {c['conn']}", "min_size " + MIN_SIZES[c["min_size"]],
           "after " + (c["kind"] if c["kind"] in LAYOUTS else c["after"]), "sense " + ("above" if c["above"] else "below")]
    out += ["nothing can be set"] if impossible(c["threshold"], c["above"]) else []
    if c["form"] == "ensemble":
        out.append("ensemble load path " + ("ragged" if ragged((c["rows"], c["cols"])) else "16 bytes"))
        out += ["retired members"] if c["retire"] else []
        out += ["fenced"] if c["fence"] else []
        out += ["a member with an empty list"] if any(c["empties"]) else []
    else:
        out.append(f"slabs {c['slabs']}")
        out += ["poisoned"] if c["poison"] else []
        out += ["one-row slabs"] if shortest_slab(c["rows"], c["slabs"]) == 1 and c["slabs"] > 1 else []
    return out


# ---- on the device -----------------------------------------------------------------------------------------------------------
def assert_match(got, want, what):
    """`want`: (before's records, after's records, overlaps) of match_ref.match."""
    rb, ra, ov = want
    assert got.before.records.dtype == got.after.records.dtype == component_list_ref.DTYPE and got.overlaps.dtype == match_ref.OVERLAP, what
    assert same(np.ascontiguousarray(got.before.records), rb), f"{what}: before {got.before.records[:4]} ..., not {rb[:4]} ..."
    assert same(np.ascontiguousarray(got.after.records), ra), f"{what}: after {got.after.records[:4]} ..., not {ra[:4]} ..."
    assert same(np.ascontiguousarray(got.overlaps), ov), f"{what}: overlaps {got.overlaps[:6]} ..., not {ov[:6]} ..."
    assert got.counts() == match_ref.events(rb, ra, ov), what


def same_match(a, b):
    return (same(np.ascontiguousarray(a.before.records), np.ascontiguousarray(b.before.records))
            and same(np.ascontiguousarray(a.after.records), np.ascontiguousarray(b.after.records))
            and same(np.ascontiguousarray(a.overlaps), np.ascontiguousarray(b.overlaps)))


def exchanged(overlaps):
    """The overlaps of the match the other way round: the columns exchanged, sorted again."""
    out = np.zeros(overlaps.shape[0], match_ref.OVERLAP)
    out["before"], out["after"], out["cells"] = overlaps["after"], overlaps["before"], overlaps["cells"]
    return out[np.lexsort((out["after"], out["before"]))]


def check_sums(got, what):
    """The overlaps of one record sum to its size at most, on either side."""
    for side, records in (("before", got.before.records), ("after", got.after.records)):
        total = np.bincount(got.overlaps[side].astype(np.int64), weights=got.overlaps["cells"].astype(np.float64), minlength=records.shape[0])
        assert (total <= records["size"].astype(np.float64)).all(), f"{what}: the overlaps of a {side}-record"


def continues_as_itself(m):
    n = m.before.count
    return (m.after.count == n and m.overlaps.shape[0] == n and np.array_equal(m.overlaps["before"], np.arange(n))
            and np.array_equal(m.overlaps["after"], np.arange(n)) and np.array_equal(m.overlaps["cells"], m.before.sizes))


def run_fields(c, before, after, slabs, poisoned, min_size, want=None, what=""):
    """The match of a field case on a chain of `slabs` slabs, as two fields or as a Species and its snapshot; with `want`
    (match_ref.match's) everything is checked on the way."""
    shape, t, above, conn = (c["rows"], c["cols"]), c["threshold"], c["above"], c["conn"]
    rule = (t, above, conn, min_size)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * slabs))
    ctx = sim.context
    try:
        if c["form"] == "species":
            from .helpers import species_from_arrays

            other = np.full(shape, 0.25, np.float32)
            species = species_from_arrays(sim, *((before, other) if c["species"] == "u" else (other, before)))
            snap = species.snapshot()
            fb = snap.u if c["species"] == "u" else snap.v
            fa = species.in_out()[0 if c["species"] == "u" else 1]
            if after is not before:
                fa.upload(ctx, after)
            match = lambda: species.match_since(snap, t, c["species"], above, conn, min_size)
        else:
            fb = HipConcentration(ctx, shape)
            fb.upload(ctx, before)
            fa = fb
            if c["after"] != "same handle" or after is not before:
                fa = HipConcentration(ctx, shape)
                fa.upload(ctx, after)
            match = lambda: fa.match(ctx, fb, *rule)
        if poisoned:
            for f in {id(fb): fb, id(fa): fa}.values():
                poison(f, O.poison_value(above))
        ctx.sync()
        counters = ctx.stats()
        got = match()
        if want is None:
            return got
        assert_match(got, want, what)
        check_sums(got, what)
        if impossible(t, above):
            assert got.before.count == got.after.count == 0 and got.overlaps.shape == (0,), f"{what}: nothing can be set"
        if MIN_SIZES[c["min_size"]] == "largest + 1":
            assert got.before.count == got.after.count == 0 and got.overlaps.shape == (0,), f"{what}: min_size beyond the largest"
        both = morph_ref.set_cells(before, t, above) & morph_ref.set_cells(after, t, above)
        every = got if min_size == 1 else fa.match(ctx, fb, t, above, conn, 1)
        assert int(every.overlaps["cells"].sum()) == int(both.sum()), f"{what}: the cells set in both planes"
        for f, records in ((fb, got.before.records), (fa, got.after.records)):
            listed = f.component_list(ctx, *rule).records
            assert same(np.ascontiguousarray(listed), np.ascontiguousarray(records)), f"{what}: the component list"
        assert continues_as_itself(fa.match(ctx, fa, *rule)), f"{what}: after against itself"
        back = fb.match(ctx, fa, *rule)
        assert same(np.ascontiguousarray(back.overlaps), exchanged(got.overlaps)), f"{what}: the match the other way round"
        assert same(np.ascontiguousarray(back.before.records), np.ascontiguousarray(got.after.records)), what
        assert ctx.stats() == counters, f"{what}: the context's counters"
        assert same(fb.make_scalar_view(ctx), before) and same(fa.make_scalar_view(ctx), after), f"{what}: the planes"
        return got
    finally:
        ctx.close()


def run_field_case(c):
    shape = (c["rows"], c["cols"])
    before, after = pair_of_planes(c, c["seed"])
    min_size = min_size_of(c, before, after)
    what = (f"match {c['form']} {shape} kind={c['kind']} density={c['density']} at={c['at']} after={c['after']} other={c['other']} "
            f"move={c['move']} seed={c['seed']} threshold={c['threshold']} above={c['above']} conn={c['conn']} min_size={min_size} "
            f"({MIN_SIZES[c['min_size']]}) slabs={c['slabs']} poison={c['poison']} species={c['species']}")
    want = match_ref.match(before, after, c["threshold"], c["above"], c["conn"], min_size)
    got = run_fields(c, before, after, c["slabs"], c["poison"], min_size, want, what)
    if c["slabs"] > 1 or c["poison"]:                        # several slabs, poison: one slab of plain planes
        assert same_match(run_fields(c, before, after, 1, False, min_size), got), f"{what}: one slab without poison"


def run_ensemble_case(c):
    shape, members, first, count = (c["rows"], c["cols"]), c["members"], c["first"], c["count"]
    t, above, conn, sp = c["threshold"], c["above"], c["conn"], c["species"]
    before, after = member_planes(c)
    retired = [m for m in range(members) if c["retired"][m]] if c["retire"] else []
    for m in retired:                                        # a retired member holds the state of the snapshot
        after[m] = before[m]
    what = (f"match of an ensemble of {members} x {shape}, members [{first}, {first + count}) kind={c['kind']} density={c['density']} "
            f"after={c['after']} other={c['other']} move={c['move']} seed={c['seed']} threshold={t} above={above} conn={conn} "
            f"min_size={MIN_SIZES[c['min_size']]} species={sp} fence={c['fence']} empties={c['empties']} retired={retired} "
            f"steps={c['steps'] if c['retire'] else 0}")
    rest = np.full((members,) + shape, 0.25, np.float32)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    lone = Simulation.new(Parameters(), HipArgs(devices=[0]))
    try:
        ctx = sim.context
        ens = sim.make_ensemble(shape, Parameters(), seed=False, members=members)
        ens.upload(*((before, rest) if sp == "u" else (rest, before)))
        snap = ens.snapshot()
        ens.upload(*((after, None) if sp == "u" else (None, after)))
        if c["retire"]:
            ens.retire(retired)
            ens.perform_steps(c["steps"])
            now = ens.u_views() if sp == "u" else ens.result_views()
            for m in retired:
                assert same(now[m], before[m]), f"member {m}: {what}"
            after = now
        min_size = min_size_of(c, before[plain_member(c)], after[plain_member(c)])
        rule = dict(species=sp, threshold=t, above=above, connectivity=conn, min_size=min_size)
        counters = ctx.stats()
        got = ens.matches_since(snap, first, count, **rule)
        whole = ens.matches_since(snap, **rule)
        assert ctx.stats() == counters, f"{what}: the context's counters"
        assert len(got) == count and len(whole) == members, what
        fb, fa = HipConcentration(lone.context, shape), HipConcentration(lone.context, shape)
        for i in range(count):
            m = first + i
            assert_match(got[i], match_ref.match(before[m], after[m], t, above, conn, min_size), f"member {m}: {what}")
            check_sums(got[i], what)
            assert same_match(whole[m], got[i]), f"member {m} of the whole ensemble: {what}"
            fb.upload(lone.context, before[m])
            fa.upload(lone.context, after[m])
            assert same_match(fa.match(lone.context, fb, t, above, conn, min_size), got[i]), f"member {m} as a lone pair of fields: {what}"
            if m in retired:
                assert continues_as_itself(got[i]), f"retired member {m}: {what}"
        now = ens.u_views() if sp == "u" else ens.result_views()
        held = snap.u_views() if sp == "u" else snap.result_views()
        assert same(now, np.ascontiguousarray(after)) and same(held, before), f"{what}: the planes"
        snap.destroy()
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
        SLOWEST[:] = [f'{c["form"]} {c["rows"]} x {c["cols"]} {c["kind"]}, {c["after"]}, {c["members"]} members']


@pytest.fixture(scope="module", autouse=True)
def report():
    SEEN.clear()
    yield
    print("\nmatch property examples: " + ", ".join(f"{k}: {v:.4g}" for k, v in sorted(SEEN.items())) + f" ({SLOWEST[0]})")


# The default keeps the file within 1.25 times the run time of tests/test_gpu_observe_property.py
EXAMPLES = int(os.environ.get("GS_PROPERTY_EXAMPLES_MATCH", "4"))
_SETTINGS = dict(max_examples=EXAMPLES, deadline=None, suppress_health_check=list(HealthCheck))


@settings(**_SETTINGS)
@given(cases("field"))
@_with_examples("field")
def test_any_match_of_two_fields_is_the_reference(built, case):
    run_case(case, "field")


@settings(**_SETTINGS)
@given(cases("species"))
@_with_examples("species")
def test_any_match_since_a_snapshot_is_the_reference(built, case):
    run_case(case, "species")


@settings(**_SETTINGS)
@given(cases("ensemble"))
@_with_examples("ensemble")
def test_any_match_of_ensemble_members_is_the_reference(built, case):
    run_case(case, "ensemble")
