"""Randomised parity of the on-device observables that return floating-point sums -- summaries, comparisons, reduced images,
regional summaries (with regional morphology on the same plane) -- against their restatements in tests/ (summary_ref.summary,
change_ref.change, reduce_ref.reduce, regions_ref.summaries, regions_ref.quads): sums as f64 bit patterns, zero extremes by
value, NaN pixels by position, no tolerance anywhere.  These are the kernels whose results depend on an order of additions: a
wrong lane, a wrong chunk or a leaked pad cell moves a last bit and nothing else.

`cases()` draws

* the shape, each side from the seams of the kernels' units and their neighbours (restated below: a workgroup's four waves,
  a lane's four columns, a wave row of 256 columns, the unroll group of 2048, the reduce kernels' batches of 8 rows and
  tiles of W(f) columns), at most CELL_CAP cells in all of a case's planes and MEMBER_CAP in an ensemble member;
* the values (KINDS: order-sensitive planes, reduce_ref.special_plane, stress fields, a constant, one finite cell, none)
  with NaN, +-inf, +-0, sub-normals and the largest finite values salted in, for some cases exactly on the last column of the
  plane, of a block of 256, of a group of 2048, of a region and of a reduce tile;
* for comparisons what `b` is: another draw, `a` itself, `a` with some cells changed in the last bit, `a` with -0 for +0;
* the reduce factor (any of 2 .. 64, by the kernels' classes) and the region shape;
* the call: HipConcentration's method on one field, the *_fields call with 1 .. 4 fields, or the ensemble's call with a
  range of members (half of the shapes on the load path that is not 16 bytes wide);
* for fields, a chain of 1 .. 5 slabs on one device (one-row slabs occur) and `poison`: the ghost rows of every slab and the
  pitch padding of every row hold NaN or 3.0e38; for ensembles, members outside the range hold the poison value, and half of
  the cases retire some members and advance the rest by an odd number of steps.

Beyond parity, on the device: a region covering the grid equals summarize_fields, the regions' non-finite counts add up and
their minima meet the plane's, regional cells are regions_ref.sizes, one region's morphology equals morphology_fields;
compare(a, a) is zero, compare(a, b) and compare(b, a) agree bit for bit, `differing` counts differing bit patterns; a
constant plane reduces to its constant, reduce=1 is the plane, blocking and overlapped downloads agree; several slabs equal
one, a member equals a lone field with its plane, a retired member holds the plane it was given, 1 .. 4 fields in one call
equal one call each; after the calls the downloaded plane is the uploaded one.  A chain whose seam is no multiple of the region
height or of the factor must refuse (GS_ERR_UNSUPPORTED); the case then runs on one slab.

Parity with a restatement cannot see an error that the restatement shares, so results are also held to exact arithmetic:
in cases of at most EXACT_CELLS cells sum, sum_sq and sum_abs to math.fsum over their terms within the bound of any order
of n - 1 additions, (n - 1) u S / (1 - (n - 1) u) with u = 2^-53 and S the fsum of the terms' magnitudes; and every finite
reduced pixel of every case to the exact mean of its block (integers scaled by 2^149) within that bound on the block's sum
over the count plus half an f32 unit in the last place of the exact mean.  tests/test_float_observe_property_cpu.py checks without a GPU that the
strategy draws legal cases of every kind and that the pinned examples would notice each single fault of a kernel."""
import collections
import math
import os
import time

import numpy as np
import pytest
from hypothesis import HealthCheck, example, given, settings, strategies as st

from grayscott_amd import GsError, HipArgs, HipConcentration, Parameters, Simulation, capi
from grayscott_amd.simulation import (compare_fields, morphology_fields, pinned_empty, region_morphology_fields,
                                      region_summaries_fields, summarize_fields)

from . import change_ref, reduce_ref, regions_ref, summary_ref
from .helpers import stress_fields
from .test_gpu_observe_property import CELL_CAP, MEMBER_CAP, poison, ragged, same, shortest_slab

pytestmark = pytest.mark.gpu

FAMILIES = ["summary", "change", "reduce", "regions"]
FORMS = {"summary": ["field", "fields", "ensemble"], "change": ["field", "fields", "ensemble"], "reduce": ["field"],
         "regions": ["field", "fields"]}
EXACT_CELLS = 20_000

# The kernels' units, restated (grayscott_amd/csrc/gs_summary.hip, gs_change.hip, gs_reduce.hip, gs_regions.hip)
WAVES = 4                               # waves of a workgroup of the row kernels: four rows at a time
LANE_COLS = 4                           # a float4 per lane
BLOCK_COLS = 64 * LANE_COLS             # a wave row: 256 columns
SUM_UNROLL = 8                          # kSumUnroll: blocks of 256 columns (or rows of a narrow region) loaded ahead
GROUP_COLS = BLOCK_COLS * SUM_UNROLL    # the column loop's step: 2048
RED_ROWS = 8                            # kRedRows: rows of a block that gs_reduce_lds_k adds per batch
RED_TILE_COLS, RED_MAX_PIX, RED_VEC_PIX = 1024, 340, 256    # kRedTileCols, kRedMaxPix; a workgroup of gs_reduce_vec_k


def npix(f):
    """Pixels of a workgroup's tile at factor f (gs_launch_reduce)."""
    if f in (2, 4):
        return RED_VEC_PIX
    return min(RED_TILE_COLS // f, RED_MAX_PIX) & ~3


def tile_cols(f):
    return npix(f) * f


def factor_class(f):
    if f in (2, 4):
        return "vec"
    if f > RED_ROWS:
        return "beyond 8"
    return "lds odd" if f % 2 else "lds even"


FACTOR_CLASSES = {"vec": [2, 4], "lds odd": [3, 5, 7], "lds even": [6, 8], "beyond 8": list(range(9, 65))}
ROWS = sorted(set(range(1, 6)) | {m * WAVES + d for m in (1, 2, 3) for d in (-1, 0, 1)}
              | {m * k + d for k in (SUM_UNROLL, 2 * SUM_UNROLL) for m in (1, 2) for d in (-1, 0, 1)})
COLS = sorted(set(range(1, 10)) | {m * BLOCK_COLS + d for m in (1, 2) for d in range(-5, 6)}
              | {m * GROUP_COLS + d for m in (1, 2) for d in range(-5, 6)})
WIDE_ROWS = 5                           # the widest planes (two groups of 2048 columns) have at most five rows
REDUCE_CELLS = 150_000                  # reduce cases stay below this (the exact check is per pixel)
REGIONS_MAX = 320                       # regions of a plane in a case (the reference crops every one)
REGION_WIDTHS = [16, 20, 60, 64, 252, 256, 260, 2044, 2048, 2052, "wider"]
REGION_HEIGHTS = [1, 2, 7, 8, 9, 15, 16, 17, "rows", "rows + 1"]
ENSEMBLE_SHAPES = [(5, 301), (2, 1031), (1, 2101), (1, 4099)]       # pinned: the load path that is not 16 bytes wide
KINDS = ["order", "special", "stress", "constant", "one-finite", "no-finite"]
B_KINDS = ["other", "same", "lastbit", "negzero"]
SALT = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38, 3.4028235e38, -3.4028235e38],
                np.float32)
SALT_SMALL = 10                         # SALT[:SALT_SMALL]: without the largest values, which swallow every fold order
CONSTANTS = [0.1, -3.0e-41, 1.0, 3.4028235e38, -0.75]
POISONS = [float("nan"), 3.0e38]
MORPH_THRESHOLDS = [0.3, 0.0]

SEEN = collections.Counter()


def rows_ok(rows, cols):
    return rows <= WIDE_ROWS or cols <= GROUP_COLS + 5


def region_of(c):
    """(rh, rw) of a case as numbers."""
    rh = {"rows": c["rows"], "rows + 1": c["rows"] + 1}.get(c["rh"], c["rh"])
    rw = max(16, (c["cols"] + 3) // 4 * 4 + 4) if c["rw"] == "wider" else c["rw"]
    return int(rh), int(rw)


def region_form(c):
    w = min(region_of(c)[1], c["cols"])
    rw = region_of(c)[1]
    if rw < BLOCK_COLS:
        return "narrow"
    if rw == BLOCK_COLS:
        return "exactly 256"
    return "wider than 2048" if w > GROUP_COLS else "wide"


def seams_of(rows, slabs):
    return [k * rows // slabs for k in range(1, slabs)]


def refuses(c, slabs=None):
    """Must the library refuse the case's chain?"""
    slabs = c["slabs"] if slabs is None else slabs
    if slabs == 1 or c["form"] == "ensemble":
        return False
    if c["family"] == "regions":
        return any(s % region_of(c)[0] for s in seams_of(c["rows"], slabs))
    if c["family"] == "reduce":
        return not reduce_ref.slab_rule(c["rows"], slabs, c["f"])
    return False


def pinned_case(family, **kw):
    base = dict(family=family, form="field", rows=9, cols=261, seed=1, kind="order", salt=0, edges=False, b_kind="other",
                slabs=1, poison=False, poison_value=0, nfields=1, f=3, rh=8, rw=64, members=1, first=0, count=1, retire=False,
                retired=[False] * 6, steps=1, above=True)
    base.update(kw)
    return base


@st.composite
def cases(draw, family=None):
    family = family or draw(st.sampled_from(FAMILIES))
    form = draw(st.sampled_from(FORMS[family]))
    c = pinned_case(family, form=form, seed=draw(st.integers(0, 2 ** 16)), kind=draw(st.sampled_from(KINDS)),
                    salt=draw(st.integers(0, 2)), edges=draw(st.booleans()), b_kind=draw(st.sampled_from(B_KINDS)),
                    poison=draw(st.booleans()), poison_value=draw(st.integers(0, 1)), retire=draw(st.booleans()),
                    retired=[draw(st.booleans()) for _ in range(6)], steps=draw(st.sampled_from([1, 3, 5])),
                    above=draw(st.booleans()))
    slabs = draw(st.integers(1, 5))
    refuse = draw(st.integers(0, 7)) == 5           # a chain that may refuse: one in eight, else one made to fit
    if form == "ensemble":
        want_ragged = draw(st.booleans())
        if want_ragged and draw(st.integers(0, 3)) == 0:
            rows, cols = draw(st.sampled_from(ENSEMBLE_SHAPES))
        else:
            rows = draw(st.sampled_from(ROWS))
            cols = draw(st.sampled_from([x for x in COLS if rows * x <= MEMBER_CAP and rows_ok(rows, x)
                                         and ragged((rows, x)) == want_ragged]))
        members = draw(st.integers(1, 6))
        first = draw(st.integers(0, members - 1))
        c.update(rows=rows, cols=cols, members=members, first=first, count=draw(st.integers(1, members - first)))
        return c
    if family == "reduce":
        f = draw(st.sampled_from(FACTOR_CLASSES[draw(st.sampled_from(sorted(FACTOR_CLASSES)))]))
        w = tile_cols(f)
        low = f + 1 if f > RED_ROWS else 1
        if slabs > 1 and not refuse:                # every slab begins at a multiple of f
            rows = slabs * f * draw(st.integers(1, 2)) + draw(st.integers(0, 1))
        else:
            rows = draw(st.sampled_from(sorted({k * f + d for k in (1, 2, 3) for d in (-1, 0, 1) if k * f + d >= low})))
        wide = [w - 1, w, w + 1, 2 * w + 1]           # half of the widths from the workgroup's tile
        if draw(st.booleans()) or rows * (w - 1) > REDUCE_CELLS:
            wide = sorted({k * f + d for k in (1, 2, 3) for d in (-1, 1)} | set(COLS))
        cols = draw(st.sampled_from([x for x in wide if 0 < x and rows * x <= REDUCE_CELLS and rows_ok(rows, x)]))
        c.update(f=f)
    else:
        rows = draw(st.sampled_from(ROWS))
        cols = draw(st.sampled_from([x for x in COLS if rows_ok(rows, x)]))
    c.update(rows=rows, cols=cols, slabs=min(slabs, rows))
    if family == "regions":
        few = [w for w in REGION_WIDTHS if regions_ref.grid((rows, cols), (1, region_of(dict(c, rw=w))[1]))[1] <= REGIONS_MAX // 4]
        if cols > GROUP_COLS and draw(st.booleans()):   # a region wider than the column loop's step
            few = [2052, "wider"]
        c.update(rw=draw(st.sampled_from(few)))
        rc = regions_ref.grid((rows, cols), region_of(dict(c, rh=1)))[1]
        fit = [h for h in REGION_HEIGHTS if -(-rows // region_of(dict(c, rh=h))[0]) * rc <= REGIONS_MAX]
        c.update(rh=draw(st.sampled_from(fit)))
        if refuses(c) and not refuse:                # made to fit: another height, or one slab
            fitting = [h for h in fit if not refuses(dict(c, rh=h))]
            if fitting and draw(st.booleans()):
                c.update(rh=draw(st.sampled_from(fitting)))
            else:
                c.update(slabs=1)
    cells = rows * cols
    c.update(nfields=draw(st.integers(1, max(1, min(4, CELL_CAP // (cells * (2 if family == "change" else 1)))))) if form == "fields" else 1)
    return c


def legal(c):
    """(the slabs a drawn case runs on, is its own chain refused).  Also the strategy's own check."""
    rows, cols, form, family = c["rows"], c["cols"], c["form"], c["family"]
    assert family in FAMILIES and form in FORMS[family] and c["kind"] in KINDS and c["b_kind"] in B_KINDS
    assert c["salt"] in (0, 1, 2) and c["poison_value"] in (0, 1) and c["steps"] % 2 == 1 and rows >= 1 and cols >= 1
    assert rows_ok(rows, cols)
    assert 1 <= c["slabs"] <= min(5, rows) and 1 <= c["nfields"] <= 4 and (form == "fields" or c["nfields"] == 1)
    assert 1 <= c["members"] <= 6 and 0 <= c["first"] and c["count"] >= 1 and c["first"] + c["count"] <= c["members"]
    if form == "ensemble":
        assert rows * cols <= MEMBER_CAP and c["slabs"] == 1
        return 1, False
    assert rows * cols * c["nfields"] * (2 if family == "change" else 1) <= CELL_CAP
    if family == "reduce":
        assert 2 <= c["f"] <= 64 and rows * cols <= REDUCE_CELLS and (c["f"] <= RED_ROWS or rows >= c["f"] + 1)
    if family == "regions":
        rh, rw = region_of(c)
        assert rh >= 1 and rw >= 16 and rw % 4 == 0 and c["rw"] in REGION_WIDTHS and c["rh"] in REGION_HEIGHTS
        rr, rc = regions_ref.grid((rows, cols), (rh, rw))
        assert rr * rc <= REGIONS_MAX
    refused = refuses(c)
    return (1 if refused else c["slabs"]), refused


# ---- values ----------------------------------------------------------------------------------------------------------------
def edge_columns(c):
    """The last column of the plane, of a block of 256, of a group of 2048, of a region and of a reduce tile."""
    cols = c["cols"]
    marks = {cols - 1, BLOCK_COLS - 1, 2 * BLOCK_COLS - 1, GROUP_COLS - 1, 2 * GROUP_COLS - 1}
    if c["family"] == "regions":
        marks |= {region_of(c)[1] - 1, 2 * region_of(c)[1] - 1}
    if c["family"] == "reduce":
        marks |= {tile_cols(c["f"]) - 1, 2 * tile_cols(c["f"]) - 1}
    return sorted(x for x in marks if 0 <= x < cols)


def base_plane(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "order":
        return change_ref.order_sensitive(shape, seed)[0]
    if kind == "special":
        return reduce_ref.special_plane(shape, seed)
    if kind == "stress":
        return stress_fields(shape, seed)[0]
    if kind == "constant":
        return np.full(shape, CONSTANTS[seed % len(CONSTANTS)], np.float32)
    a = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, size=shape)]
    if kind == "one-finite":
        a[int(rng.integers(shape[0])), int(rng.integers(shape[1]))] = np.float32([1e-45, -0.375, 3.4028235e38][seed % 3])
    return a


def make_plane(c, seed):
    shape = (c["rows"], c["cols"])
    a = np.ascontiguousarray(base_plane(c["kind"], shape, seed), np.float32)
    rng = np.random.default_rng(seed + 77)
    if c["salt"] and c["kind"] not in ("one-finite", "no-finite"):
        odd = SALT[:SALT_SMALL] if c["salt"] == 1 else SALT
        n = min(2 * len(odd), a.size // 4)
        a.flat[rng.choice(a.size, size=n, replace=False)] = np.resize(odd[rng.permutation(len(odd))], n)
        if c["edges"]:
            for i, col in enumerate(edge_columns(c)):
                a[int(rng.integers(shape[0])), col] = odd[(i + seed) % len(odd)]
    return a


def pair_of(c, seed):
    """(a, b) of a comparison; b is None where `a` itself is compared."""
    shape = (c["rows"], c["cols"])
    a = make_plane(c, seed)
    rng = np.random.default_rng(seed + 99)
    kind = c["b_kind"]
    if kind == "same":
        return a, None
    if kind == "other":
        if c["kind"] == "order" and not c["salt"]:
            return change_ref.order_sensitive(shape, seed)
        return a, make_plane(c, seed + 1000)
    k = max(1, min(7, a.size // 3))
    at = rng.choice(a.size, size=k, replace=False)
    if kind == "lastbit":
        b = a.copy()
        b.view(np.uint32).flat[at] ^= np.uint32(1)
        return a, b
    a.flat[at] = np.float32(0.0)
    b = a.copy()
    b.flat[at] = np.float32(-0.0)
    return a, b


def member_planes(c, shift=0):
    """[species][member] planes of an ensemble case: the members of the range carry the case's values, the others hold the
    poison value in every cell."""
    planes = np.empty((2, c["members"], c["rows"], c["cols"]), np.float32)
    for s in (0, 1):
        for m in range(c["members"]):
            if c["first"] <= m < c["first"] + c["count"]:
                planes[s, m] = make_plane(c, c["seed"] + 2 * m + s + shift)
            else:
                planes[s, m] = np.float32(POISONS[c["poison_value"]])
    return planes


def member_pairs(c):
    """(a, b) as [species][member] planes of a comparison over an ensemble's members."""
    a = member_planes(c)
    b = a.copy()
    for s in (0, 1):
        for m in range(c["first"], c["first"] + c["count"]):
            x, y = pair_of(c, c["seed"] + 2 * m + s)
            a[s, m], b[s, m] = x, (x if y is None else y)
    return a, b


# ---- exact arithmetic ------------------------------------------------------------------------------------------------------
U53 = 2.0 ** -53


def sum_bound(n, magnitude):
    """|fl(sum) - sum| of n terms added in any order: (n - 1) u S / (1 - (n - 1) u)."""
    return (n - 1) * U53 * magnitude / (1.0 - (n - 1) * U53) if n > 1 else 0.0


def assert_sum(got, terms, what):
    terms = np.asarray(terms, np.float64).ravel()
    exact, magnitude = math.fsum(terms), math.fsum(np.abs(terms))
    bound = sum_bound(terms.size, magnitude)
    assert abs(float(got) - exact) <= bound, f"{what}: {float(got)!r}, exactly {exact!r}: off by more than {bound!r}"


def assert_summary_exact(got, plane, what):
    x = plane[np.isfinite(plane)].astype(np.float64)
    g = summary_ref.as_dict(got)
    assert_sum(g["sum"], x, what + " sum")
    assert_sum(g["sum_sq"], x * x, what + " sum_sq")       # (a 24-bit significand squared is exact in f64)


def assert_change_exact(got, a, b, what):
    both = np.isfinite(a) & np.isfinite(b)
    d = a[both].astype(np.float64) - b[both].astype(np.float64)
    g = change_ref.as_dict(got)
    assert_sum(g["sum_abs"], np.abs(d), what + " sum_abs")
    assert_sum(g["sum_sq"], d * d, what + " sum_sq")


def scaled_ints(a):
    """Finite f32 values as Python integers, times 2^149 (every f32 is such an integer)."""
    m, e = np.frexp(np.asarray(a, np.float32).astype(np.float64))
    mant = (m * 2.0 ** 24).astype(np.int64)                 # 24 bits: exact
    shift = e.astype(np.int64) - 24 + 149                   # below 0 for sub-normals alone, whose low bits are 0 then
    return [(int(x) << s) if s >= 0 else (int(x) >> -s) for x, s in zip(mant.ravel().tolist(), shift.ravel().tolist())]


def assert_reduce_exact(got, plane, f, what):
    """Every finite pixel against the exact mean of its block, in integers scaled by 2^149:
    |got - total / count| <= (n - 1) S / ((2^53 - (n - 1)) count) + ulp32(mean) / 2, multiplied out."""
    rows, cols = plane.shape
    orows, ocols = got.shape
    fin = np.isfinite(plane)
    values = np.array(scaled_ints(np.where(fin, plane, np.float32(0))), object).reshape(rows, cols)
    pad = np.zeros((orows * f, ocols * f), object)
    pad[:rows, :cols] = values
    blocks = pad.reshape(orows, f, ocols, f)
    total, magnitude = blocks.sum(axis=(1, 3)), np.abs(blocks).sum(axis=(1, 3))
    lost = np.ones((orows * f, ocols * f), bool)
    lost[:rows, :cols] = fin
    whole = lost.reshape(orows, f, ocols, f).all(axis=(1, 3)) & np.isfinite(got)
    pixels = np.array(scaled_ints(np.where(whole, got, np.float32(0))), object).reshape(got.shape)
    for R, C in np.argwhere(whole):
        R, C = int(R), int(C)
        n = min(f, rows - R * f) * min(f, cols - C * f)
        t, s, g = int(total[R, C]), int(magnitude[R, C]), int(pixels[R, C])
        q = abs(t) // n
        e = q.bit_length() - 1 - 149 if q else -149
        ulp = 1 << (max(e, -126) - 23 + 149)
        d = (1 << 53) - (n - 1)
        assert 2 * d * abs(g * n - t) <= 2 * (n - 1) * s + n * d * ulp, f"{what}: pixel ({R}, {C}) = {got[R, C]!r} of {n} cells"


# ---- pinned examples ------------------------------------------------------------------------------------------------------
_G, _B = GROUP_COLS, BLOCK_COLS
# The cases that must always run, per family:
# - widths beyond one and two unroll groups with a ragged tail (2053, 4101 columns), on the 16-byte path and -- ensembles of
#   301, 1031, 2101 and 4099 columns -- on the other; widths on either side of a block of 256; one to four columns;
# - row counts on either side of a workgroup's four waves and of 8 and 16; chains of 1 .. 5 slabs with one-row slabs;
# - order-sensitive values, where another fold moves last bits; special values salted in and put on the last columns of
#   every unit; a constant, one finite cell, none; NaN and 3.0e38 in the ghost rows and the pitch padding;
# - comparisons with a itself, with last bits changed, with -0 for +0;
# - reduce factors 2 .. 8, 9 .. 15 (a partial second batch of rows), 16, 17, 33, 63, 64, at W - 1, W, W + 1 and 2 W + 1 columns;
# - regions 16 .. 2052 columns wide and wider than the plane, 1 .. 17 rows high and higher than the plane, chains that
#   must refuse.
EDGE_EXAMPLES = (
    [pinned_case(f, rows=r, cols=w, kind=k, salt=s, edges=e, slabs=n, poison=p, poison_value=v, seed=seed, b_kind=b)
     for f in ("summary", "change")
     for r, w, k, s, e, n, p, v, seed, b in (
         (9, _G + 5, "order", 0, False, 1, True, 0, 3, "other"), (5, 2 * _G + 5, "order", 0, False, 5, True, 1, 4, "other"),
         (4, _G + 1, "order", 1, True, 2, False, 0, 5, "other"), (33, _B + 5, "order", 2, True, 2, True, 1, 6, "lastbit"),
         (17, 2 * _B + 1, "special", 0, False, 3, True, 0, 7, "negzero"), (15, _B - 1, "order", 1, True, 4, True, 1, 8, "other"),
         (4, _G - 5, "one-finite", 0, False, 1, True, 0, 9, "other"), (3, 7, "no-finite", 0, False, 3, True, 1, 10, "other"),
         (7, 3, "stress", 1, False, 1, True, 0, 11, "same"), (1, 1, "stress", 0, False, 1, True, 0, 12, "lastbit"),
         (16, _B, "order", 0, False, 1, False, 0, 13, "other"), (2, 5, "constant", 0, False, 1, True, 0, 16, "lastbit"),
         (6, _B + 3, "constant", 0, False, 2, True, 1, 26, "lastbit"))]
    + [pinned_case(f, form="fields", rows=r, cols=w, kind=k, salt=s, edges=True, slabs=n, poison=True, poison_value=v, nfields=nf,
                   seed=seed, b_kind=b)
       for f in ("summary", "change")
       for r, w, k, s, n, v, nf, seed, b in ((8, _G + 3, "order", 1, 2, 0, 2, 21, "other"), (5, 2 * _B - 3, "special", 0, 5, 1, 4, 22, "other"),
                                             (12, 9, "constant", 1, 3, 0, 3, 23, "negzero"), (2, _B + 2, "stress", 2, 1, 1, 1, 24, "same"))]
    + [pinned_case(f, form="ensemble", rows=r, cols=w, kind=k, salt=s, edges=e, members=m, first=a, count=n, retire=ret,
                   retired=[False, True, True, False, True, False], steps=3, poison_value=v, seed=seed, b_kind=b)
       for f in ("summary", "change")
       for r, w, k, s, e, m, a, n, ret, v, seed, b in (
           (5, 301, "order", 0, False, 4, 1, 2, False, 0, 31, "other"), (2, 1031, "order", 1, True, 3, 0, 3, True, 1, 32, "other"),
           (1, 2101, "order", 0, False, 6, 2, 3, True, 0, 33, "lastbit"), (1, 4099, "order", 1, True, 2, 1, 1, False, 1, 34, "other"),
           (8, _G + 4, "order", 0, False, 3, 1, 1, False, 0, 35, "other"), (3, _B, "special", 2, True, 2, 0, 1, True, 1, 36, "negzero"))]
    + [pinned_case("reduce", rows=r, cols=w, f=f, kind=k, salt=s, edges=e, slabs=n, poison=p, poison_value=v, seed=f + r)
       for f, r, w, k, s, e, n, p, v in (
           (2, 9, 2 * tile_cols(2) + 1, "special", 0, False, 1, True, 0), (4, 17, tile_cols(4) + 1, "special", 1, True, 2, True, 1),
           (3, 10, tile_cols(3) + 1, "special", 0, False, 3, True, 0), (5, 11, 2 * tile_cols(5) + 1, "special", 1, True, 1, True, 1),
           (6, 13, tile_cols(6) + 1, "special", 0, False, 2, True, 0), (6, 12, tile_cols(6) - 1, "order", 1, False, 2, True, 1),
           (7, 15, tile_cols(7) + 1, "special", 0, False, 1, True, 1), (8, 17, tile_cols(8), "special", 2, True, 2, True, 0),
           (9, 19, tile_cols(9) + 1, "special", 0, False, 2, True, 1), (12, 25, tile_cols(12) + 1, "special", 1, True, 1, True, 0),
           (15, 31, 2 * tile_cols(15) + 1, "special", 0, False, 1, True, 1), (10, 21, 29, "order", 1, False, 2, False, 0),
           (16, 33, tile_cols(16) + 1, "special", 0, False, 2, True, 0), (17, 35, tile_cols(17) + 1, "special", 1, True, 1, True, 1),
           (33, 67, tile_cols(33) + 1, "special", 0, False, 2, True, 0), (63, 64, tile_cols(63) + 1, "special", 0, False, 1, True, 1),
           (64, 65, tile_cols(64) - 1, "special", 1, True, 1, True, 0), (13, 27, _G + 5, "constant", 0, False, 1, True, 1),
           (3, 5, _G + 5, "one-finite", 0, False, 5, True, 0), (11, 12, 23, "stress", 1, False, 1, True, 1),
           (5, 5, 7, "stress", 0, False, 5, True, 1), (7, 8, 2 * tile_cols(7) + 1, "order", 2, True, 1, False, 0))]
    + [pinned_case("regions", form=form, rows=r, cols=w, rh=rh, rw=rw, kind=k, salt=s, edges=e, slabs=n, poison=True, poison_value=v,
                   nfields=nf, seed=seed, above=seed % 2 == 0)
       for form, r, w, rh, rw, k, s, e, n, v, nf, seed in (
           ("field", 9, _G + 5, 8, 2052, "order", 0, False, 1, 0, 1, 41), ("field", 5, 2 * _G + 5, 2, "wider", "order", 1, True, 1, 1, 1, 42),
           ("field", 4, 2 * _G + 5, 1, 2048, "order", 0, False, 4, 0, 1, 43), ("fields", 17, _B + 5, 8, 16, "order", 1, True, 1, 1, 2, 44),
           ("field", 33, 2 * _B + 1, 16, 256, "order", 0, False, 2, 0, 1, 45), ("field", 16, 2 * _B + 5, 7, 260, "special", 1, True, 1, 1, 1, 46),
           ("fields", 24, _B + 4, 8, 252, "order", 2, True, 3, 0, 3, 47), ("field", 17, _B - 1, 9, 60, "order", 0, False, 1, 1, 1, 48),
           ("field", 33, 2 * _B + 3, 17, 64, "special", 0, False, 1, 0, 1, 49), ("field", 31, _B, 15, 20, "order", 1, True, 1, 1, 1, 50),
           ("field", 5, 9, "rows + 1", 16, "stress", 1, False, 1, 0, 1, 51), ("field", 5, 2 * _B, 1, 2044, "order", 0, False, 5, 1, 1, 52),
           ("field", 16, _B + 1, 16, 64, "order", 0, False, 3, 0, 1, 53), ("fields", 9, 7, 2, "wider", "no-finite", 0, False, 2, 1, 4, 54),
           ("field", 12, _G - 5, "rows", 2048, "one-finite", 0, False, 1, 0, 1, 55), ("field", 8, _B + 2, 8, 64, "constant", 1, True, 2, 1, 1, 56),
           ("field", 3, _G + 3, 2, "wider", "constant", 0, False, 1, 0, 1, 61))])


def _with_examples(family):
    def decorate(test):
        for ex in reversed([e for e in EDGE_EXAMPLES if e["family"] == family]):
            test = example(case=ex)(test)
        return test
    return decorate


def counts_of(c):
    """What the run report counts an example under."""
    slabs, refused = legal(c)
    family, cols = c["family"], c["cols"]
    out = ["examples", family, f"{family} form {c['form']}"]
    tail = cols > GROUP_COLS and cols % GROUP_COLS != 0
    if c["form"] == "ensemble":
        path = "ragged" if ragged((c["rows"], cols)) else "16 bytes"
        out.append("ensemble load path " + path)
        out += ["retired members"] if c["retire"] else []
        out += [f"beyond 2048 with a ragged tail, {path}"] if tail else []
    else:
        out.append(f"slabs {slabs}")
        out += ["poisoned"] if c["poison"] else []
        out += ["one-row slabs"] if shortest_slab(c["rows"], slabs) == 1 and slabs > 1 else []
        out += ["refused chains"] if refused else []
        out += ["beyond 2048 with a ragged tail, 16 bytes"] if tail and family != "reduce" else []
    if family == "reduce":
        out += [f"factor {c['f']}", "factor class " + factor_class(c["f"]), "reduce form blocking", "reduce form overlapped"]
    if family == "regions":
        out.append("region form " + region_form(c))
    return out


# ---- on the device ----------------------------------------------------------------------------------------------------------
def poison_of(c, negate=False):
    value = POISONS[c["poison_value"]]
    return -value if negate else value


def upload_fields(ctx, c, planes, negate=False):
    out = []
    for p in planes:
        f = HipConcentration(ctx, p.shape)
        f.upload(ctx, p)
        if c["poison"]:
            poison(f, poison_of(c, negate))
        out.append(f)
    ctx.sync()
    return out


def field_inputs(c):
    """The planes of a field case: [a] per field, and for comparisons [b or None] too."""
    if c["family"] == "change":
        pairs = [pair_of(c, c["seed"] + 10 * i) for i in range(c["nfields"])]
        return [a for a, _ in pairs], [b for _, b in pairs]
    return [make_plane(c, c["seed"] + 10 * i) for i in range(c["nfields"])], None


def region_results(ctx, c, fields, one_by_one):
    region = region_of(c)
    thresholds, above = MORPH_THRESHOLDS, c["above"]
    if one_by_one:
        return ([f.region_summaries(ctx, region) for f in fields], [f.region_morphology(ctx, region, thresholds, above) for f in fields])
    return (region_summaries_fields(ctx, fields, region),
            region_morphology_fields(ctx, fields, region, [thresholds] * len(fields), [above] * len(fields)))


def observe(ctx, c, fields, others, one_by_one):
    """The case's observable of every field: a list of results (regions: a pair of lists)."""
    family = c["family"]
    if family == "summary":
        return [f.summary(ctx) for f in fields] if one_by_one else summarize_fields(ctx, fields)
    if family == "change":
        return [f.change_from(ctx, g) for f, g in zip(fields, others)] if one_by_one else compare_fields(ctx, fields, others)
    if family == "reduce":
        return [f.make_scalar_view(ctx, reduce=c["f"]) for f in fields]
    return region_results(ctx, c, fields, one_by_one)


def same_result(family, got, want):
    if family == "summary":
        return summary_ref.same(got, want)
    if family == "change":
        return change_ref.same(got, want)
    if family == "reduce":
        return reduce_ref.same_bits(got, want)
    (gs, gm), (ws, wm) = got, want
    return (regions_ref.same_summaries(gs, ws) and len(gm) == len(wm)
            and all(same(np.ascontiguousarray(g.quads), w) for g, w in zip(gm, wm)))


def reference(c, a, b=None):
    family = c["family"]
    if family == "summary":
        return summary_ref.summary(a)
    if family == "change":
        return change_ref.change(a, a if b is None else b)
    if family == "reduce":
        return reduce_ref.reduce(a, c["f"])
    region = region_of(c)
    return regions_ref.summaries(a, region), [regions_ref.quads(a, region, t, c["above"]) for t in MORPH_THRESHOLDS]


def identical(family, x, y):
    """Two device results, bit for bit."""
    if family == "summary":
        return summary_ref.same(x, y)
    if family == "change":
        return change_ref.same(x, y)
    if family == "reduce":
        return reduce_ref.same_bits(x, y)
    (xs, xm), (ys, ym) = x, y
    return (all(getattr(xs, f).tobytes() == getattr(ys, f).tobytes() for f in summary_ref.FIELDS + ("size",))
            and all(same(p.quads, q.quads) for p, q in zip(xm, ym)))


def per_field(family, results, i):
    return (results[0][i], results[1][i]) if family == "regions" else results[i]


def check_relations(ctx, c, fields, others, planes, others_planes, got, slabs, what):
    family, f0, a = c["family"], fields[0], planes[0]
    rows, cols = a.shape
    cover = (rows, max(16, (cols + 3) // 4 * 4))
    if family in ("summary", "regions"):
        whole = summarize_fields(ctx, fields[:1])[0]
        assert summary_ref.same(whole, summary_ref.summary(a)), what
        if slabs == 1:                                       # a region covering the grid: the whole-grid calls
            rs = f0.region_summaries(ctx, cover)
            assert rs.sum.shape == (1, 1) and summary_ref.same(rs.at(0, 0), whole) and rs.at(0, 0).size == whole.size, what
            rm = f0.region_morphology(ctx, cover, MORPH_THRESHOLDS, c["above"])
            mf = morphology_fields(ctx, fields[:1], [MORPH_THRESHOLDS], [c["above"]])[0]
            assert all(same(np.ascontiguousarray(m.quads[0, 0]), np.ascontiguousarray(w.quads)) for m, w in zip(rm, mf)), what
        if family == "regions":
            rs = per_field(family, got, 0)[0]
            assert int(rs.nonfinite.sum()) == whole.nonfinite and float(rs.min.min()) == whole.min, what
            assert float(rs.max.max()) == whole.max, what
            assert np.array_equal(rs.size, regions_ref.sizes(a.shape, region_of(c))), what
            assert all(np.array_equal(m.cells, rs.size) for m in per_field(family, got, 0)[1]), what
    if family == "change":
        b_field, b = others[0], (a if others_planes[0] is None else others_planes[0])
        zero = f0.change_from(ctx, f0)
        assert zero.differing == 0 and zero.equal and all(change_ref.bits(getattr(zero, k)) == 0 for k in ("sum_abs", "sum_sq", "max_abs")), what
        assert zero.nonfinite == int(np.count_nonzero(~np.isfinite(a))), what
        back = b_field.change_from(ctx, f0)
        assert change_ref.same(back, got[0]), f"b against a: {change_ref.as_dict(back)}, not {change_ref.as_dict(got[0])}: {what}"
        assert got[0].differing == int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))), what
    if family == "reduce":
        image = pinned_empty(got[0].shape)
        image[...] = -7.0
        f0.write_scalar_view_after(ctx, image, reduce=c["f"])
        ctx.download_wait()
        assert reduce_ref.same_bits(np.array(image), got[0]), f"overlapped against blocking: {what}"
        assert same(f0.make_scalar_view(ctx, reduce=1), a), what
        if c["kind"] == "constant" and not c["salt"]:
            assert (got[0] == a[0, 0]).all(), f"a constant plane: {what}"


def check_exact(c, got, planes, others_planes, what):
    family = c["family"]
    for i, a in enumerate(planes):
        if a.size > EXACT_CELLS and family != "reduce":
            continue
        g = per_field(family, got, i)
        if family == "summary":
            assert_summary_exact(g, a, what)
        elif family == "change":
            assert_change_exact(g, a, a if others_planes[i] is None else others_planes[i], what)
        elif family == "reduce":
            assert_reduce_exact(g, a, c["f"], what)
        else:
            for at, crop in regions_ref.crops(a, region_of(c)):
                assert_summary_exact(g[0].at(*at), crop, f"{what} region {at}")


def run_field_case(c):
    slabs, refused = legal(c)
    family, shape = c["family"], (c["rows"], c["cols"])
    planes, others_planes = field_inputs(c)
    what = (f"{family} {c['form']} {shape} x {c['nfields']} kind={c['kind']} salt={c['salt']} edges={c['edges']} seed={c['seed']} "
            f"b={c['b_kind']} f={c['f']} region={region_of(c)} above={c['above']} slabs={slabs} (drawn {c['slabs']}) "
            f"poison={poison_of(c) if c['poison'] else None}")
    want = [reference(c, a, None if others_planes is None else others_planes[i]) for i, a in enumerate(planes)]

    def fields_on(ctx):
        fields = upload_fields(ctx, c, planes)
        others = None
        if family == "change":
            made = iter(upload_fields(ctx, c, [b for b in others_planes if b is not None], negate=True))
            others = [f if b is None else next(made) for f, b in zip(fields, others_planes)]
        return fields, others

    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * c["slabs"]))
    try:
        ctx = sim.context
        fields, others = fields_on(ctx)
        if refused:
            with pytest.raises(GsError) as e:
                observe(ctx, c, fields, others, True)
            assert e.value.code == capi.GS_ERR_UNSUPPORTED, what
            ctx.close()
            sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
            ctx = sim.context
            fields, others = fields_on(ctx)
        got = observe(ctx, c, fields, others, one_by_one=c["form"] == "field")
        for i, w in enumerate(want):
            g = per_field(family, got, i)
            assert same_result(family, g, w), f"field {i}: {g if family != 'regions' else 'regions'}, not {w if family != 'regions' else 'theirs'}: {what}"
        if c["form"] == "fields":                            # 1 .. 4 fields in one call: one call each
            alone = observe(ctx, c, fields, others, one_by_one=True)
            assert all(identical(family, per_field(family, got, i), per_field(family, alone, i)) for i in range(len(fields))), f"one call each: {what}"
        check_relations(ctx, c, fields, others, planes, others_planes, got, slabs, what)
        check_exact(c, got, planes, others_planes, what)
        for f, p in zip(fields + (others or []), planes + (others_planes or [])):   # the poison is where it belongs:
            assert p is None or same(f.make_scalar_view(ctx), p), what              # the cells are the planes'
    finally:
        sim.context.close()
    if slabs > 1:                                            # several slabs: one
        sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
        try:
            plain = dict(c, poison=False)
            fields = upload_fields(sim.context, plain, planes[:1])
            others = None
            if family == "change":
                others = fields if others_planes[0] is None else upload_fields(sim.context, plain, others_planes[:1])
            one = observe(sim.context, c, fields, others, one_by_one=True)
            assert identical(family, per_field(family, one, 0), per_field(family, got, 0)), f"one slab: {what}"
        finally:
            sim.context.close()


def run_ensemble_case(c):
    legal(c)
    family, shape, first, count = c["family"], (c["rows"], c["cols"]), c["first"], c["count"]
    if family == "change":
        (u, v), (bu, bv) = member_pairs(c)
    else:
        u, v = member_planes(c)
    retired = [m for m in range(c["members"]) if c["retired"][m]] if c["retire"] else []
    what = (f"{family} ensemble of {c['members']} x {shape}, members [{first}, {first + count}) kind={c['kind']} salt={c['salt']} "
            f"edges={c['edges']} seed={c['seed']} b={c['b_kind']} poison={poison_of(c)} retired={retired} "
            f"steps={c['steps'] if c['retire'] else 0}")
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    lone = Simulation.new(Parameters(), HipArgs(devices=[0]))
    try:
        ens = sim.make_ensemble(shape, Parameters(), seed=False, members=c["members"])
        ens.upload(u, v)
        ref = None
        if family == "change":
            ref = sim.make_ensemble(shape, Parameters(), seed=False, members=c["members"])
            ref.upload(bu, bv)
        if c["retire"]:
            ens.retire(retired)
            ens.perform_steps(c["steps"])
            now_u, now_v = ens.u_views(), ens.result_views()
            for m in retired:                                # a retired member holds the planes it was given
                assert same(now_u[m], u[m]) and same(now_v[m], v[m]), f"member {m}: {what}"
            u, v = now_u, now_v
        held = (u, v)
        got = ens.summaries(first, count) if family == "summary" else ens.changes_since(ref, first, count)
        assert got.shape == (count, 2), what
        field, other = HipConcentration(lone.context, shape), HipConcentration(lone.context, shape)
        for m in range(count):
            for s in (0, 1):
                a = np.ascontiguousarray(held[s][first + m])
                field.upload(lone.context, a)
                if family == "summary":
                    want, alone = summary_ref.summary(a), field.summary(lone.context)
                    ok, ok_alone = summary_ref.same(got[m, s], want), summary_ref.same(got[m, s], alone)
                    if a.size <= EXACT_CELLS:
                        assert_summary_exact(got[m, s], a, what)
                else:
                    b = np.ascontiguousarray((bu, bv)[s][first + m])
                    other.upload(lone.context, b)
                    want, alone = change_ref.change(a, b), field.change_from(lone.context, other)
                    ok, ok_alone = change_ref.same(got[m, s], want), change_ref.same(got[m, s], alone)
                    assert int(got[m, s]["differing"]) == int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))), what
                    if a.size <= EXACT_CELLS:
                        assert_change_exact(got[m, s], a, b, what)
                assert ok, f"member {first + m} {'UV'[s]}: {got[m, s]}, not {want}: {what}"
                assert ok_alone, f"member {first + m} {'UV'[s]} as a lone field: {got[m, s]}, not {alone}: {what}"
        if family == "change":                                # the ensemble against itself: all zero
            zero = ens.changes_since(ens, first, count)
            assert not zero["differing"].any() and not zero["sum_abs"].any() and not zero["max_abs"].any(), what
            ref.destroy()
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
    SEEN.update({"pinned examples": 1} if pinned else {"drawn examples": 1})
    took = time.perf_counter() - started
    SEEN["seconds in pinned examples" if pinned else "seconds in drawn examples"] += took
    SEEN["slowest example, seconds"] = max(SEEN["slowest example, seconds"], took)


@pytest.fixture(scope="module", autouse=True)
def report():
    SEEN.clear()
    yield
    print("\nfloat observe property examples: " + ", ".join(f"{k}: {v:.4g}" for k, v in sorted(SEEN.items())))


# The default keeps the file within the run time of tests/test_gpu_observe_property.py
EXAMPLES = int(os.environ.get("GS_PROPERTY_EXAMPLES_FLOAT", "4"))
_SETTINGS = dict(max_examples=EXAMPLES, deadline=None, suppress_health_check=list(HealthCheck))


@settings(**_SETTINGS)
@given(cases("summary"))
@_with_examples("summary")
def test_any_summary_matches_the_reference(built, case):
    run_case(case, "summary")


@settings(**_SETTINGS)
@given(cases("change"))
@_with_examples("change")
def test_any_change_matches_the_reference(built, case):
    run_case(case, "change")


@settings(**_SETTINGS)
@given(cases("reduce"))
@_with_examples("reduce")
def test_any_reduced_image_matches_the_reference(built, case):
    run_case(case, "reduce")


@settings(**_SETTINGS)
@given(cases("regions"))
@_with_examples("regions")
def test_any_regional_summary_and_morphology_match_the_reference(built, case):
    run_case(case, "regions")
