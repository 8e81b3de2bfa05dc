"""Planes for the on-device observables' tests that no fixed list holds: the `seams` and `lane_runs` layouts, the other
pattern kinds of tests/test_gpu_observe_property.py, and how a pattern of set and unset cells becomes f32 values around a
threshold.  Everything is numpy, drawn from a generator the caller seeds; nothing here touches the device.

The kernels' units, restated from the references that restate them: a labelling tile is TILE_ROWS x TILE_COLS cells, a
wave of the bit-quad kernel marches over QUAD_ROWS quad rows, one of the pair kernel over PAIR_ROWS rows of a strip of
STRIP_COLS columns, which it keeps as words of WORD_COLS columns; a lane holds LANE_COLS columns."""
import numpy as np

from tests import components_ref, corr_ref, morph_ref

TILE_ROWS, TILE_COLS = components_ref.TILE_ROWS, components_ref.TILE_COLS
QUAD_ROWS = morph_ref.UNIT_ROWS
PAIR_ROWS, STRIP_COLS = corr_ref.UNIT_ROWS, corr_ref.STRIP_COLS
LANE_COLS = 4                           # a float4 per lane (gs_plane_scan.h: gs_load_columns)
WORD_COLS = TILE_COLS // LANE_COLS      # the lanes of a wave; the pair kernel's word

DENSITIES = [0.02, 0.3, 0.5, 0.593, 0.95]
ADVERSARIAL = {"serpentine": components_ref.serpentine, "comb": components_ref.comb, "rings": components_ref.rings,
               "checkerboard": components_ref.checkerboard, "staircase": components_ref.staircase,
               "column": components_ref.column}
KINDS = ["planted"] + sorted(ADVERSARIAL) + ["u_shape", "full", "empty", "one-set", "one-unset", "seams", "lane_runs"]
PLACES = ["nw", "n", "ne", "w", "e", "sw", "s", "se"]      # corners and edge midpoints of one-set / one-unset


def seam_rows(rows, slabs):
    """The first rows of slabs 1 .. slabs - 1 of a chain over `rows` rows (the library's i * rows // slabs); row 0 is no
    seam, whatever the division gives."""
    return sorted({i * rows // slabs for i in range(1, slabs)} - {0})


def place_of(name, shape):
    rows, cols = shape
    return {"n": 0, "s": rows - 1}.get(name[0], rows // 2), {"w": 0, "e": cols - 1}.get(name[-1], cols // 2)


def seam_lines(shape, slabs=1):
    """(rows, columns) of the `seams` layout: the rows on either side of every tile, quad-unit and pair-unit seam (and one
    below the quad unit's, whose wave reads its first row twice), every slab's first row and the row above it, the columns
    on either side of every word and strip seam (and one right of the strip's)."""
    rows, cols = shape
    line_rows = {m * TILE_ROWS + d for m in range(1, rows // TILE_ROWS + 2) for d in (-1, 0)}
    line_rows |= {m * QUAD_ROWS + d for m in range(1, rows // QUAD_ROWS + 2) for d in (-1, 0, 1)}
    line_rows |= {m * PAIR_ROWS + d for m in range(1, rows // PAIR_ROWS + 2) for d in (-1, 0)}
    line_rows |= {r + d for r in seam_rows(rows, min(slabs, rows)) for d in (-1, 0)}
    line_cols = {m * WORD_COLS + d for m in range(1, cols // WORD_COLS + 2) for d in (-1, 0)}
    line_cols |= {m * STRIP_COLS + d for m in range(1, cols // STRIP_COLS + 2) for d in (-1, 0, 1)}
    return sorted(r for r in line_rows if 0 <= r < rows), sorted(c for c in line_cols if 0 <= c < cols)


def seams_are_mixed(bits, line_rows, line_cols):
    """Does every seam line of 8 cells or more hold a set cell and a gap?"""
    lines = ([bits[r, :] for r in line_rows] if bits.shape[1] >= 8 else []) + ([bits[:, c] for c in line_cols] if bits.shape[0] >= 8 else [])
    return all(line.any() and not line.all() for line in lines)


def seams(shape, rng, slabs=1):
    """Set lines on every seam of `seam_lines`, each cell opened again half of the time, over a plane that is random at
    density 0.3; drawn again until every line has set cells and gaps."""
    line_rows, line_cols = seam_lines(shape, slabs)
    on_line = np.zeros(shape, bool)
    on_line[line_rows, :] = True
    on_line[:, line_cols] = True
    for _ in range(64):
        bits = np.where(on_line, rng.random(shape) < 0.5, rng.random(shape) < 0.3)
        if seams_are_mixed(bits, line_rows, line_cols):
            break
    return bits


def lane_patterns(bits):
    """The four-bit pattern (bit j: column 4 l + j) of every whole lane of every row, as an int array [rows, lanes]."""
    rows, cols = bits.shape
    lanes = cols // LANE_COLS
    b = bits[:, :lanes * LANE_COLS].reshape(rows, lanes, LANE_COLS).astype(np.int64)
    return (b << np.arange(LANE_COLS)).sum(axis=2)


def lane_runs(shape, rng):
    """Rows of horizontal runs for the tile kernel's run logic.  Rows 0, 4, 8, ... draw a pattern per lane of LANE_COLS
    columns: a lane stays full (pattern 15) three times out of four after a full one, else it takes any of the 16 patterns,
    so runs begin and end in every column of a lane beside long stretches of full lanes.  Row 4 k + 1 is row 4 k moved one
    column right, row 4 k + 2 draws anew, row 4 k + 3 is row 4 k + 2 moved one column left: runs meet the row above
    straight up and across both corners."""
    rows, cols = shape
    lanes = -(-cols // LANE_COLS)
    bits = np.zeros((rows, lanes * LANE_COLS + 2), bool)

    def fresh():
        full = False
        pattern = np.empty(lanes, np.int64)
        for l in range(lanes):
            full = rng.random() < (0.75 if full else 0.4)
            pattern[l] = 15 if full else int(rng.integers(0, 16))
            full = pattern[l] == 15
        return ((pattern[:, None] >> np.arange(LANE_COLS)) & 1).astype(bool).reshape(-1)

    for r in range(rows):
        if r % 2 == 0:
            bits[r, 1:-1] = fresh()
        elif r % 4 == 1:
            bits[r, 2:] = bits[r - 1, 1:-1]
        else:
            bits[r, :-2] = bits[r - 1, 1:-1]
    return bits[:, 1:cols + 1].copy()


def pattern(kind, shape, rng, density=0.5, at=None, slabs=1):
    """The set cells of pattern `kind` as a boolean plane (`planted` is made of values at once: `plane`)."""
    rows, cols = shape
    if kind in ADVERSARIAL:
        return ADVERSARIAL[kind](shape) != 0
    if kind == "u_shape":
        if cols < 3:                                # no room for two arms
            return components_ref.column(shape) != 0
        at_rows = seam_rows(rows, min(max(slabs, 2), rows)) or [rows // 2]
        return components_ref.u_shape(shape, at_rows[int(rng.integers(0, len(at_rows)))]) != 0
    if kind == "full":
        return np.ones(shape, bool)
    if kind == "empty":
        return np.zeros(shape, bool)
    if kind in ("one-set", "one-unset"):
        cell = place_of(at, shape) if at else (int(rng.integers(0, rows)), int(rng.integers(0, cols)))
        bits = np.zeros(shape, bool)
        bits[cell] = True
        return bits if kind == "one-set" else ~bits
    if kind == "seams":
        return seams(shape, rng, slabs)
    if kind == "lane_runs":
        return lane_runs(shape, rng)
    raise ValueError(kind)


def values_of(bits, t, above, rng, special=True):
    """A f32 plane whose cells are set with respect to threshold `t` and the sense exactly where `bits` says, as far as a
    value can be (nothing is above +inf or below -inf): set and unset cells lie at least 1e-3 on either side of t -- beside
    an infinite t, finite on one side and t itself or NaN on the other.  With `special`, a few cells (one in four at most)
    then become NaN, +-inf, +-0, sub-normals of both signs, the largest finite values, t and its two f32 neighbours, as
    morph_ref.planted sprinkles them: what is set is then the values' business (morph_ref.set_cells), not the pattern's."""
    bits = np.asarray(bits, bool)
    shape = bits.shape
    t32, inf = np.float32(t), np.float32(np.inf)
    with np.errstate(all="ignore"):
        if np.isinf(t32):
            finite = ((rng.random(shape, dtype=np.float32) - np.float32(0.5)) * np.float32(4.0)).astype(np.float32)
            beyond = np.where(rng.random(shape) < 0.5, t32, np.float32(np.nan)).astype(np.float32)
            a = np.where(bits, finite, beyond)     # (the sense that nothing satisfies: the realised plane is empty)
        else:
            span = np.float32(max(1.0, abs(float(t32))))
            hi = t32 + span * rng.random(shape, dtype=np.float32) + np.float32(1e-3)
            lo = t32 - span * rng.random(shape, dtype=np.float32) - np.float32(1e-3)
            a = np.where(bits, hi if above else lo, lo if above else hi)
    a = a.astype(np.float32)
    if special and a.size >= 4:
        with np.errstate(over="ignore"):             # (the neighbour above the largest finite value is +inf)
            odd = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38, 3.4028235e38,
                            -3.4028235e38, t32, t32, t32, np.nextafter(t32, -inf), np.nextafter(t32, inf)], np.float32)
        n = min(len(odd), a.size // 4)
        a.flat[rng.choice(a.size, size=n, replace=False)] = odd[rng.permutation(len(odd))[:n]]
    return a


def plane(kind, shape, t, above, seed, density=0.5, at=None, slabs=1, special=True):
    """The f32 plane of pattern `kind` for threshold `t` and the sense, all drawn from `seed`."""
    if kind == "planted":
        with np.errstate(all="ignore"):             # (beside an infinite or the largest threshold)
            return morph_ref.planted(shape, t, seed, density, above)
    rng = np.random.default_rng(seed)
    bits = pattern(kind, shape, rng, density, at, slabs)
    # one set or unset cell, full and empty planes stay what they are called: no special cells
    return values_of(bits, t, above, rng, special and kind not in ("full", "empty", "one-set", "one-unset"))


def poison_value(above):
    """A value that is set by the widest margin there is under the sense (not even it is above +inf or below -inf)."""
    return np.float32(np.inf) if above else np.float32(-np.inf)
