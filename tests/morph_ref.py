"""A numpy restatement of the bit-quad counts of include/gs_hip.h (gs_fields_morphology).  For a plane x of R x C cells, a
threshold t and a sense ``above``:

1. a cell is set iff x > t (``above``) or x < t: one f32 comparison -- NaN is never set, a cell equal to t is not set;
2. the binary image is padded with one ring of unset cells;
3. each of the (R + 1)(C + 1) 2 x 2 blocks of the padded image counts in one of six classes: Q0 no set cell, Q1 one, Q2 two
   that share a side, Q3 three, Q4 four, QD two on a diagonal.

``quads`` forms the four shifted views of the padded image and classifies by their sum and the diagonal test; ``literal`` is
the same rule as a per-quad Python loop, for small planes.  Both return a ``uint64`` vector of six counters, the layout of
``gs_morphology``.  ``measures`` derives the set cells, the 4-connected boundary length and the two Euler numbers."""
import numpy as np

UNIT_ROWS = 32  # kQuadRows of grayscott_amd/csrc/gs_morphology.hip, restated: the quad rows one wave marches over


def set_cells(a: np.ndarray, t, above: bool) -> np.ndarray:
    a, t = np.asarray(a, np.float32), np.float32(t)
    with np.errstate(invalid="ignore"):
        return (a > t) if above else (a < t)


def quads(a: np.ndarray, t, above: bool = True) -> np.ndarray:
    a = np.asarray(a, np.float32)
    if a.ndim != 2 or a.size == 0:
        return np.zeros(6, np.uint64)
    b = np.pad(set_cells(a, t, above), 1).astype(np.int64)
    tl, tr, bl, br = b[:-1, :-1], b[:-1, 1:], b[1:, :-1], b[1:, 1:]
    n = tl + tr + bl + br
    diagonal = (n == 2) & (tl == br)
    out = [np.count_nonzero(n == 0), np.count_nonzero(n == 1), np.count_nonzero((n == 2) & ~diagonal),
           np.count_nonzero(n == 3), np.count_nonzero(n == 4), np.count_nonzero(diagonal)]
    return np.array(out, np.uint64)


def literal(a: np.ndarray, t, above: bool = True) -> np.ndarray:
    a, t = np.asarray(a, np.float32), np.float32(t)
    rows, cols = a.shape
    out = [0] * 6
    if rows == 0 or cols == 0:
        return np.array(out, np.uint64)

    def cell(r, c):
        if r < 0 or r >= rows or c < 0 or c >= cols:
            return False
        x = a[r, c]
        return bool(x > t) if above else bool(x < t)

    for r in range(-1, rows):
        for c in range(-1, cols):
            q = [cell(r, c), cell(r, c + 1), cell(r + 1, c), cell(r + 1, c + 1)]
            n = sum(q)
            if n == 2:
                out[5 if q[0] == q[3] else 2] += 1
            else:
                out[n] += 1
    return np.array(out, np.uint64)


def measures(q) -> dict:
    """Set cells, boundary length and Euler numbers from six counters (exact integers)."""
    q0, q1, q2, q3, q4, qd = (int(x) for x in q)
    area4, e8, e4 = q1 + 2 * q2 + 2 * qd + 3 * q3 + 4 * q4, q1 - q3 - 2 * qd, q1 - q3 + 2 * qd
    assert area4 % 4 == 0 and e8 % 4 == 0 and e4 % 4 == 0, q
    return {"area": area4 // 4, "perimeter": q1 + q2 + 2 * qd + q3, "euler8": e8 // 4, "euler4": e4 // 4}


def planted(shape, t, seed: int, density: float = 0.5, above: bool = True) -> np.ndarray:
    """A plane whose cells are set (with respect to t and the sense) with probability ``density``, plus, where it has room:
    set cells in all four corners, along the first and last row and column, in both rows of every seam between the units
    of UNIT_ROWS quad rows; and NaN, +-inf, sub-normals, +-0 and cells equal to t and its f32 neighbours."""
    rng = np.random.default_rng(seed)
    rows, cols = shape
    t32, inf = np.float32(t), np.float32(np.inf)
    span = np.float32(max(1.0, abs(float(t32))))
    hi, lo = t32 + span * rng.random(shape, dtype=np.float32) + np.float32(1e-3), t32 - span * rng.random(shape, dtype=np.float32) - np.float32(1e-3)
    on, off = (hi, lo) if above else (lo, hi)
    a = np.where(rng.random(shape) < density, on, off).astype(np.float32)
    if a.size == 0:
        return a
    edge = rng.random(shape) < 0.7
    for r in {0, rows - 1}:
        a[r] = np.where(edge[r], on[r], a[r])
    for c in {0, cols - 1}:
        a[:, c] = np.where(edge[:, c], on[:, c], a[:, c])
    # quad row q (lower row q) ends a unit when q % UNIT_ROWS == UNIT_ROWS - 1: rows q - 1, q, q + 1 straddle the seam
    for q in range(UNIT_ROWS - 1, rows, UNIT_ROWS):
        for r in (q - 1, q, q + 1):
            if 0 <= r < rows:
                a[r] = np.where(rng.random(cols) < 0.6, on[r], off[r])
    for r, c in ((0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)):
        a[r, c] = on[r, c]
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38, 3.4028235e38,
                        -3.4028235e38, t32, t32, t32, np.nextafter(t32, -inf), np.nextafter(t32, inf)], np.float32)
    if a.size >= 4 * len(special):
        idx = rng.choice(a.size, size=len(special), replace=False)
        a.flat[idx] = special
    return a
