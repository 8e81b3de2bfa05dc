"""A numpy restatement of the comparison of two planes of include/gs_hip.h (gs_fields_compare).  Per cell
d = (double)a - (double)b, one f64 subtraction; a cell is comparable when a and b are both finite, any other cell counts
in ``nonfinite`` and adds nothing; ``differing`` counts the cells whose 32-bit patterns differ, over all cells.  The sums of
|d| and d * d are folded in the summaries' order:

1. row partial: 64 lane accumulators (f64, from +0.0); lane l adds the cells at columns 256 k + 4 l + j for k = 0, 1, ...
   and j = 0..3, in that order; a column >= cols or a cell that is not comparable adds nothing;
2. lane combine: p[0:32] + p[32:64], then p[0:16] + p[16:32], ... down to one value;
3. field fold: the row partials added one after the other in ascending row order, from +0.0.

No ``np.sum`` anywhere (it is pairwise): the lanes are vectors, k and j are Python loops, and the row fold is
``np.cumsum`` (sequential).  ``literal`` is the same definition as a per-cell, per-lane Python loop, for small arrays, and
``ascending`` folds a row's cells in plain ascending column order -- the order a wrong kernel would most likely use."""
import math

import numpy as np

FIELDS = ("sum_abs", "sum_sq", "max_abs", "differing", "nonfinite")
COUNTS = ("differing", "nonfinite")


def _comparable(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.isfinite(a) & np.isfinite(b)


def _diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """d per cell in f64, +0.0 where the cell is not comparable."""
    fin = _comparable(a, b)
    with np.errstate(invalid="ignore"):
        d = a.astype(np.float64) - b.astype(np.float64)
    return np.where(fin, d, 0.0)


def _row_partials(d: np.ndarray):
    """Row partials of sum |d| and sum d * d of a 2-D f64 array of differences: f64 vectors over the rows."""
    rows, cols = d.shape
    k_blocks = (cols + 255) // 256
    x = np.zeros((rows, k_blocks * 256), np.float64)
    x[:, :cols] = d
    x = x.reshape(rows, k_blocks, 64, 4)
    s = np.zeros((rows, 64))
    q = np.zeros((rows, 64))
    for k in range(k_blocks):
        for j in range(4):
            v = x[:, k, :, j]
            s = s + np.abs(v)
            q = q + v * v
    while s.shape[1] > 1:
        h = s.shape[1] // 2
        s = s[:, :h] + s[:, h:]
        q = q[:, :h] + q[:, h:]
    return s[:, 0], q[:, 0]


def _order_free(a: np.ndarray, b: np.ndarray, d: np.ndarray) -> dict:
    fin = _comparable(a, b)
    return {"max_abs": float(np.abs(d).max()) if d.size else 0.0,
            "differing": int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))),
            "nonfinite": int(a.size - np.count_nonzero(fin))}


def change(a: np.ndarray, b: np.ndarray, block_rows: int = 1024) -> dict:
    """The comparison of two 2-D f32 arrays of one shape (the whole grid, rows in order): a against b."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.ndim == 2 and a.shape == b.shape
    rows, cols = a.shape
    if rows == 0 or cols == 0:
        return {"sum_abs": 0.0, "sum_sq": 0.0, "max_abs": 0.0, "differing": 0, "nonfinite": 0}
    d = _diff(a, b)
    s_parts, q_parts = [], []
    for r0 in range(0, rows, block_rows):
        s, q = _row_partials(d[r0:r0 + block_rows])
        s_parts.append(s)
        q_parts.append(q)
    s_rows = np.concatenate([[0.0]] + s_parts)
    q_rows = np.concatenate([[0.0]] + q_parts)
    out = {"sum_abs": float(np.cumsum(s_rows)[-1]), "sum_sq": float(np.cumsum(q_rows)[-1])}
    out.update(_order_free(a, b, d))
    return out


def literal(a: np.ndarray, b: np.ndarray) -> dict:
    """The definition cell by cell and lane by lane, in plain Python floats (IEEE f64): small arrays only."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    rows, cols = a.shape
    ab, bb = a.view(np.uint32), b.view(np.uint32)
    total_s = total_q = mx = 0.0
    df = nf = 0
    for r in range(rows):
        lanes_s = [0.0] * 64
        lanes_q = [0.0] * 64
        for k in range((cols + 255) // 256):
            for lane in range(64):
                for j in range(4):
                    c = 256 * k + 4 * lane + j
                    if c >= cols:
                        continue
                    if ab[r, c] != bb[r, c]:
                        df += 1
                    x, y = float(a[r, c]), float(b[r, c])
                    if not (math.isfinite(x) and math.isfinite(y)):
                        nf += 1
                        continue
                    d = x - y
                    lanes_s[lane] += abs(d)
                    lanes_q[lane] += d * d
                    mx = max(mx, abs(d))
        while len(lanes_s) > 1:
            h = len(lanes_s) // 2
            lanes_s = [lanes_s[i] + lanes_s[i + h] for i in range(h)]
            lanes_q = [lanes_q[i] + lanes_q[i + h] for i in range(h)]
        total_s += lanes_s[0]
        total_q += lanes_q[0]
    return {"sum_abs": total_s, "sum_sq": total_q, "max_abs": mx, "differing": df, "nonfinite": nf}


def ascending(a: np.ndarray, b: np.ndarray) -> dict:
    """NOT the rule: every row folded in plain ascending column order (then the rows in order).  Planes on which this
    differs from ``change`` in the bits of the sums tell a kernel with the wrong fold order from a right one."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    d = _diff(a, b)
    z = np.zeros((d.shape[0], 1))
    s = np.cumsum(np.concatenate([z, np.abs(d)], axis=1), axis=1)[:, -1]
    q = np.cumsum(np.concatenate([z, d * d], axis=1), axis=1)[:, -1]
    out = {"sum_abs": float(np.cumsum(np.concatenate([[0.0], s]))[-1]),
           "sum_sq": float(np.cumsum(np.concatenate([[0.0], q]))[-1])}
    out.update(_order_free(a, b, d))
    return out


def order_sensitive(shape, seed, binades=12):
    """Two planes whose differences spread over 2 x ``binades`` binades around 1, cell by cell at random, so that cells
    thousands of times larger stand next to cells near 1 and smaller.  |d| and d * d are all positive and nothing cancels,
    but every addition rounds away low bits of the smaller term, so another fold order gives sums that are a few units in
    the last place away.  (A few much larger cells, +-2^80 say, would hide that: the last place of their squares, 2^108,
    swallows every other cell whole in any order.)  Two orders can still round to the same f64 by chance: the callers
    check, for the seeds they use, that plain ascending column order does not."""
    rng = np.random.default_rng(seed)
    scale = np.ldexp(np.float32(1.0), rng.integers(-binades, binades + 1, size=shape)).astype(np.float32)
    sign = np.where(rng.random(shape) < 0.5, np.float32(-1), np.float32(1))
    a = (rng.random(shape, dtype=np.float32) + np.float32(0.5)) * scale * sign
    b = rng.random(shape, dtype=np.float32) * scale * np.float32(0.25)
    return a.astype(np.float32), b.astype(np.float32)


def bits(x: float) -> int:
    return int(np.float64(x).view(np.uint64))


def as_dict(c) -> dict:
    if isinstance(c, dict):
        return c
    if isinstance(c, np.void):
        return {f: (int(c[f]) if f in COUNTS else float(c[f])) for f in FIELDS}
    return {f: getattr(c, f) for f in FIELDS}


def same(got, want) -> bool:
    """Sums and the maximum as f64 bit patterns, equal counts.  ``got`` / ``want``: dicts, ``Change`` objects or records
    of ``CHANGE_DTYPE``."""
    g, w = as_dict(got), as_dict(want)
    return all(bits(g[f]) == bits(w[f]) for f in ("sum_abs", "sum_sq", "max_abs")) and all(g[f] == w[f] for f in COUNTS)
