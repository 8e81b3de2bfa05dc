"""A numpy restatement of the summaries of include/gs_hip.h (gs_fields_summarize), in its fold order:

1. row partial: 64 lane accumulators (f64, from +0.0); lane l adds the cells at columns 256 k + 4 l + j for k = 0, 1, ...
   and j = 0..3, in that order; a column >= cols or a non-finite cell adds nothing;
2. lane combine: p[0:32] + p[32:64], then p[0:16] + p[16:32], ... down to one value;
3. field fold: the row partials added one after the other in ascending row order, from +0.0.

No ``np.sum`` anywhere (it is pairwise): the lanes are vectors, k and j are Python loops, and the row fold is
``np.cumsum`` (sequential).  ``literal`` is the same definition as a per-cell Python loop, for small arrays."""
import math

import numpy as np

FIELDS = ("sum", "sum_sq", "min", "max", "nonfinite")


def _row_partials(a: np.ndarray):
    """Row partials of a 2-D f32 array: (sum, sum_sq) as f64 vectors over the rows."""
    rows, cols = a.shape
    k_blocks = (cols + 255) // 256
    x = np.zeros((rows, k_blocks * 256), np.float32)
    x[:, :cols] = a
    fin = np.zeros(x.shape, bool)
    fin[:, :cols] = np.isfinite(a)
    d = np.where(fin, x.astype(np.float64), 0.0).reshape(rows, k_blocks, 64, 4)
    s = np.zeros((rows, 64))
    q = np.zeros((rows, 64))
    for k in range(k_blocks):
        for j in range(4):
            v = d[:, k, :, j]
            s = s + v
            q = q + v * v
    while s.shape[1] > 1:
        h = s.shape[1] // 2
        s = s[:, :h] + s[:, h:]
        q = q[:, :h] + q[:, h:]
    return s[:, 0], q[:, 0]


def summary(a: np.ndarray, block_rows: int = 1024) -> dict:
    """The summary of a 2-D f32 array (the whole grid, rows in order)."""
    a = np.asarray(a, np.float32)
    assert a.ndim == 2
    rows, cols = a.shape
    if rows == 0 or cols == 0:
        return {"sum": 0.0, "sum_sq": 0.0, "min": math.inf, "max": -math.inf, "nonfinite": 0}
    s_parts, q_parts = [], []
    for r0 in range(0, rows, block_rows):
        s, q = _row_partials(a[r0:r0 + block_rows])
        s_parts.append(s)
        q_parts.append(q)
    s_rows = np.concatenate([[0.0]] + s_parts)
    q_rows = np.concatenate([[0.0]] + q_parts)
    fin = np.isfinite(a)
    nonfinite = int(a.size - np.count_nonzero(fin))
    finite = a[fin]
    return {"sum": float(np.cumsum(s_rows)[-1]), "sum_sq": float(np.cumsum(q_rows)[-1]),
            "min": float(finite.min()) if finite.size else math.inf,
            "max": float(finite.max()) if finite.size else -math.inf, "nonfinite": nonfinite}


def literal(a: np.ndarray) -> dict:
    """The definition cell by cell, in plain Python floats (IEEE f64): small arrays only."""
    a = np.asarray(a, np.float32)
    rows, cols = a.shape
    total_s = total_q = 0.0
    mn, mx, nf = math.inf, -math.inf, 0
    for r in range(rows):
        lanes_s = [0.0] * 64
        lanes_q = [0.0] * 64
        for k in range((cols + 255) // 256):
            for lane in range(64):
                for j in range(4):
                    c = 256 * k + 4 * lane + j
                    if c >= cols:
                        continue
                    x = float(a[r, c])
                    if not math.isfinite(x):
                        nf += 1
                        continue
                    lanes_s[lane] += x
                    lanes_q[lane] += x * x
                    mn, mx = min(mn, x), max(mx, x)
        while len(lanes_s) > 1:
            h = len(lanes_s) // 2
            lanes_s = [lanes_s[i] + lanes_s[i + h] for i in range(h)]
            lanes_q = [lanes_q[i] + lanes_q[i + h] for i in range(h)]
        total_s += lanes_s[0]
        total_q += lanes_q[0]
    return {"sum": total_s, "sum_sq": total_q, "min": mn, "max": mx, "nonfinite": nf}


def bits(x: float) -> int:
    return int(np.float64(x).view(np.uint64))


def same(got, want) -> bool:
    """Sums as f64 bit patterns, min and max as values (a zero extreme's sign is not specified), equal counts.
    ``got`` / ``want``: dicts, ``Summary`` objects or records of ``SUMMARY_DTYPE``."""
    g, w = as_dict(got), as_dict(want)
    return (bits(g["sum"]) == bits(w["sum"]) and bits(g["sum_sq"]) == bits(w["sum_sq"]) and g["min"] == w["min"]
            and g["max"] == w["max"] and g["nonfinite"] == w["nonfinite"])


def as_dict(s) -> dict:
    if isinstance(s, dict):
        return s
    if isinstance(s, np.void):
        return {f: (int(s[f]) if f == "nonfinite" else float(s[f])) for f in FIELDS}
    return {f: getattr(s, f) for f in FIELDS}
