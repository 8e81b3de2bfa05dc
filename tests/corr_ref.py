"""A numpy restatement of the two-point pair counts of include/gs_hip.h (gs_fields_correlation).  For a plane x of R x C
cells, a threshold t, a sense ``above`` and a largest lag L:

1. a cell is set by morphology's rule (tests/morph_ref.py: ``set_cells``): x > t (``above``) or x < t, one f32 comparison;
2. four unit steps e_k = (dr, dc): (0, 1), (1, 0), (1, 1), (1, -1);
3. ``pairs[k][d]``, d = 0 .. L, counts the unordered cell pairs {p, p + d e_k} with both cells inside the grid and both set.
   Pairs never wrap; a lag that does not fit the grid counts 0; d = 0 counts the set cells.

``pairs`` is one ``count_nonzero`` of the set image and-ed with itself shifted per (k, d); ``literal`` is the same rule as a
per-pair Python loop, for small planes.  Both return ``uint64[4, L + 1]``, the device's layout.  ``totals`` is the geometry:
the number of pairs that exist."""
import numpy as np

from tests.morph_ref import set_cells

STEPS = ((0, 1), (1, 0), (1, 1), (1, -1))
UNIT_ROWS = 512  # kPairRows of grayscott_amd/csrc/gs_correlation.hip, restated (tests/test_correlation_cpu.py holds the two
                 # together): the rows one wave marches over
STRIP_COLS = 256


def pairs(a: np.ndarray, t, above: bool = True, max_lag: int = 32) -> np.ndarray:
    a = np.asarray(a, np.float32)
    out = np.zeros((4, max_lag + 1), np.uint64)
    if a.ndim != 2 or a.size == 0:
        return out
    b = set_cells(a, t, above)
    rows, cols = b.shape
    for k, (dr, dc) in enumerate(STEPS):
        for d in range(max_lag + 1):
            if d * dr >= rows or d * abs(dc) >= cols:
                continue
            upper = b[:rows - d * dr]
            lower = b[d * dr:]
            if dc > 0:
                upper, lower = upper[:, :cols - d], lower[:, d:]
            elif dc < 0:
                upper, lower = upper[:, d:], lower[:, :cols - d]
            out[k, d] = np.count_nonzero(upper & lower)
    return out


def literal(a: np.ndarray, t, above: bool = True, max_lag: int = 32) -> np.ndarray:
    a, t = np.asarray(a, np.float32), np.float32(t)
    rows, cols = a.shape if a.ndim == 2 else (0, 0)
    out = [[0] * (max_lag + 1) for _ in range(4)]

    def cell(r, c):
        x = a[r, c]
        return bool(x > t) if above else bool(x < t)

    for k, (dr, dc) in enumerate(STEPS):
        for d in range(max_lag + 1):
            for r in range(rows):
                for c in range(cols):
                    r2, c2 = r + d * dr, c + d * dc
                    if 0 <= r2 < rows and 0 <= c2 < cols and cell(r, c) and cell(r2, c2):
                        out[k][d] += 1
    return np.array(out, np.uint64)


def totals(rows: int, cols: int, max_lag: int) -> np.ndarray:
    """N_k(d) = max(R - d dr, 0) max(C - d |dc|, 0) as int64[4, L + 1]."""
    return np.array([[max(rows - d * dr, 0) * max(cols - d * abs(dc), 0) for d in range(max_lag + 1)] for dr, dc in STEPS],
                    np.int64)


def stripes(shape, period: int, k: int, lo=0.0, hi=1.0) -> np.ndarray:
    """Stripes (half set to `hi`, half `lo`) with a period of `period` STEPS of e_k across them: the value depends on the
    column (k = 0), the row (k = 1), (r + c) // 2 (k = 2: one step of (1, 1) adds 1) or (r - c) // 2 (k = 3)."""
    r, c = np.indices(shape)
    phase = (c, r, (r + c) // 2, (r - c) // 2)[k]
    return np.where(np.mod(phase, period) < period // 2, np.float32(hi), np.float32(lo)).astype(np.float32)
