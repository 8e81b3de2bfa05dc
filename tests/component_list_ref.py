"""A numpy restatement of the component lists of include/gs_hip.h (gs_field_component_list).  For a plane x of R x C cells, a
threshold t, a sense ``above``, a connectivity of 4 or 8 and a ``min_size`` >= 1:

1. a cell is set by morphology's rule (``morph_ref.set_cells``: one f32 comparison; NaN and cells equal to t are not set);
2. ``scipy.ndimage.label`` with the 4- or 8-structure joins the set cells into components, which never wrap, and numbers
   them in the order of their first cells in row-major order;
3. every component of at least ``min_size`` cells is one record of ``DTYPE`` (gs_component_record): its cells, the sums of
   their row and column indices, its first cell, its bounding box -- from ``find_objects``, ``sum_labels`` and ``np.nonzero``.

``literal`` says the same with a flood fill, cell by cell, for small planes; ``counters`` turns a list taken with ``min_size`` 1
into the 35 words of a ``gs_components`` (tests/components_ref.py: ``counters``)."""
import numpy as np

from tests import morph_ref

DTYPE = np.dtype([("size", np.uint64), ("sum_row", np.uint64), ("sum_col", np.uint64), ("first_row", np.uint32),
                  ("first_col", np.uint32), ("row_min", np.uint32), ("row_max", np.uint32), ("col_min", np.uint32),
                  ("col_max", np.uint32)])


def records(a: np.ndarray, t, above: bool = True, connectivity: int = 8, min_size: int = 1) -> np.ndarray:
    from scipy import ndimage

    assert connectivity in (4, 8) and min_size >= 1
    a = np.asarray(a, np.float32)
    if a.ndim != 2 or a.size == 0:
        return np.zeros(0, DTYPE)
    b = morph_ref.set_cells(a, t, above)
    labels, n = ndimage.label(b, ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2))
    out = np.zeros(n, DTYPE)
    if n == 0:
        return out
    index = np.arange(1, n + 1)
    r, c = np.indices(a.shape)
    out["size"] = np.bincount(labels.ravel(), minlength=n + 1)[1:]
    # (exact: a float64 sum of integers below 2^53)
    out["sum_row"] = np.rint(ndimage.sum_labels(r.astype(np.float64), labels, index)).astype(np.uint64)
    out["sum_col"] = np.rint(ndimage.sum_labels(c.astype(np.float64), labels, index)).astype(np.uint64)
    assert a.size * max(a.shape) < 2 ** 53
    for k, (rows, cols) in enumerate(ndimage.find_objects(labels)):
        out["row_min"][k], out["row_max"][k] = rows.start, rows.stop - 1
        out["col_min"][k], out["col_max"][k] = cols.start, cols.stop - 1
    # the first cell of label k in row-major order: the first place its number appears
    flat = labels.ravel()
    cells = np.flatnonzero(flat)
    _, first = np.unique(flat[cells], return_index=True)
    out["first_row"], out["first_col"] = np.divmod(cells[first], a.shape[1])
    assert np.all(np.diff(cells[first]) > 0), "scipy numbers components by their first cells"
    return out[out["size"] >= np.uint64(min_size)]


def literal(a: np.ndarray, t, above: bool = True, connectivity: int = 8, min_size: int = 1) -> np.ndarray:
    """The same list by a flood fill from every cell in row-major order, one cell at a time."""
    a = np.asarray(a, np.float32)
    if a.ndim != 2 or a.size == 0:
        return np.zeros(0, DTYPE)
    rows, cols = a.shape
    b = morph_ref.set_cells(a, t, above)
    seen = np.zeros(a.shape, bool)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    out = []
    for r0 in range(rows):
        for c0 in range(cols):
            if not b[r0, c0] or seen[r0, c0]:
                continue
            seen[r0, c0] = True
            stack, cells = [(r0, c0)], []
            while stack:
                r, c = stack.pop()
                cells.append((r, c))
                for dr, dc in steps:
                    rr, cc = r + dr, c + dc
                    if 0 <= rr < rows and 0 <= cc < cols and b[rr, cc] and not seen[rr, cc]:
                        seen[rr, cc] = True
                        stack.append((rr, cc))
            if len(cells) >= min_size:
                rs, cs = [r for r, _ in cells], [c for _, c in cells]
                out.append((len(cells), sum(rs), sum(cs), r0, c0, min(rs), max(rs), min(cs), max(cs)))
    return np.array(out, DTYPE) if out else np.zeros(0, DTYPE)


def counters(rec: np.ndarray) -> np.ndarray:
    """The 35 u64 words of a ``gs_components`` -- components, set_cells, largest, by_size[32] -- from a list taken with
    ``min_size`` 1."""
    out = np.zeros(35, np.uint64)
    sizes = [int(x) for x in rec["size"]]
    if not sizes:
        return out
    out[0], out[1], out[2] = len(sizes), sum(sizes), max(sizes)
    for x in sizes:
        out[3 + min(x.bit_length() - 1, 31)] += np.uint64(1)
    return out


def shifted(rec: np.ndarray, rows: int) -> np.ndarray:
    """The records of a plane that lies ``rows`` rows further down in a larger one."""
    out = rec.copy()
    for k in ("first_row", "row_min", "row_max"):
        out[k] += np.uint32(rows)
    out["sum_row"] += out["size"] * np.uint64(rows)
    return out
