"""A plain numpy/Python restatement of the connected components of include/gs_hip.h (gs_fields_components).  For a plane x of
R x C cells, a threshold t, a sense ``above`` and a connectivity of 4 or 8:

1. a cell is set by morphology's rule (``morph_ref.set_cells``: one f32 comparison; NaN and cells equal to t are not set);
2. set cells are neighbours across a side, under 8 also across a corner; components never wrap;
3. the result is the number of components, the sum of their sizes, the largest size and, per b < 32, the number of
   components with 2^b <= size < 2^(b+1) (the last bin also takes every larger one).

``sizes`` is a union-find over the horizontal runs of set cells: the runs of a row are united with the runs of the row above
that they touch.  ``counters`` returns the 35 u64 words of a ``gs_components``: components, set_cells, largest, by_size[32]."""
import numpy as np

from tests import morph_ref

TILE_ROWS, TILE_COLS = 16, 256  # kCompTileRows, kCompTileCols of grayscott_amd/csrc/gs_kernels.h, restated


def sizes(a: np.ndarray, t, above: bool = True, connectivity: int = 8) -> list:
    """The sizes of the components, in no particular order."""
    assert connectivity in (4, 8)
    a = np.asarray(a, np.float32)
    if a.ndim != 2 or a.size == 0:
        return []
    b = morph_ref.set_cells(a, t, above)
    reach = 1 if connectivity == 8 else 0
    parent, size = [], []

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    prev = []  # (start, end, id) of the runs of the row above, end exclusive
    for r in range(b.shape[0]):
        d = np.diff(np.concatenate(([0], b[r].astype(np.int8), [0])))
        starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
        cur = []
        j = 0
        for s, e in zip(starts.tolist(), ends.tolist()):
            me = len(parent)
            parent.append(me)
            size.append(e - s)
            cur.append((s, e, me))
            while j < len(prev) and prev[j][1] + reach <= s:   # runs above that end before this one begins
                j += 1
            k = j
            while k < len(prev) and prev[k][0] < e + reach:
                x, y = find(me), find(prev[k][2])
                if x != y:
                    parent[max(x, y)] = min(x, y)
                    size[min(x, y)] += size[max(x, y)]
                k += 1
        prev = cur
    return [size[i] for i in range(len(parent)) if parent[i] == i]


def counters(a: np.ndarray, t, above: bool = True, connectivity: int = 8) -> np.ndarray:
    out = np.zeros(35, np.uint64)
    s = sizes(a, t, above, connectivity)
    if not s:
        return out
    out[0], out[1], out[2] = len(s), sum(s), max(s)
    for x in s:
        out[3 + min(int(x).bit_length() - 1, 31)] += np.uint64(1)
    a = np.asarray(a, np.float32)
    assert int(out[1]) == int(np.count_nonzero(morph_ref.set_cells(a, t, above)))
    return out


def result(a: np.ndarray, t, above: bool = True, connectivity: int = 8) -> dict:
    c = counters(a, t, above, connectivity)
    return {"components": int(c[0]), "set_cells": int(c[1]), "largest": int(c[2]), "by_size": c[3:].copy()}


# ---- planes that are hard for a tiled union-find ------------------------------------------------------------------------

def serpentine(shape) -> np.ndarray:
    """One component, one cell wide: every other row is set, joined at alternating ends."""
    rows, cols = shape
    a = np.zeros(shape, np.float32)
    a[0::2] = 1
    for i, r in enumerate(range(1, rows, 2)):
        a[r, cols - 1 if i % 2 == 0 else 0] = 1
    return a


def comb(shape) -> np.ndarray:
    a = np.zeros(shape, np.float32)
    a[0] = 1
    a[:, 0::2] = 1
    return a


def rings(shape) -> np.ndarray:
    rows, cols = shape
    r, c = np.indices(shape)
    depth = np.minimum(np.minimum(r, rows - 1 - r), np.minimum(c, cols - 1 - c))
    return (depth % 2 == 0).astype(np.float32)


def checkerboard(shape) -> np.ndarray:
    r, c = np.indices(shape)
    return ((r + c) % 2 == 0).astype(np.float32)


def staircase(shape) -> np.ndarray:
    """Cells (i, i mod cols): connected under 8 as long as the diagonal does not jump, dust under 4."""
    rows, cols = shape
    a = np.zeros(shape, np.float32)
    n = min(rows, cols)
    a[np.arange(n), np.arange(n)] = 1
    return a


def u_shape(shape, seam) -> np.ndarray:
    """A U whose arms cross the seam above row `seam` twice."""
    rows, cols = shape
    a = np.zeros(shape, np.float32)
    top, bottom = max(seam - 2, 0), min(seam + 1, rows - 1)
    a[top:bottom + 1, 1] = 1
    a[top:bottom + 1, cols - 2] = 1
    a[top, 1:cols - 1] = 1
    return a


def column(shape) -> np.ndarray:
    a = np.zeros(shape, np.float32)
    a[:, shape[1] // 2] = 1
    return a
