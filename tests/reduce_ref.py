"""A numpy restatement of the reduced result image of include/gs_hip.h (gs_field_download_reduced), in its fold order.

For a plane of shape [rows, cols] and a factor f the image has shape [ceil(rows / f), ceil(cols / f)]; pixel (R, C) covers
the cells r in [R f, min((R + 1) f, rows)), c in [C f, min((C + 1) f, cols)):

1. row partial p_r: an f64 accumulator starting at +0.0 to which the block's cells of row r are added in ascending column order;
2. block sum: an f64 accumulator starting at +0.0 to which p_r is added in ascending row order;
3. pixel = float32(block sum / float64(count)), count = the number of cells in the block.

``reduce`` is that definition on whole arrays: Python loops over the at most f columns and f rows of a block, every pixel
of the image at once -- f64 adds in the stated order, no ``np.sum`` and no ``reshape(...).mean`` (their orders are numpy's
business).  A cell outside the plane is +0.0, which leaves an accumulator that started at +0.0 as it was (it never holds
-0.0).  f = 1 is the plain download, not the fold: the input's bits, a cell
of -0.0 included.  ``literal`` is the same definition as a per-pixel Python loop over the cells that exist, for small arrays.
``slab_rule`` mirrors the library's verdict on slab chains; ``same_bits`` is the comparison the tests use."""
import numpy as np


def shape(rows: int, cols: int, f: int):
    return (-(-rows // f), -(-cols // f))


def reduce(a: np.ndarray, f: int, reverse_columns: bool = False) -> np.ndarray:
    """The reduced image of a 2-D f32 array.  ``reverse_columns`` folds every row's cells in DESCENDING column order
    instead: not the definition -- the tests use it to show that the order is observable."""
    a = np.asarray(a, np.float32)
    assert a.ndim == 2 and 1 <= f <= 64
    rows, cols = a.shape
    if f == 1:
        return a.copy()
    orows, ocols = shape(rows, cols, f)
    x = np.zeros((orows * f, ocols * f), np.float64)
    x[:rows, :cols] = a                                    # exact: every f32 is an f64
    x = x.reshape(orows, f, ocols, f)
    nr = np.minimum(f, rows - np.arange(orows) * f)
    nc = np.minimum(f, cols - np.arange(ocols) * f)
    order = range(f - 1, -1, -1) if reverse_columns else range(f)
    with np.errstate(all="ignore"):
        total = np.zeros((orows, ocols), np.float64)
        for i in range(f):
            p = np.zeros((orows, ocols), np.float64)
            for j in order:
                p = p + x[:, i, :, j]
            total = total + p
        count = (nr[:, None] * nc[None, :]).astype(np.float64)
        return (total / count).astype(np.float32)


def literal(a: np.ndarray, f: int) -> np.ndarray:
    """The definition, cell by cell (slow: small arrays only)."""
    a = np.asarray(a, np.float32)
    rows, cols = a.shape
    orows, ocols = shape(rows, cols, f)
    out = np.empty((orows, ocols), np.float32)
    with np.errstate(all="ignore"):
        for R in range(orows):
            for C in range(ocols):
                total = np.float64(0.0)
                count = 0
                for r in range(R * f, min((R + 1) * f, rows)):
                    p = np.float64(0.0)
                    for c in range(C * f, min((C + 1) * f, cols)):
                        p = p + np.float64(a[r, c])
                        count += 1
                    total = total + p
                out[R, C] = np.float32(total / np.float64(count))
    return out


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    """Equal bit patterns, NaN pixels compared by position (a NaN pixel is any NaN)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != np.float32 or want.dtype != np.float32:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return False
    return np.array_equal(np.ascontiguousarray(got).view(np.uint32)[~gn], np.ascontiguousarray(want).view(np.uint32)[~wn])


def slab_starts(rows: int, slabs: int):
    """First global rows of the slabs of a grid (the split of gs_field_create: k * rows / S)."""
    return [k * rows // slabs for k in range(slabs)]


def slab_rule(rows: int, slabs: int, f: int) -> bool:
    """True when a grid of `rows` rows over `slabs` slabs (all processes' together) admits the factor: every slab begins at
    a multiple of f.  The library refuses the others with GS_ERR_UNSUPPORTED."""
    return all(r0 % f == 0 for r0 in slab_starts(rows, slabs))


def local_rows(rows: int, slabs: int, first_slab: int, n_local: int, f: int):
    """Output rows [row0 / f, ceil(row1 / f)) of a process that holds slabs [first_slab, first_slab + n_local)."""
    r0 = first_slab * rows // slabs
    r1 = (first_slab + n_local) * rows // slabs
    return r0 // f, -(-r1 // f)


def special_plane(shape_, seed: int) -> np.ndarray:
    """A random f32 plane with the values that make the definition observable: sub-normals, signed zeros, a NaN, an
    infinity of either sign, and cells of widely differing magnitude, some beyond what an f64 accumulator holds exactly (so
    that the fold order shows in the result)."""
    rng = np.random.default_rng(seed)
    rows, cols = shape_
    a = rng.random((rows, cols), dtype=np.float32)
    n = rows * cols
    flat = a.reshape(-1)
    k = max(1, n // 16)
    flat[rng.choice(n, k, replace=False)] *= np.float32(1.0e6)
    flat[rng.choice(n, k, replace=False)] *= np.float32(-1.0e-6)
    flat[rng.choice(n, k, replace=False)] = np.float32(3.0e-41)          # sub-normal
    flat[rng.choice(n, k, replace=False)] = np.float32(-1.0e-45)         # the smallest sub-normal, negative
    flat[rng.choice(n, k, replace=False)] = np.float32(-0.0)
    flat[rng.choice(n, k, replace=False)] = np.float32(0.0)
    # pairs (+2^80, -2^80) side by side and one above the other: inside one block the f64 accumulator absorbs what came
    # before the pair and keeps what comes after it, so another column or row order gives another f32
    big = np.float32(2.0 ** 80)
    for _ in range(max(1, n // 48)):
        r, c = int(rng.integers(rows)), int(rng.integers(cols))
        if c + 1 < cols:
            a[r, c], a[r, c + 1] = big, -big
        r, c = int(rng.integers(rows)), int(rng.integers(cols))
        if r + 1 < rows:
            a[r, c], a[r + 1, c] = -big, big
    if n >= 64:
        i = rng.choice(n, 3, replace=False)
        flat[i[0]] = np.float32(np.nan)
        flat[i[1]] = np.float32(np.inf)
        flat[i[2]] = np.float32(-np.inf)
    if rows >= 8 and cols >= 8:
        a[-1, -1] = np.float32(-0.0)
        a[:2, :2] = np.float32(-0.0)                                    # a whole block of -0.0 at f = 2: the pixel is +0.0
        a[2:4, 0:2] = np.float32(1.0e-45)                               # ... and one whose mean is a sub-normal
    return a
