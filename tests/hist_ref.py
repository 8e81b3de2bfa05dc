"""A numpy restatement of the histograms of include/gs_hip.h (gs_fields_histogram).  For a range lo < hi (finite f32) and
``bins``, every cell x lands in exactly one of ``bins + 3`` counters -- counts[0 .. bins), below, above, nan:

1. x is NaN -> nan;  2. x < lo -> below;  3. x > hi -> above;
4. otherwise counts[min(int(t), bins - 1)] with t = (x - lo) * scale, the subtraction and the multiplication one f32
   operation each, and scale = f32(bins) / (hi - lo) formed in f32: one subtraction, one division.

Everything stays in ``np.float32`` (numpy rounds each f32 operation to nearest even and keeps sub-normals); nothing here
calls ``numpy.histogram``, which bins in f64 and disagrees next to an edge.  ``literal`` is the same rule as a per-cell
Python loop, for small arrays.  Both return a ``uint64`` vector of ``bins + 3`` counters, the layout of the C ABI."""
import numpy as np


def scale_of(lo, hi, bins: int) -> np.float32:
    lo, hi = np.float32(lo), np.float32(hi)
    return np.float32(bins) / (hi - lo)


def slots(a: np.ndarray, lo, hi, bins: int) -> np.ndarray:
    """The counter index of every cell: [0, bins) a bin, bins = below, bins + 1 = above, bins + 2 = nan."""
    a = np.asarray(a, np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    scale = scale_of(lo, hi, bins)
    nan, below, above = np.isnan(a), a < lo, a > hi
    inside = ~(nan | below | above)
    x = np.where(inside, a, lo).astype(np.float32)
    with np.errstate(all="ignore"):
        t = (x - lo) * scale
    assert t.dtype == np.float32
    b = np.minimum(t.astype(np.int64), bins - 1)  # (t >= 0: the conversion truncates)
    b = np.where(below, bins, b)
    b = np.where(above, bins + 1, b)
    return np.where(nan, bins + 2, b)


def histogram(a: np.ndarray, lo, hi, bins: int) -> np.ndarray:
    return np.bincount(slots(a, lo, hi, bins).ravel(), minlength=bins + 3).astype(np.uint64)


def literal(a: np.ndarray, lo, hi, bins: int) -> np.ndarray:
    lo, hi = np.float32(lo), np.float32(hi)
    width = np.float32(hi - lo)
    scale = np.float32(np.float32(bins) / width)
    out = [0] * (bins + 3)
    for x in np.asarray(a, np.float32).ravel():
        if x != x:
            out[bins + 2] += 1
        elif x < lo:
            out[bins] += 1
        elif x > hi:
            out[bins + 1] += 1
        else:
            d = np.float32(x - lo)
            t = np.float32(d * scale)
            out[min(int(t), bins - 1)] += 1
    return np.array(out, np.uint64)


def t_of(x, lo, hi, bins: int) -> np.ndarray:
    """t of rule 4 for in-range cells (f32)."""
    return (np.asarray(x, np.float32) - np.float32(lo)) * scale_of(lo, hi, bins)


def planted(shape, lo, hi, bins: int, seed: int) -> np.ndarray:
    """A plane of values spread a little beyond [lo, hi] that also holds, where it has room: NaN, +-inf, +-0,
    sub-normals, lo, hi, their f32 neighbours on both sides, and the nominal edges lo + i (hi - lo) / bins with theirs."""
    rng = np.random.default_rng(seed)
    lo32, hi32 = np.float32(lo), np.float32(hi)
    w = float(hi32) - float(lo32)
    a = (float(lo32) - 0.1 * w + rng.random(shape) * 1.2 * w).astype(np.float32)
    inf = np.float32(np.inf)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-40, 1.1754942e-38, -3e-39, 3.4028235e38, -3.4028235e38,
               lo32, hi32, np.nextafter(lo32, -inf), np.nextafter(lo32, inf), np.nextafter(hi32, -inf), np.nextafter(hi32, inf)]
    which = np.unique(np.concatenate([np.arange(0, bins + 1, max(1, bins // 16)), [1, bins - 1, bins]]))
    for i in which:
        e = np.float32(float(lo32) + i * w / bins)
        special += [e, np.nextafter(e, -inf), np.nextafter(e, inf)]
    special = np.array(special, np.float32)
    if a.size:
        idx = rng.choice(a.size, size=min(a.size, len(special)), replace=False)
        a.flat[idx] = special[rng.permutation(len(special))[:len(idx)]]
    return a
