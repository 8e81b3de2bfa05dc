"""A numpy restatement of the component matches of include/gs_hip.h (gs_fields_match).  For two planes of one shape, a
threshold t, a sense ``above``, a connectivity of 4 or 8 and a ``min_size`` >= 1:

1. each plane's component list is ``component_list_ref.records`` of that plane and rule;
2. ``scipy.ndimage.label`` numbers each plane's components (all of them, in first-cell order); a ``np.unique`` over the
   (label in before, label in after) of the cells set in BOTH planes gives every pair that shares a cell and how many;
3. labels become record indices after ``min_size``: a pair of which a partner is not listed is dropped.

``match`` returns (before's records, after's records, overlaps) with overlaps a structured array of ``OVERLAP`` in ascending
(before, after) order.  ``literal`` says the same with flood fills and a per-cell dictionary, for small planes.  ``pieces``
counts, per overlap, the connected pieces of the intersection it is made of.  ``pair_of_planes`` makes the planes the GPU
tests match: every kind is meant to show the events ``EVENTS`` names (tests/test_match_cpu.py holds it to that)."""
import numpy as np

from tests import component_list_ref, morph_ref

OVERLAP = np.dtype([("before", np.uint32), ("after", np.uint32), ("cells", np.uint64)])


def _structure(connectivity):
    from scipy import ndimage

    return ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)


def _labels(a, t, above, connectivity, min_size):
    """(labels, index): scipy's labels of the plane and, per label (entry 0: unset), its record index or -1."""
    from scipy import ndimage

    labels, n = ndimage.label(morph_ref.set_cells(a, t, above), _structure(connectivity))
    sizes = np.bincount(labels.ravel(), minlength=n + 1)
    keep = sizes >= min_size
    keep[0] = False
    index = np.where(keep, np.cumsum(keep) - 1, -1)
    return labels, index


def _overlaps(pairs, cells):
    out = np.zeros(len(cells), OVERLAP)
    if len(cells):
        out["before"], out["after"], out["cells"] = pairs[:, 0], pairs[:, 1], cells
    return out


def match(before, after, t, above=True, connectivity=8, min_size=1):
    before, after = np.asarray(before, np.float32), np.asarray(after, np.float32)
    assert before.shape == after.shape and connectivity in (4, 8) and min_size >= 1
    rule = (t, above, connectivity, min_size)
    rec_b, rec_a = component_list_ref.records(before, *rule), component_list_ref.records(after, *rule)
    if before.ndim != 2 or before.size == 0:
        return rec_b, rec_a, np.zeros(0, OVERLAP)
    lab_b, idx_b = _labels(before, *rule)
    lab_a, idx_a = _labels(after, *rule)
    both = (lab_b > 0) & (lab_a > 0)
    pairs = np.stack([idx_b[lab_b[both]], idx_a[lab_a[both]]], axis=1).reshape(-1, 2)
    pairs = pairs[(pairs[:, 0] >= 0) & (pairs[:, 1] >= 0)]
    uniq, cells = np.unique(pairs, axis=0, return_counts=True) if len(pairs) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    return rec_b, rec_a, _overlaps(uniq, cells)


def _fill(b, connectivity):
    """{cell: number} of the set cells of the bool plane b, components numbered in first-cell order; and their sizes."""
    rows, cols = b.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    of, sizes = {}, []
    for r0 in range(rows):
        for c0 in range(cols):
            if not b[r0, c0] or (r0, c0) in of:
                continue
            k = len(sizes)
            of[(r0, c0)] = k
            stack, n = [(r0, c0)], 0
            while stack:
                r, c = stack.pop()
                n += 1
                for dr, dc in steps:
                    rr, cc = r + dr, c + dc
                    if 0 <= rr < rows and 0 <= cc < cols and b[rr, cc] and (rr, cc) not in of:
                        of[(rr, cc)] = k
                        stack.append((rr, cc))
            sizes.append(n)
    return of, sizes


def literal(before, after, t, above=True, connectivity=8, min_size=1):
    """The same match, one cell at a time."""
    before, after = np.asarray(before, np.float32), np.asarray(after, np.float32)
    rule = (t, above, connectivity, min_size)
    rec_b, rec_a = component_list_ref.literal(before, *rule), component_list_ref.literal(after, *rule)
    if before.ndim != 2 or before.size == 0:
        return rec_b, rec_a, np.zeros(0, OVERLAP)
    sides = []
    for plane in (before, after):
        of, sizes = _fill(morph_ref.set_cells(plane, t, above), connectivity)
        index, n = [], 0
        for s in sizes:
            index.append(n if s >= min_size else -1)
            n += s >= min_size
        sides.append((of, index))
    (of_b, idx_b), (of_a, idx_a) = sides
    shared = {}
    for cell, kb in of_b.items():
        ka = of_a.get(cell)
        if ka is None or idx_b[kb] < 0 or idx_a[ka] < 0:
            continue
        key = (idx_b[kb], idx_a[ka])
        shared[key] = shared.get(key, 0) + 1
    keys = sorted(shared)
    return rec_b, rec_a, _overlaps(np.array(keys, np.int64).reshape(-1, 2), [shared[k] for k in keys])


def pieces(before, after, t, above=True, connectivity=8, min_size=1):
    """Per overlap of ``match``, in its order: the connected pieces of the cells set in both planes that it is made of."""
    from scipy import ndimage

    rule = (t, above, connectivity, min_size)
    lab_b, idx_b = _labels(np.asarray(before, np.float32), *rule)
    lab_a, idx_a = _labels(np.asarray(after, np.float32), *rule)
    lab_p, n = ndimage.label((lab_b > 0) & (lab_a > 0), _structure(connectivity))
    cells = np.flatnonzero(lab_p.ravel())
    _, first = np.unique(lab_p.ravel()[cells], return_index=True)
    at = cells[first]  # one cell of every piece
    pairs = np.stack([idx_b[lab_b.ravel()[at]], idx_a[lab_a.ravel()[at]]], axis=1).reshape(-1, 2)
    pairs = pairs[(pairs[:, 0] >= 0) & (pairs[:, 1] >= 0)]
    if not len(pairs):
        return np.zeros(0, np.int64)
    return np.unique(pairs, axis=0, return_counts=True)[1]


def events(rec_b, rec_a, overlaps):
    """The five event counts of a match, restated: degrees from the overlaps, then who has 0, 1 or more partners."""
    deg_b = np.bincount(overlaps["before"].astype(np.int64), minlength=len(rec_b))
    deg_a = np.bincount(overlaps["after"].astype(np.int64), minlength=len(rec_a))
    lone = (deg_b[overlaps["before"].astype(np.int64)] == 1) & (deg_a[overlaps["after"].astype(np.int64)] == 1)
    return {"continued": int(lone.sum()), "split": int((deg_b >= 2).sum()), "merged": int((deg_a >= 2).sum()),
            "born": int((deg_a == 0).sum()), "died": int((deg_b == 0).sum())}


THRESHOLD = 0.5
KINDS = ("noise", "flip", "blocks", "sparse")
# what every kind is meant to show, summed over the shapes of the GPU tests
EVENTS = {"noise": ("split", "merged", "born", "died", "continued"), "flip": ("split", "merged", "continued"),
          "blocks": ("continued", "born", "died"), "sparse": ("born", "died")}


def _plane(rng, set_cells):
    """An f32 plane that is set (above THRESHOLD) exactly where ``set_cells`` says: set cells in (0.5, 1], the others in
    [0, 0.5] -- some of them equal to the threshold, some NaN, some -inf -- and some set cells +inf."""
    hi = (np.float32(0.5) + np.float32(0.5) * (np.float32(1) - rng.random(set_cells.shape, dtype=np.float32))).astype(np.float32)
    hi = np.maximum(hi, np.nextafter(np.float32(0.5), np.float32(1)))
    lo = (np.float32(0.5) * rng.random(set_cells.shape, dtype=np.float32)).astype(np.float32)
    odd = rng.integers(0, 16, set_cells.shape)
    lo[odd == 0] = np.float32(0.5)
    lo[odd == 1] = np.nan
    lo[odd == 2] = -np.inf
    hi[odd == 3] = np.inf
    return np.where(set_cells, hi, lo).astype(np.float32)


def _blocks(rng, shape, n):
    rows, cols = shape
    b = np.zeros(shape, bool)
    for _ in range(n):
        h, w = int(rng.integers(2, 5)), int(rng.integers(3, 8))
        r, c = int(rng.integers(0, max(rows, 1))), int(rng.integers(0, max(cols, 1)))
        b[r:r + h, c:c + w] = True
    return b


def pair_of_planes(shape, seed, kind):
    """(before, after): two f32 planes of ``shape`` to match at ``THRESHOLD``, above.
    noise   two independent planes near the percolation densities: every event, pairs made of several pieces;
    flip    a dense plane and itself with one cell in twelve flipped: components that break and join;
    blocks  scattered rectangles, moved by (1, 2) without wrapping, some removed and some added: continued, died, born;
    sparse  two independent thin planes: almost nothing overlaps."""
    assert kind in KINDS
    rng = np.random.default_rng([int(seed), KINDS.index(kind), int(shape[0]), int(shape[1])])
    rows, cols = shape
    if kind == "noise":
        b, a = rng.random(shape) < 0.45, rng.random(shape) < 0.5
    elif kind == "flip":
        b = rng.random(shape) < 0.55
        a = b ^ (rng.random(shape) < 1.0 / 12.0)
    elif kind == "blocks":
        n = max(1, rows * cols // 150)
        b = _blocks(rng, shape, n)
        a = np.zeros(shape, bool)
        a[1:, 2:] = b[:rows - 1, :cols - 2] if rows > 1 and cols > 2 else False
        gone = _blocks(rng, shape, max(1, n // 4))
        a &= ~gone
        a |= _blocks(rng, shape, max(1, n // 4))
    else:
        b, a = rng.random(shape) < 0.06, rng.random(shape) < 0.06
    return _plane(rng, b), _plane(rng, a)
