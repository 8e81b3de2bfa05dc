"""A numpy restatement of the regional observables of include/gs_hip.h (gs_fields_region_summaries,
gs_fields_region_morphology).  A region shape (rh, rw) cuts a plane of R x C cells into ceil(R / rh) x ceil(C / rw) regions,
ragged ones at the lower and right edge kept, and a region's result is what the whole-grid call returns for a plane that
holds that region's cells alone.  So every region is cropped and handed to tests/summary_ref.summary or tests/morph_ref.quads:
that is the whole definition."""
import numpy as np

from tests import morph_ref, summary_ref

SUMMARY_DTYPE = np.dtype([("sum", "<f8"), ("sum_sq", "<f8"), ("min", "<f4"), ("max", "<f4"), ("nonfinite", "<u8")])


def shape_of(region):
    if np.isscalar(region):
        return int(region), int(region)
    return int(region[0]), int(region[1])


def grid(shape, region):
    rh, rw = shape_of(region)
    return -(-shape[0] // rh), -(-shape[1] // rw)


def crops(a, region):
    """((i, j), the cells of region (i, j)) for every region of the plane, in index order."""
    a = np.asarray(a, np.float32)
    rh, rw = shape_of(region)
    rr, rc = grid(a.shape, region)
    for i in range(rr):
        for j in range(rc):
            yield (i, j), a[i * rh:(i + 1) * rh, j * rw:(j + 1) * rw]


def summaries(a, region) -> np.ndarray:
    """(RR, RC) records of SUMMARY_DTYPE."""
    out = np.zeros(grid(np.shape(a), region), SUMMARY_DTYPE)
    for at, crop in crops(a, region):
        s = summary_ref.summary(crop)
        out[at] = tuple(s[f] for f in summary_ref.FIELDS)
    return out


def sizes(shape, region) -> np.ndarray:
    """(RR, RC) int64: every region's number of cells."""
    out = np.zeros(grid(shape, region), np.int64)
    for at, crop in crops(np.zeros(shape, np.float32), region):
        out[at] = crop.size
    return out


def quads(a, region, t, above: bool = True) -> np.ndarray:
    """(RR, RC, 6) uint64: Q0, Q1, Q2, Q3, Q4, QD of every region padded with its own ring of unset cells."""
    out = np.zeros(grid(np.shape(a), region) + (6,), np.uint64)
    for at, crop in crops(a, region):
        out[at] = morph_ref.quads(crop, t, above)
    return out


def same_summaries(got, want) -> bool:
    """Every region by summary_ref.same: sums as bits, extremes as values, counts equal.  ``got``: a ``RegionSummaries`` or
    records; ``want``: records."""
    if not isinstance(got, np.ndarray):
        rec = np.zeros(got.sum.shape, SUMMARY_DTYPE)
        for f in summary_ref.FIELDS:
            rec[f] = getattr(got, f)
        got = rec
    return got.shape == want.shape and all(summary_ref.same(got[at], want[at]) for at in np.ndindex(want.shape))
