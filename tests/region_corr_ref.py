"""A numpy restatement of the regional two-point pair counts of include/gs_hip.h (gs_fields_region_correlation): a region's
counts are what the whole-grid call returns for a plane that holds that region's cells alone.  So every region is cropped
(tests/regions_ref.crops) and handed to tests/corr_ref.pairs: that is the whole definition.  A pair across a region border
is in no crop; a lag that does not fit a (ragged) crop counts 0."""
import numpy as np

from tests import corr_ref, regions_ref
from tests.morph_ref import set_cells


def pairs(a, region, t, above: bool = True, max_lag: int = 32, count=corr_ref.pairs) -> np.ndarray:
    """(RR, RC, 4, L + 1) uint64."""
    out = np.zeros(regions_ref.grid(np.shape(a), region) + (4, max_lag + 1), np.uint64)
    for at, crop in regions_ref.crops(a, region):
        out[at] = count(crop, t, above, max_lag)
    return out


def pairs_by_label(a, region, t, above: bool = True, max_lag: int = 32) -> np.ndarray:
    """The same counts without cropping, for planes of many regions: the whole plane's pairs of set cells whose two cells
    carry the same region index, added up per region (tests/test_region_correlation_cpu.py holds it to ``pairs``)."""
    a = np.asarray(a, np.float32)
    rh, rw = regions_ref.shape_of(region)
    rr, rc = regions_ref.grid(a.shape, region)
    out = np.zeros((rr * rc, 4, max_lag + 1), np.uint64)
    if a.size == 0:
        return out.reshape(rr, rc, 4, max_lag + 1)
    b = set_cells(a, t, above)
    rows, cols = b.shape
    r, c = np.indices(b.shape)
    label = (r // rh) * rc + c // rw
    for k, (dr, dc) in enumerate(corr_ref.STEPS):
        for d in range(max_lag + 1):
            if d * dr >= rows or d * abs(dc) >= cols:
                continue
            upper, lower = np.s_[:rows - d * dr], np.s_[d * dr:]
            left, right = (np.s_[:cols - d], np.s_[d:]) if dc >= 0 else (np.s_[d:], np.s_[:cols - d])
            if dc == 0:
                left = right = np.s_[:]
            both = b[upper, left] & b[lower, right] & (label[upper, left] == label[lower, right])
            out[:, k, d] = np.bincount(label[upper, left][both], minlength=rr * rc)
    return out.reshape(rr, rc, 4, max_lag + 1)


def totals(shape, region, max_lag: int) -> np.ndarray:
    """(RR, RC, 4, L + 1) int64: the pairs that exist inside every region's own cells."""
    out = np.zeros(regions_ref.grid(shape, region) + (4, max_lag + 1), np.int64)
    for at, crop in regions_ref.crops(np.zeros(shape, np.float32), region):
        out[at] = corr_ref.totals(crop.shape[0], crop.shape[1], max_lag)
    return out


def stripe_thirds(shape=(96, 192), periods=(8, 12, 16)) -> np.ndarray:
    """A plane whose column thirds hold vertical stripes of the given periods, each third's phase counted from its own first
    column."""
    width = shape[1] // len(periods)
    return np.concatenate([corr_ref.stripes((shape[0], width), p, 0) for p in periods], axis=1)
