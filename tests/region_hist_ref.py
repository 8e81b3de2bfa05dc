"""A numpy restatement of the regional histograms of include/gs_hip.h (gs_fields_region_histogram): a region's bins + 3
counters are what the whole-grid call returns for a plane that holds that region's cells alone, with the same range and
bins.  So every region is cropped (tests/regions_ref.crops) and handed to tests/hist_ref.histogram: that is the whole
definition.  ``by_label`` is the same result without cropping, for planes of many regions."""
import numpy as np

from tests import hist_ref, regions_ref

# The most rows of one tile of gs_region_hist_k (grayscott_amd/csrc/gs_region_hist.hip: kTileRows), restated: a region higher
# than this is counted by several tiles into the same counters, whatever the launch makes of a tile.
TILE_ROWS = 256


def histograms(a, region, lo, hi, bins: int, count=hist_ref.histogram) -> np.ndarray:
    """(RR, RC, bins + 3) uint64: counts, below, above, nan of every region."""
    out = np.zeros(regions_ref.grid(np.shape(a), region) + (bins + 3,), np.uint64)
    for at, crop in regions_ref.crops(a, region):
        out[at] = count(crop, lo, hi, bins)
    return out


def by_label(a, region, lo, hi, bins: int) -> np.ndarray:
    """The same counters from one ``np.bincount`` over region index x (bins + 3) + the cell's slot."""
    a = np.asarray(a, np.float32)
    rh, rw = regions_ref.shape_of(region)
    rr, rc = regions_ref.grid(a.shape, region)
    if a.size == 0:
        return np.zeros((rr, rc, bins + 3), np.uint64)
    r, c = np.indices(a.shape)
    label = (r // rh) * rc + c // rw
    key = label * (bins + 3) + hist_ref.slots(a, lo, hi, bins)
    return np.bincount(key.ravel(), minlength=rr * rc * (bins + 3)).astype(np.uint64).reshape(rr, rc, bins + 3)


def counters_of(h) -> np.ndarray:
    """(RR, RC, bins + 3) uint64 from a ``RegionHistogram``: the C ABI's slots."""
    return np.concatenate([h.counts, np.stack([h.below, h.above, h.nan], axis=2)], axis=2).astype(np.uint64)
