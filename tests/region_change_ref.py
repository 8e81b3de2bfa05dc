"""The definition of the regional state comparison of include/gs_hip.h (gs_fields_region_compare): a region's result is what
the whole-grid comparison (tests/change_ref.py) gives for two planes that hold that region's cells alone -- ``change_ref.change``
applied to ``regions_ref.crops`` of both planes.  UNROLL and BAND restate the kernels' unroll depth (rows or chunks of both
planes loaded before the adds) and the record route's band height (grayscott_amd/csrc/gs_kernels.h)."""
import numpy as np

from tests import change_ref, regions_ref

UNROLL = 4
BAND = 16

CHANGE_DTYPE = np.dtype([("sum_abs", "<f8"), ("sum_sq", "<f8"), ("max_abs", "<f8"), ("differing", "<u8"), ("nonfinite", "<u8")])


def changes(a, b, region) -> np.ndarray:
    """(RR, RC) records of CHANGE_DTYPE: plane ``a`` against plane ``b``, region by region."""
    out = np.zeros(regions_ref.grid(np.shape(a), region), CHANGE_DTYPE)
    for (at, crop_a), (_, crop_b) in zip(regions_ref.crops(a, region), regions_ref.crops(b, region)):
        c = change_ref.change(crop_a, crop_b)
        out[at] = tuple(c[f] for f in change_ref.FIELDS)
    return out
