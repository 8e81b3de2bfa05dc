"""A numpy restatement of the regional connected components of include/gs_hip.h (gs_fields_region_components): a region's
result is what gs_fields_components returns for a plane that holds that region's cells alone.  So every region is cropped
(tests/regions_ref.crops) and handed to tests/components_ref.counters: that is the whole definition -- a crop has no
neighbours, so a region's border is a wall."""
import numpy as np

from tests import components_ref, regions_ref


def counters(a, region, t, above: bool = True, connectivity: int = 8) -> np.ndarray:
    """(RR, RC, 35) uint64: components, set_cells, largest, by_size[32] of every region."""
    out = np.zeros(regions_ref.grid(np.shape(a), region) + (35,), np.uint64)
    for at, crop in regions_ref.crops(a, region):
        out[at] = components_ref.counters(crop, t, above, connectivity)
    return out


def invariants(a, region, t, above: bool = True, connectivity: int = 8, got=None) -> np.ndarray:
    """Asserts the three invariants of the header on `got` (default: the reference's own counters) against the whole plane's
    components and returns `got`: set_cells sums to the whole grid's, the components sum to at least the whole grid's, and
    one region over the whole plane is the whole grid's result."""
    got = counters(a, region, t, above, connectivity) if got is None else np.asarray(got)
    whole = components_ref.counters(a, t, above, connectivity)
    assert int(got[..., 1].sum()) == int(whole[1])
    assert int(got[..., 0].sum()) >= int(whole[0])
    assert int(got[..., 2].max(initial=0)) <= int(whole[2])
    assert np.array_equal(got[..., 3:].sum(axis=-1), got[..., 0])
    if got.shape[:2] == (1, 1):
        assert np.array_equal(got[0, 0], whole)
    return got
