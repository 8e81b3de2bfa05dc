"""The definition of the regional power spectra (include/gs_hip.h: gs_fields_region_spectrum): a region's result is what
gs_fields_spectrum returns for a field that holds exactly that region's cells.  So every region is cropped and handed to
tests/spectrum_ref.spectrum, and nothing else is done.  ``records`` restates the header's count of segment records."""
import numpy as np

from tests import regions_ref, spectrum_ref


def by_crop(plane, region, T, window, h, w):
    """(power f64 [RR, RC, T, T/2 + 1], tiles uint64 [RR, RC, 2] = {used, skipped}) of the plane's regions."""
    plane = np.asarray(plane, np.float32)
    rr, rc = regions_ref.grid(plane.shape, region)
    power = np.zeros((rr, rc, T, T // 2 + 1), np.float64)
    tiles = np.zeros((rr, rc, 2), np.uint64)
    for (i, j), crop in regions_ref.crops(plane, region):
        power[i, j], tiles[i, j] = spectrum_ref.spectrum(crop, T, window, h, w)
    return power, tiles


def records(shape, region, T, n=1):
    """The header's record count in words: n times the sum over the regions of (bands of the region) (segments of a band of the
    region) (T (T/2 + 1) + 2)."""
    rh, rw = regions_ref.shape_of(region)
    rr, rc = regions_ref.grid(shape, region)
    total = 0
    for i in range(rr):
        bands = min(rh, shape[0] - i * rh) // T
        for j in range(rc):
            tiles = min(rw, shape[1] - j * rw) // T
            total += bands * (-(-tiles // spectrum_ref.SEGMENT))
    return n * total * (T * (T // 2 + 1) + 2)
