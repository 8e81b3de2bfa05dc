"""The C++ mirror's regional histograms (include/grayscott_hip.hpp: Species::region_histogram) through
tests/cpp/region_histogram_mirror.cpp, against the restatement on the planes the program downloaded and against the Python
result on the same planes."""
import numpy as np
import pytest

from tests import region_hist_ref, regions_ref
from tests.children import build_program, run_program

pytestmark = pytest.mark.gpu


def test_cpp_mirror_region_histogram(built, tmp_path):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from tests.helpers import species_from_arrays

    exe = build_program("region_histogram_mirror", tmp_path)
    rows, cols, region, bins = 72, 200, (32, 64), 48
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(rows), str(cols), str(region[0]), str(region[1]), "31", str(bins), str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    rr, rc, b = (int(x) for x in np.frombuffer(raw[:24], np.uint64))
    assert (rr, rc) == regions_ref.grid((rows, cols), region) == (3, 4) and b == bins
    n, words = rr * rc, bins + 4
    rec = np.frombuffer(raw[24:24 + 2 * n * words * 8], np.uint64).reshape(2, rr, rc, words)
    counters, sizes = rec[..., :bins + 3], rec[..., bins + 3]
    planes = np.frombuffer(raw[24 + 2 * n * words * 8:], np.float32).reshape(2, rows, cols)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = species_from_arrays(sim, planes[0].copy(), planes[1].copy())
    hu, hv = species.region_histogram(region, bins, (0.0, 1.0), (-0.125, 0.5))
    assert np.array_equal(counters[0], region_hist_ref.histograms(planes[0], region, 0.0, 1.0, bins))
    assert np.array_equal(counters[1], region_hist_ref.histograms(planes[1], region, -0.125, 0.5, bins))
    assert np.array_equal(counters[0], region_hist_ref.counters_of(hu)) and np.array_equal(counters[1], region_hist_ref.counters_of(hv))
    for p in range(2):
        assert np.array_equal(sizes[p].astype(np.int64), regions_ref.sizes((rows, cols), region)), p
    sim.context.close()
