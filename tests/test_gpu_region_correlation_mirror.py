"""The C++ mirror's regional two-point correlations (include/grayscott_hip.hpp: Species::region_correlation) through
tests/cpp/region_correlation_mirror.cpp, against the restatement on the planes the program downloaded and against the Python
result on the same planes."""
import numpy as np
import pytest

from tests import region_corr_ref, regions_ref
from tests.children import build_program, run_program

pytestmark = pytest.mark.gpu


def test_cpp_mirror_region_correlation(built, tmp_path):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from tests.helpers import species_from_arrays

    exe = build_program("region_correlation_mirror", tmp_path)
    rows, cols, region, L = 72, 200, (32, 64), 12
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(rows), str(cols), str(region[0]), str(region[1]), "31", str(L), str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    rr, rc, lag = (int(x) for x in np.frombuffer(raw[:24], np.uint64))
    assert (rr, rc) == regions_ref.grid((rows, cols), region) == (3, 4) and lag == L
    n, words = rr * rc, 4 * (L + 1) + 2
    rec = np.frombuffer(raw[24:24 + 4 * n * words * 8], np.uint64).reshape(2, 2, rr, rc, words)
    pairs, shapes = rec[..., :4 * (L + 1)].reshape(2, 2, rr, rc, 4, L + 1), rec[..., 4 * (L + 1):]
    planes = np.frombuffer(raw[24 + 4 * n * words * 8:], np.float32).reshape(2, rows, cols)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = species_from_arrays(sim, planes[0].copy(), planes[1].copy())
    pu, pv = species.region_correlation(region, (0.25, 0.1), (0.5, 0.8), L)
    for k, (tu, tv) in enumerate(((0.5, 0.25), (0.8, 0.1))):
        assert np.array_equal(pairs[0, k], region_corr_ref.pairs(planes[0], region, tu, False, L)), k
        assert np.array_equal(pairs[1, k], region_corr_ref.pairs(planes[1], region, tv, True, L)), k
        assert np.array_equal(pairs[0, k], pu[k].pairs) and np.array_equal(pairs[1, k], pv[k].pairs), k
    for (i, j), crop in regions_ref.crops(planes[1], region):
        assert tuple(int(x) for x in shapes[1, 0, i, j]) == crop.shape, (i, j)
    sim.context.close()
