"""The C++ mirror's regional connected components (include/grayscott_hip.hpp: Species::region_components) through
tests/cpp/region_components_mirror.cpp, against the restatement on the planes the program downloaded and against the Python
result on the same planes."""
import numpy as np
import pytest

from tests import region_components_ref, regions_ref
from tests.children import build_program, run_program

pytestmark = pytest.mark.gpu


def test_cpp_mirror_region_components(built, tmp_path):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from tests.helpers import species_from_arrays

    exe = build_program("region_components_mirror", tmp_path)
    rows, cols, region, connectivity = 72, 200, (32, 64), 4
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(rows), str(cols), str(region[0]), str(region[1]), "31", str(connectivity), str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    rr, rc, nt = (int(x) for x in np.frombuffer(raw[:24], np.uint64))
    assert (rr, rc) == regions_ref.grid((rows, cols), region) == (3, 4) and nt == 2
    words = 2 * nt * rr * rc * 35
    rec = np.frombuffer(raw[24:24 + words * 8], np.uint64).reshape(2, nt, rr, rc, 35)
    planes = np.frombuffer(raw[24 + words * 8:], np.float32).reshape(2, rows, cols)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = species_from_arrays(sim, planes[0].copy(), planes[1].copy())
    cu, cv = species.region_components(region, (0.25, 0.1), (0.5, 0.9), connectivity=connectivity)
    for k, (tu, tv) in enumerate(((0.5, 0.25), (0.9, 0.1))):
        assert np.array_equal(rec[0, k], region_components_ref.counters(planes[0], region, tu, False, connectivity)), k
        assert np.array_equal(rec[1, k], region_components_ref.counters(planes[1], region, tv, True, connectivity)), k
        assert np.array_equal(rec[0, k], cu[k].counters()) and np.array_equal(rec[1, k], cv[k].counters()), k
    assert rec[1, 0, ..., 0].sum() > 0                                     # the seeded square is there
    sim.context.close()
