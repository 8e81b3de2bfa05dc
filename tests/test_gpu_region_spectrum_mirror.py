"""The C++ mirror's regional power spectra (include/grayscott_hip.hpp: Species::region_spectrum) through
tests/cpp/region_spectrum_mirror.cpp, against the restatement on the planes the program downloaded and against the Python
result on the same planes."""
import numpy as np
import pytest

from tests import region_spectrum_ref, regions_ref
from tests.children import build_program, run_program

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("T,hann", [(16, 1), (32, 0)])
def test_cpp_mirror_region_spectrum(built, tmp_path, T, hann):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from grayscott_amd.simulation import spectrum_tables
    from tests.helpers import species_from_arrays

    exe = build_program("region_spectrum_mirror", tmp_path)
    rows, cols, region = 72, 200, (40, 84)
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(rows), str(cols), str(region[0]), str(region[1]), str(T), str(hann), str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    rr, rc, t = (int(x) for x in np.frombuffer(raw[:24], np.uint64))
    assert (rr, rc) == regions_ref.grid((rows, cols), region) == (2, 3) and t == T
    n, bins = rr * rc, T * (T // 2 + 1)
    rec = np.frombuffer(raw[24:24 + 2 * n * (bins + 2) * 8], np.uint64).reshape(2, rr, rc, bins + 2)
    power, tiles = rec[..., :bins].copy().view(np.float64).reshape(2, rr, rc, T, T // 2 + 1), rec[..., bins:]
    planes = np.frombuffer(raw[24 + 2 * n * (bins + 2) * 8:], np.float32).reshape(2, rows, cols)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = species_from_arrays(sim, planes[0].copy(), planes[1].copy())
    got = species.region_spectrum(region, T, "hann" if hann else "none")
    h, w = spectrum_tables(T)
    for p in range(2):
        want_power, want_tiles = region_spectrum_ref.by_crop(planes[p], region, T, hann, h, w)
        assert power[p].tobytes() == want_power.tobytes() and np.array_equal(tiles[p], want_tiles), p
        assert got[p].raw.tobytes() == power[p].tobytes(), p
        assert np.array_equal(got[p].tiles_used, tiles[p][..., 0]) and np.array_equal(got[p].tiles_skipped, tiles[p][..., 1]), p
    assert tiles[1][0, 0, 0] == (region[0] // T) * (region[1] // T)
    sim.context.close()
