"""The C++ mirror's power spectra (include/grayscott_hip.hpp: Species::spectrum, Ensemble::spectra) through
tests/cpp/spectrum_mirror.cpp, against the restatement on the planes the program downloaded and against the Python result on
the same planes."""
import numpy as np
import pytest

from tests import spectrum_ref as ref
from tests.children import build_program, run_program

pytestmark = pytest.mark.gpu


def test_cpp_mirror_spectrum(built, tmp_path):
    from grayscott_amd import HipArgs, Parameters, Simulation, Spectrum
    from grayscott_amd.simulation import spectrum_tables
    from tests.helpers import species_from_arrays

    exe = build_program("spectrum_mirror", tmp_path)
    members, rows, cols, steps, T = 3, 64, 128, 60, 32
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(members), str(rows), str(cols), str(steps), str(T), str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    bins, n = T * (T // 2 + 1), 2 + 2 * members
    rec = np.frombuffer(raw[:n * (bins + 2) * 8], np.uint64).reshape(n, bins + 2)
    power, tiles = rec[:, :bins].view(np.float64).reshape(n, T, T // 2 + 1), rec[:, bins:]
    wavelength = np.frombuffer(raw[n * (bins + 2) * 8:n * (bins + 2) * 8 + 8], np.float64)[0]
    planes = np.frombuffer(raw[n * (bins + 2) * 8 + 8:], np.float32).reshape(2, rows, cols)
    h, w = spectrum_tables(T)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = species_from_arrays(sim, planes[0].copy(), planes[1].copy())
    got = species.spectrum(T, "hann")
    for s in range(2):
        want_power, want_tiles = ref.spectrum(planes[s], T, 1, h, w)
        assert power[s].tobytes() == want_power.tobytes() == got[s].raw.tobytes(), s
        assert tuple(tiles[s]) == tuple(want_tiles) == (got[s].tiles_used, got[s].tiles_skipped) == (8, 0), s
        for m in range(members):                       # every member took the lone Species' steps with its parameters
            assert power[2 + 2 * m + s].tobytes() == power[s].tobytes() and tuple(tiles[2 + 2 * m + s]) == (8, 0), (m, s)
    mine = Spectrum.from_raw(power[1], T, "hann", tiles[1]).wavelength()
    assert mine is not None and abs(wavelength - mine) <= 1e-9 * mine
    sim.context.close()
