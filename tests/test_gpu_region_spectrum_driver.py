"""The simulate driver's regional power spectra (--hip-region-spectrum-tile): the arrays of <stem>.regions.npz -- keys, shapes,
dtypes --, the last sample against a direct call on the last image of the HDF5 file, and the option errors."""
import sys

import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Parameters, RegionSpectrum, Simulation, hdf5_min
from tests.children import ROOT, run_program

pytestmark = pytest.mark.gpu
BASE = [sys.executable, "-m", "grayscott_amd.simulate", "-r", "128", "-c", "256", "-n", "2", "-e", "24", "--hip-feed-map", "0.01:0.06",
        "--hip-kill-map", "0.04:0.07"]


def test_the_driver_writes_the_regions_spectra(built, tmp_path):
    out = tmp_path / "run.h5"
    cmd = BASE + ["--hip-regions", "64", "--hip-regions-every", "1", "--hip-region-spectrum-tile", "16", "-o", str(out)]
    r = run_program(cmd, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    images = hdf5_min.read(str(out))
    assert images.shape == (2, 128, 256)
    z = np.load(tmp_path / "run.regions.npz")
    assert tuple(z["region"]) == (64, 64) and list(z["steps"]) == [24, 48]
    assert int(z["spectrum_tile"]) == 16 and str(z["spectrum_window"]) == "hann"
    for name in ("u", "v"):
        assert z[f"spectrum_{name}"].shape == (2, 2, 4, 16, 9) and z[f"spectrum_{name}"].dtype == np.float64
        assert z[f"spectrum_tiles_{name}"].shape == (2, 2, 4, 2) and z[f"spectrum_tiles_{name}"].dtype == np.uint64
        assert np.all(z[f"spectrum_tiles_{name}"][..., 0] == 16) and not z[f"spectrum_tiles_{name}"][..., 1].any()
    assert "sum_v" in z.files and "quads_v" in z.files                             # beside the other regional arrays
    # the last sample against a direct call on the last image (the images are the V planes)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    f = HipConcentration(sim.context, (128, 256))
    f.upload(sim.context, images[-1])
    want = f.region_spectrum(sim.context, 64, 16, "hann")
    assert z["spectrum_v"][-1].tobytes() == want.raw.tobytes()
    assert np.array_equal(z["spectrum_tiles_v"][-1, ..., 0], want.tiles_used)
    again = RegionSpectrum.from_raw(z["spectrum_v"][-1], z["spectrum_tiles_v"][-1], 16, str(z["spectrum_window"]), (64, 64), (128, 256))
    assert np.array_equal(again.wavelength(), want.wavelength(), equal_nan=True)
    sim.context.close()
    # without the option the file has none of the arrays
    plain = tmp_path / "plain.h5"
    r = run_program(BASE + ["--hip-regions", "64", "-o", str(plain)], cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert not [k for k in np.load(tmp_path / "plain.regions.npz").files if k.startswith("spectrum")]
    assert hdf5_min.read(str(plain)).tobytes() == images.tobytes()                  # and the images do not depend on it


def test_the_option_errors(built, tmp_path):
    for wrong in (["--hip-region-spectrum-tile", "16"], ["--hip-regions", "64", "--hip-region-spectrum-tile", "48"],
                  ["--hip-regions", "64", "--hip-region-spectrum-window", "none"],
                  ["--hip-regions", "64", "--hip-region-spectrum-tile", "16", "--hip-region-spectrum-window", "hamming"]):
        r = run_program(BASE + wrong + ["-o", str(tmp_path / "x.h5")], cwd=ROOT)
        assert r.returncode == 2 and "hip-region-spectrum" in r.stderr, (wrong, r.stderr)
