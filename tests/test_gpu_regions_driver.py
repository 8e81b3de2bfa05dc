"""The simulate driver's regional observables (--hip-regions): <stem>.regions.npz against the restatement applied to the images
of the HDF5 file, and its feed / kill arrays against the region means of the ramps."""
import sys

import numpy as np
import pytest

from grayscott_amd import hdf5_min, simulate
from tests import regions_ref, summary_ref
from tests.children import ROOT, run_program

pytestmark = pytest.mark.gpu


def test_the_driver_writes_the_phase_diagram(built, tmp_path):
    out = tmp_path / "run.h5"
    cmd = [sys.executable, "-m", "grayscott_amd.simulate", "-r", "64", "-c", "128", "-n", "3", "-e", "16", "--hip-feed-map", "0.01:0.06",
           "--hip-kill-map", "0.04:0.07", "--hip-regions", "16x32", "--hip-regions-every", "1", "-o", str(out)]
    r = run_program(cmd, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    images = hdf5_min.read(str(out))
    assert images.shape == (3, 64, 128)
    z = np.load(tmp_path / "run.regions.npz")
    region = (16, 32)
    assert tuple(z["region"]) == region and tuple(z["shape"]) == (64, 128) and list(z["steps"]) == [16, 32, 48]
    assert list(z["thresholds_v"]) == [np.float32(0.25)] and z["thresholds_u"].size == 0 and "quads_u" not in z.files
    assert z["quads_v"].shape == (3, 1, 4, 4, 6) and z["quads_v"].dtype == np.uint64
    assert np.array_equal(z["cells"], regions_ref.sizes((64, 128), region))
    for k in range(3):                                          # (the images are the V planes)
        want = regions_ref.summaries(images[k], region)
        for at in np.ndindex(want.shape):
            got = {f: z[f + "_v"][k][at] for f in summary_ref.FIELDS}
            assert summary_ref.same({f: (int(x) if f == "nonfinite" else float(x)) for f, x in got.items()}, want[at]), (k, at)
        assert np.array_equal(z["quads_v"][k, 0], regions_ref.quads(images[k], region, 0.25, True)), k
        assert z["sum_u"][k].shape == (4, 4) and np.all(z["nonfinite_u"][k] == 0) and np.all(z["max_u"][k] <= 1.0)
    feed = np.repeat(simulate.linear_values(0.01, 0.06, 64)[:, None], 128, axis=1)
    kill = np.repeat(simulate.linear_values(0.04, 0.07, 128)[None, :], 64, axis=0)
    for name, ramp in (("feed", feed), ("kill", kill)):
        assert z[name].shape == (4, 4) and z[name].dtype == np.float64
        for (i, j), crop in regions_ref.crops(ramp, region):
            assert z[name][i, j] == pytest.approx(float(crop.astype(np.float64).mean()), rel=1e-13), (name, i, j)
    assert np.all(np.diff(z["feed"][:, 0]) > 0) and np.all(np.diff(z["kill"][0]) > 0)
