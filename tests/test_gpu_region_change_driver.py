"""The simulate driver's regional change (--hip-regions ... --hip-region-change --hip-region-steady-tol): the change_* arrays of
<stem>.regions.npz against the restatement applied to consecutive images of the HDF5 file (the first image against the initial
state), `steady` as it follows from the arrays, and the interval in steps."""
import sys

import numpy as np
import pytest

from grayscott_amd import hdf5_min
from tests import change_ref, region_change_ref
from tests.children import ROOT, run_program

pytestmark = pytest.mark.gpu


def test_the_driver_writes_the_regions_change(built, tmp_path):
    from grayscott_amd import HipArgs, Parameters, Simulation

    out = tmp_path / "run.h5"
    tol = 1e-3
    cmd = [sys.executable, "-m", "grayscott_amd.simulate", "-r", "64", "-c", "128", "-n", "3", "-e", "16", "--hip-feed-map", "0.01:0.06",
           "--hip-kill-map", "0.04:0.07", "--hip-regions", "16x32", "--hip-regions-every", "1", "--hip-region-change",
           "--hip-region-steady-tol", str(tol), "-o", str(out)]
    r = run_program(cmd, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    images = hdf5_min.read(str(out))
    assert images.shape == (3, 64, 128)
    z = np.load(tmp_path / "run.regions.npz")
    region = (16, 32)
    assert tuple(z["region"]) == region and list(z["steps"]) == [16, 32, 48]
    assert int(z["change_steps"]) == 16 and float(z["steady_tol"]) == tol
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))            # the initial state: what image 1 is compared with
    start = sim.make_species([64, 128]).in_out()[1].make_scalar_view(sim.context)
    sim.context.close()
    states = [start] + [images[k] for k in range(3)]                    # (the images are the V planes)
    for name in ("u", "v"):
        for f in change_ref.FIELDS:
            a = z[f"change_{f}_{name}"]
            assert a.shape == (3, 4, 4) and a.dtype == (np.uint64 if f in change_ref.COUNTS else np.float64), (f, name)
    for k in range(3):
        want = region_change_ref.changes(states[k + 1], states[k], region)
        for at in np.ndindex(want.shape):
            got = {f: z[f"change_{f}_v"][k][at] for f in change_ref.FIELDS}
            got = {f: (int(x) if f in change_ref.COUNTS else float(x)) for f, x in got.items()}
            assert change_ref.same(got, want[at]), (k, at, got, change_ref.as_dict(want[at]))
    steady = z["steady"]
    assert steady.shape == (3, 4, 4) and steady.dtype == np.bool_
    follows = ((z["change_max_abs_u"] <= tol) & (z["change_nonfinite_u"] == 0) & (z["change_max_abs_v"] <= tol)
               & (z["change_nonfinite_v"] == 0))
    assert np.array_equal(steady, follows)
    assert not steady.all() and z["change_differing_v"].sum() > 0       # the seeded square moves
    # without the flag the file holds none of it
    plain = tmp_path / "plain.h5"
    r = run_program(cmd[:cmd.index("--hip-region-change")] + ["-o", str(plain)], cwd=ROOT)
    assert r.returncode == 0, r.stderr
    zp = np.load(tmp_path / "plain.regions.npz")
    assert not [k for k in zp.files if k.startswith(("change_", "steady"))]
    assert hdf5_min.read(str(plain)).tobytes() == images.tobytes()      # observing the change does not touch the run
