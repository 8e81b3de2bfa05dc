"""The C++ mirror's regional state comparison (include/grayscott_hip.hpp: Species::region_changes_since) through
tests/cpp/region_change_mirror.cpp, against the restatement on the planes the program downloaded and against the Python result
on the same planes."""
import numpy as np
import pytest

from tests import change_ref, region_change_ref, regions_ref
from tests.children import build_program, run_program

pytestmark = pytest.mark.gpu


def test_cpp_mirror_region_changes_since(built, tmp_path):
    from grayscott_amd import HipArgs, Parameters, Simulation
    from tests.helpers import species_from_arrays

    exe = build_program("region_change_mirror", tmp_path)
    rows, cols, region = 72, 200, (32, 64)
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(rows), str(cols), str(region[0]), str(region[1]), "31", str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    rr, rc = (int(x) for x in np.frombuffer(raw[:16], np.uint64))
    assert (rr, rc) == regions_ref.grid((rows, cols), region) == (3, 4)
    record = np.dtype([("sum_abs", "<f8"), ("sum_sq", "<f8"), ("max_abs", "<f8"), ("differing", "<u8"), ("nonfinite", "<u8"), ("cells", "<u8")])
    rec = np.frombuffer(raw[16:16 + 2 * rr * rc * record.itemsize], record).reshape(2, rr, rc)
    planes = np.frombuffer(raw[16 + 2 * rr * rc * record.itemsize:], np.float32).reshape(4, rows, cols)   # snapshot U, V; current U, V
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = species_from_arrays(sim, planes[0].copy(), planes[1].copy())
    snap = species.snapshot()
    species.in_out()[0].upload(sim.context, planes[2].copy())
    species.in_out()[1].upload(sim.context, planes[3].copy())
    python = species.region_changes_since(snap, region)
    for k in range(2):
        want = region_change_ref.changes(planes[2 + k], planes[k], region)
        assert np.array_equal(rec[k]["cells"], regions_ref.sizes((rows, cols), region))
        for at in np.ndindex(want.shape):
            assert change_ref.same(rec[k][at], want[at]), (k, at)
            assert change_ref.same(rec[k][at], python[k].at(*at)), (k, at)
    assert rec[1]["differing"].sum() > 0                                   # the seeded square moves
    snap.close()
    sim.context.close()
