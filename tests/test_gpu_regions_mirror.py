"""The C++ mirror's regional observables (include/grayscott_hip.hpp: Species::region_summaries, Species::region_morphology)
through tests/cpp/regions_mirror.cpp, against the restatement on the planes the program downloaded."""
import numpy as np
import pytest

from tests import regions_ref
from tests.children import build_program, run_program

pytestmark = pytest.mark.gpu


def test_cpp_mirror_regions(built, tmp_path):
    exe = build_program("regions_mirror", tmp_path)
    rows, cols, region = 72, 200, (32, 64)
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(rows), str(cols), str(region[0]), str(region[1]), "31", str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    rr, rc = (int(x) for x in np.frombuffer(raw[:16], np.uint64))
    assert (rr, rc) == regions_ref.grid((rows, cols), region) == (3, 4)
    n, at = rr * rc, 16
    sums, sizes = [], []
    for _ in range(2):
        sums.append(np.frombuffer(raw[at:at + 32 * n], regions_ref.SUMMARY_DTYPE).reshape(rr, rc))
        sizes.append(np.frombuffer(raw[at + 32 * n:at + 40 * n], np.uint64).reshape(rr, rc))
        at += 40 * n
    quads = np.frombuffer(raw[at:at + 4 * n * 48], np.uint64).reshape(2, 2, rr, rc, 6)
    planes = np.frombuffer(raw[at + 4 * n * 48:], np.float32).reshape(2, rows, cols)
    for p in range(2):
        assert regions_ref.same_summaries(sums[p], regions_ref.summaries(planes[p], region)), p
        assert np.array_equal(sizes[p].astype(np.int64), regions_ref.sizes((rows, cols), region)), p
    for k, (tu, tv) in enumerate(((0.5, 0.25), (0.8, 0.1))):
        assert np.array_equal(quads[0, k], regions_ref.quads(planes[0], region, tu, False)), k
        assert np.array_equal(quads[1, k], regions_ref.quads(planes[1], region, tv, True)), k
