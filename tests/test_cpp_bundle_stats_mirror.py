"""The C++ mirror's bundle statistics (include/grayscott_hip.hpp: Ensemble::bundle_stats) over the C ABI.

CPU: the program compiles with plain g++ against gs_hip.h, links libgs_hip.so and fails loudly (HipError, GS_ERR_NO_DEVICE)
without a GPU.  GPU: every result plane of every bundle equals the restatement of tests/bundle_stats_ref.py applied to the
members the program wrote."""
import os

import numpy as np
import pytest

from tests import bundle_stats_ref as ref
from tests.children import ROOT, build_program, run_program


@pytest.fixture(scope="module")
def exe(built, tmp_path_factory):
    return str(build_program("bundle_stats_mirror", tmp_path_factory.mktemp("cpp")))


def test_cpp_method_is_declared(exe):
    hpp = open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    assert "std::vector<Ensemble> bundle_stats(std::size_t span, const std::vector<int32_t> &which" in hpp
    assert "gs_members_bundle_stats(" in hpp


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_cpp_bundle_stats_builds_and_fails_loudly_without_gpu(exe, tmp_path):
    r = run_program([exe, "6", "8", "16", "3", "5", str(tmp_path / "o.bin")])
    assert r.returncode == 14 and "HipError" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("members,rows,cols,span", [(6, 8, 16, 3), (8, 37, 53, 4)])
def test_cpp_bundle_stats_match_the_restatement(exe, tmp_path, members, rows, cols, span):
    out = tmp_path / "o.bin"
    r = run_program([exe, str(members), str(rows), str(cols), str(span), "9", str(out)])
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, np.float32)
    cells, bundles = rows * cols, members // span
    assert raw.size == 2 * members * cells + 5 * 2 * bundles * cells
    u, v = raw[:2 * members * cells].reshape(2, members, rows, cols)
    assert not np.array_equal(u[0], u[1])                                # the members differ: each has its own seed
    got = raw[2 * members * cells:].reshape(5, 2, bundles, rows, cols)
    want = ref.bundles(u, span, 0.5, False), ref.bundles(v, span, 0.25, True)
    for i, name in enumerate(ref.RESULTS):
        for species in (0, 1):
            assert ref.same_bits(got[i, species], want[species][name]), (name, species, ref.describe(got[i, species], want[species][name]))
