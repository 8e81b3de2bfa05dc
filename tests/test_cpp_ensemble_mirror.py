"""The C++ mirror's Ensemble (include/grayscott_hip.hpp) over the C ABI.

CPU: the program compiles with plain g++ against gs_hip.h, links libgs_hip.so and fails loudly (HipError,
GS_ERR_NO_DEVICE) without a GPU.  GPU: a sweep of members with their own feed and kill rates, run in two calls, equals a
lone Species per member and the oracle, bit for bit."""
import os

import numpy as np
import pytest

from tests.children import build_program, run_program


@pytest.fixture(scope="module")
def exe(built, tmp_path_factory):
    out = build_program("ensemble_mirror", tmp_path_factory.mktemp("cpp"))
    return str(out)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_cpp_ensemble_builds_and_fails_loudly_without_gpu(exe, tmp_path):
    r = run_program([exe, "4", "8", "16", "3", str(tmp_path / "o.bin")])
    assert r.returncode == 14 and "HipError" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(8, 16), (72, 200)])
def test_cpp_ensemble_matches_lone_species_and_oracle(exe, tmp_path, rows, cols):
    import oracle

    members, steps = 5, 41
    out = tmp_path / "o.bin"
    r = run_program([exe, str(members), str(rows), str(cols), str(steps), str(out)])
    assert r.returncode == 0, r.stderr
    data = np.fromfile(out, np.float32).reshape(2, members, rows, cols)
    u0, v0 = oracle.init_species(rows, cols)
    for i in range(members):
        assert data[0, i].tobytes() == data[1, i].tobytes(), f"member {i} differs from its lone Species"
        p = oracle.default_params()
        p.feed = np.float32(0.010) + np.float32(0.004) * np.float32(i)
        p.kill = np.float32(0.050) + np.float32(0.002) * np.float32(members - 1 - i)
        assert data[0, i].tobytes() == oracle.run(u0, v0, steps, params=p)[1].tobytes(), f"member {i} differs from the oracle"
