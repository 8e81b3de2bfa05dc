"""The C++ mirror's Ensemble (include/grayscott_hip.hpp) over the C ABI.

CPU: the program compiles with plain g++ against gs_hip.h, links libgs_hip.so and fails loudly (HipError,
GS_ERR_NO_DEVICE) without a GPU.  GPU: a sweep of members with their own feed and kill rates, run in two calls, equals a
lone Species per member and the oracle, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(built, tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp") / "ensemble_mirror"
    libdir = os.path.join(ROOT, "grayscott_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "ensemble_mirror.cpp"), "-o", str(out),
           "-L", libdir, "-lgs_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_cpp_ensemble_builds_and_fails_loudly_without_gpu(exe, tmp_path):
    r = subprocess.run([exe, "4", "8", "16", "3", str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 14 and "HipError" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(8, 16), (72, 200)])
def test_cpp_ensemble_matches_lone_species_and_oracle(exe, tmp_path, rows, cols):
    import oracle

    members, steps = 5, 41
    out = tmp_path / "o.bin"
    r = subprocess.run([exe, str(members), str(rows), str(cols), str(steps), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    data = np.fromfile(out, np.float32).reshape(2, members, rows, cols)
    u0, v0 = oracle.init_species(rows, cols)
    for i in range(members):
        assert data[0, i].tobytes() == data[1, i].tobytes(), f"member {i} differs from its lone Species"
        p = oracle.default_params()
        p.feed = np.float32(0.010) + np.float32(0.004) * np.float32(i)
        p.kill = np.float32(0.050) + np.float32(0.002) * np.float32(members - 1 - i)
        assert data[0, i].tobytes() == oracle.run(u0, v0, steps, params=p)[1].tobytes(), f"member {i} differs from the oracle"
