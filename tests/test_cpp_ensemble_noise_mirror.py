"""The C++ mirror's ensemble noise (include/grayscott_hip.hpp: Ensemble::set_noise / noise / clear_noise) over the C ABI.

CPU: the program compiles with plain g++ against gs_hip.h, links libgs_hip.so and fails loudly (HipError, GS_ERR_NO_DEVICE)
without a GPU.  GPU: the structs round-trip with their step counters advanced, and every member equals the restatement of
tests/noise_ref.py with its own struct."""
import os

import numpy as np
import pytest

from tests.children import ROOT, build_program, run_program


@pytest.fixture(scope="module")
def exe(built, tmp_path_factory):
    return str(build_program("ensemble_noise_mirror", tmp_path_factory.mktemp("cpp")))


def test_cpp_methods_are_declared(exe):
    hpp = open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    for name in ("void set_noise(const std::vector<gs_noise> &noise", "void set_noise(const gs_noise &noise",
                 "std::vector<gs_noise> noise() const", "void clear_noise()"):
        assert name in hpp, name


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_cpp_ensemble_noise_builds_and_fails_loudly_without_gpu(exe, tmp_path):
    r = run_program([exe, "4", "8", "16", "3", str(tmp_path / "o.bin")])
    assert r.returncode == 14 and "HipError" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(8, 16), (72, 200)])
def test_cpp_ensemble_noise_round_trips_and_matches_the_reference(exe, tmp_path, rows, cols):
    import oracle

    from grayscott_amd.simulation import NOISE_DTYPE

    from . import noise_ref as N

    members, steps = 4, 13
    out = tmp_path / "o.bin"
    r = run_program([exe, str(members), str(rows), str(cols), str(steps), str(out)])
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    got = np.frombuffer(raw[:members * 24], NOISE_DTYPE)
    planes = np.frombuffer(raw[members * 24:], np.float32).reshape(2, members, rows, cols)
    want = [dict(sigma_u=np.float32(0.01) * np.float32(i + 1), sigma_v=np.float32(0.005) * np.float32(i), seed=100 + i, step=7 * i)
            for i in range(members)]
    want[0] = dict(sigma_u=np.float32(0.02), sigma_v=np.float32(0.0), seed=5, step=1)  # (overwritten through the one-struct form)
    u0, v0 = oracle.init_species(rows, cols)
    for i, w in enumerate(want):
        assert (got[i]["sigma_u"], got[i]["sigma_v"], got[i]["seed"], got[i]["step"]) == (w["sigma_u"], w["sigma_v"], w["seed"],
                                                                                          w["step"] + steps), i
        ru, rv = N.run(u0, v0, steps, w)
        assert planes[0, i].tobytes() == ru.tobytes(), f"U of member {i}"
        assert planes[1, i].tobytes() == rv.tobytes(), f"V of member {i}"
