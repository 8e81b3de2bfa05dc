"""The C++ mirror's noise term (include/grayscott_hip.hpp: Simulation::set_noise, noise, clear_noise) through
tests/cpp/noise_mirror.cpp: the planes the program leaves against the restatement of tests/noise_ref.py, bit for bit."""
import numpy as np
import pytest

import oracle
from tests import noise_ref
from tests.children import build_program, run_program
from tests.helpers import assert_bits_equal

pytestmark = pytest.mark.gpu


def test_cpp_mirror_noise(built, tmp_path):
    exe = build_program("noise_mirror", tmp_path)
    rows, cols, steps = 72, 200, 11
    noise = dict(sigma_u=0.02, sigma_v=0.005, seed=987654321987, step=2 ** 32 - 4)
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(rows), str(cols), str(steps), repr(noise["sigma_u"]), repr(noise["sigma_v"]), str(noise["seed"]),
                     str(noise["step"]), str(out)])
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = out.read_bytes()
    assert int(np.frombuffer(raw[:8], np.uint64)[0]) == noise["step"] + steps
    planes = np.frombuffer(raw[8:], np.float32).reshape(2, rows, cols)
    ref = noise_ref.run(*oracle.init_species(rows, cols), steps, noise)
    assert_bits_equal(planes[0], ref[0], "U of the C++ mirror")
    assert_bits_equal(planes[1], ref[1], "V of the C++ mirror")
