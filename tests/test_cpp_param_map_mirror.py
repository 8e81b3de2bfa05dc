"""Simulation::set_param_map of the C++ mirror (include/grayscott_hip.hpp) over the C ABI.

CPU: the program compiles with plain g++ against gs_hip.h and links libgs_hip.so.  GPU: a map with F rising along the
rows and k along the columns, then the map detached, both bit for bit against the mapped reference (tests/param_map_ref.py)."""
import os

import numpy as np
import pytest

from . import param_map_ref as R
from tests.children import build_program, run_program


@pytest.fixture(scope="module")
def exe(built, tmp_path_factory):
    out = build_program("param_map_mirror", tmp_path_factory.mktemp("cpp"))
    return str(out)


def test_cpp_param_map_builds(exe):
    assert os.access(exe, os.X_OK)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", [(40, 70), (300, 517)])
def test_cpp_param_map_matches_the_reference(exe, tmp_path, rows, cols):
    import oracle

    steps = 37
    out = tmp_path / "o.bin"
    r = run_program([exe, str(rows), str(cols), str(steps), str(out)])
    assert r.returncode == 0, r.stderr
    data = np.fromfile(out, np.float32).reshape(2, rows, cols)
    f32 = np.float32
    feed = (f32(0.01) + f32(0.0005) * np.arange(rows, dtype=np.float32)[:, None] * np.ones((1, cols), np.float32)).astype(np.float32)
    kill = (f32(0.045) + f32(0.0002) * np.arange(cols, dtype=np.float32)[None, :] * np.ones((rows, 1), np.float32)).astype(np.float32)
    u, v = oracle.init_species(rows, cols)
    u, v = R.run(u, v, steps, feed, kill)
    assert data[0].tobytes() == v.tobytes(), "mapped steps differ from the reference"
    p = oracle.numpy_ref.default_params()
    u, v = R.run(u, v, steps, p["feed"], p["kill"])
    assert data[1].tobytes() == v.tobytes(), "steps after the map was detached differ from the reference"
