"""Parameter maps without a GPU: the mapped reference of tests/param_map_ref.py held to the C oracle (uniform maps under
every rule, maps constant within row bands through ``step_rows``) and to the literal per-cell loop (random maps, all four
rules); the new symbol is exported and declared, the ABI version is unchanged; the simulate driver's map options and
the linear formula."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

import oracle
from grayscott_amd import capi, simulate

from . import param_map_ref as R
from .helpers import rule_run, stress_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = [R.CLIPPED, R.ZERO_HALO, R.PERIODIC, R.NEUMANN]


@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (3, 5), (17, 33), (64, 40)])
def test_uniform_map_is_the_oracle(shape, boundary):
    u0, v0 = stress_fields(shape, 1)
    p = oracle.numpy_ref.default_params()
    ref_u, ref_v = rule_run(u0, v0, 5, boundary=boundary)
    got_u, got_v = R.run(u0, v0, 5, p["feed"], p["kill"], boundary=boundary)
    assert got_u.tobytes() == ref_u.tobytes() and got_v.tobytes() == ref_v.tobytes()


@pytest.mark.parametrize("shape,bands", [((12, 20), [0, 4, 9, 12]), ((30, 17), [0, 1, 15, 30]), ((5, 8), [0, 5])])
def test_row_band_map_is_step_rows(shape, bands):
    """A map constant within row bands = the C oracle's step_rows, band by band, with that band's scalar rates."""
    u, v = stress_fields(shape, 2)
    rates = [(0.01 + 0.01 * i, 0.045 + 0.005 * i) for i in range(len(bands) - 1)]
    feed, kill = np.empty(shape, np.float32), np.empty(shape, np.float32)
    for (r0, r1), (f, k) in zip(zip(bands, bands[1:]), rates):
        feed[r0:r1], kill[r0:r1] = np.float32(f), np.float32(k)
    ref_u, ref_v = u.copy(), v.copy()
    for _ in range(4):
        nu, nv = np.empty_like(ref_u), np.empty_like(ref_v)
        for (r0, r1), (f, k) in zip(zip(bands, bands[1:]), rates):
            q = oracle.default_params()
            q.feed, q.kill = np.float32(f), np.float32(k)
            oracle.step_rows(ref_u, ref_v, nu, nv, q, r0, r1)
        ref_u, ref_v = nu, nv
    got_u, got_v = R.run(u, v, 4, feed, kill)
    assert got_u.tobytes() == ref_u.tobytes() and got_v.tobytes() == ref_v.tobytes()


@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (4, 4), (5, 7)])
def test_random_map_is_the_literal_loop(shape, boundary):
    rng = np.random.default_rng(3)
    u, v = stress_fields(shape, 3)
    feed = rng.uniform(0.01, 0.06, shape).astype(np.float32)
    kill = rng.uniform(0.04, 0.07, shape).astype(np.float32)
    for _ in range(3):
        nu, nv = R.run(u, v, 1, feed, kill, boundary=boundary)
        prev = oracle.set_ftz(True)
        try:
            lu, lv = R.loop_step(u, v, feed, kill, boundary=boundary)
        finally:
            oracle.set_ftz(prev)
        assert nu.tobytes() == lu.tobytes() and nv.tobytes() == lv.tobytes()
        u, v = nu, nv


def test_the_symbol_is_exported_and_declared(built):
    assert "gs_ctx_set_param_map" in capi.EXPORTS
    lib = ctypes.CDLL(os.path.join(ROOT, "grayscott_amd", "libgs_hip.so"))
    assert hasattr(lib, "gs_ctx_set_param_map")
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    assert re.search(r"int32_t gs_ctx_set_param_map\(gs_ctx \*ctx, gs_field \*feed, gs_field \*kill\);", header)
    assert "fn gs_ctx_set_param_map(" in open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    assert "set_param_map(" in open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    lib.gs_abi_version.restype = ctypes.c_int32
    assert lib.gs_abi_version() == 4


def test_detach_without_a_context_is_refused(built):
    lib = capi.load()
    assert lib.gs_ctx_set_param_map(None, None, None) == capi.GS_ERR_INVALID


def test_linear_formula():
    for a, b, n in ((0.01, 0.05, 1), (0.01, 0.05, 2), (0.01, 0.05, 1080), (0.07, 0.045, 7)):
        got = simulate.linear_values(a, b, n)
        want = np.array([np.float32(a + (b - a) * i / (n - 1)) if n > 1 else np.float32(a) for i in range(n)], np.float32)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
        assert got.tobytes() == R.linear(a, b, n).tobytes()
    assert simulate.linear_values(0.01, 0.05, 5)[0] == np.float32(0.01)
    assert simulate.linear_values(0.01, 0.05, 5)[-1] == np.float32(0.05)


def test_driver_options(tmp_path):
    args = simulate.parse(["-r", "4", "-c", "6", "--hip-feed-map", "0.01:0.05", "--hip-kill-map", "0.06:0.04"])
    p = simulate.simulation_parameters(args)
    feed, kill, d = simulate.param_map(args, (4, 6), p)
    assert feed.shape == kill.shape == (4, 6)
    assert (feed == R.linear(0.01, 0.05, 4)[:, None]).all() and (kill == R.linear(0.06, 0.04, 6)[None, :]).all()
    assert d["feed"] == {"along": "rows", "from": 0.01, "to": 0.05} and d["kill"]["along"] == "columns"
    # one option: the other rate stays the uniform -f / -k value
    args = simulate.parse(["-r", "4", "-c", "6", "-k", "0.055", "--hip-feed-map", "0.01:0.05"])
    feed, kill, d = simulate.param_map(args, (4, 6), simulate.simulation_parameters(args))
    assert np.ndim(kill) == 0 and kill == np.float32(0.055) and d["kill"] == {"value": 0.055}
    # a file
    path = tmp_path / "m.npz"
    np.savez(path, feed=np.full((4, 6), 0.02, np.float32), kill=np.full((4, 6), 0.05, np.float32))
    args = simulate.parse(["-r", "4", "-c", "6", "--hip-param-map", str(path)])
    feed, kill, d = simulate.param_map(args, (4, 6), simulate.simulation_parameters(args))
    assert feed.shape == (4, 6) and d["file"].endswith("m.npz")
    for bad in (["--hip-param-map", str(path), "--hip-feed-map", "0:1"], ["-r", "5", "--hip-param-map", str(path)],
                ["--hip-feed-map", "0.01"]):
        a = simulate.parse(["-c", "6"] + bad)
        with pytest.raises(ValueError):
            simulate.param_map(a, (a.nbrow, 6), simulate.simulation_parameters(a))
    # no option: no map
    args = simulate.parse([])
    assert simulate.param_map(args, (args.nbrow, args.nbcol), simulate.simulation_parameters(args)) is None
    assert simulate.sidecar_path("out.h5") == "out.param_map.json"
