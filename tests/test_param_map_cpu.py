"""Parameter maps without a GPU: the mapped reference of tests/param_map_ref.py held to the C oracle (uniform maps under
every rule, maps constant within row bands through ``step_rows``) and to the literal per-cell loop (random maps, all four
rules) at parameters other than the defaults (power-of-two weights with a centre, the named stencils, other dt, du and
dv; with FTZ and without) and on maps holding +-0, zero kill, sub-normal feed and sub-normal feed + kill; the new symbol
is exported and declared, the ABI version is unchanged; the simulate driver's map options and
the linear formula."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

import oracle
from grayscott_amd import Parameters, capi, simulate

from . import param_map_ref as R
from .helpers import oracle_params, rule_run, stress_fields
from tests.children import ROOT

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


# Parameters other than the defaults: power-of-two weights with a centre, the reference's named stencils ("pretty", a
# centre weight of 1, with dt = 0.25), dt of 0.5, 0.75 and 2, other diffusion rates
PARAMS = [Parameters(weights=((0.125, 0.5, 0.25), (1.0, 0.5, 0.5), (0.25, 0.5, 0.0)), diffusion_rate_u=0.2, diffusion_rate_v=0.1),
          Parameters.with_stencil("5points"), Parameters.with_stencil("patrakarttunen"),
          Parameters.with_stencil("pretty", time_step=0.25),
          Parameters(time_step=0.5), Parameters(time_step=0.75),
          Parameters(weights=((0.25, 0.5, 0.125), (0.5, 0.25, 0.5), (0.0, 0.5, 0.25)), time_step=2.0),
          Parameters(diffusion_rate_u=0.05, diffusion_rate_v=0.1)]
PARAM_IDS = ["pow2-centre", "5points", "patrakarttunen", "pretty", "dt0.5", "dt0.75", "dt2", "du-dv"]


def _loop(u, v, feed, kill, params, boundary, ftz):
    prev = oracle.set_ftz(ftz)
    try:
        return R.loop_step(u, v, feed, kill, params, boundary=boundary)
    finally:
        oracle.set_ftz(prev)


@pytest.mark.parametrize("ftz", [True, False])
@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("p", PARAMS, ids=PARAM_IDS)
def test_random_map_is_the_literal_loop_at_any_parameters(p, boundary, ftz):
    q = R.params_of(p)
    rng = np.random.default_rng(4)
    for shape in ((1, 1), (2, 3), (4, 4), (5, 7)):
        u, v = stress_fields(shape, 4)
        feed = rng.uniform(0.01, 0.06, shape).astype(np.float32)
        kill = rng.uniform(0.04, 0.07, shape).astype(np.float32)
        for _ in range(3):
            nu, nv = R.run(u, v, 1, feed, kill, params=q, boundary=boundary, ftz=ftz)
            lu, lv = _loop(u, v, feed, kill, q, boundary, ftz)
            assert nu.tobytes() == lu.tobytes() and nv.tobytes() == lv.tobytes(), (shape, p)
            u, v = nu, nv


@pytest.mark.parametrize("ftz", [True, False])
@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("p", [Parameters()] + PARAMS[:1] + PARAMS[4:5], ids=["default", "pow2-centre", "dt0.5"])
def test_edge_rates_are_the_literal_loop(p, boundary, ftz):
    """Maps holding +-0, zero kill, sub-normal feed and feed + kill that rounds to a sub-normal (R.EDGE_RATES), on states
    with sub-normal values sprinkled in: the sub-normal F + K is flushed under FTZ, kept without it, in both."""
    q = R.params_of(p)
    rng = np.random.default_rng(5)
    for shape in ((1, 1), (3, 4), (6, 5)):
        u, v = stress_fields(shape, 5)
        v[rng.random(shape) < 0.3] *= np.float32(1e-37)
        u[rng.random(shape) < 0.1] = np.float32(3e-38)
        feed, kill = R.planted_map(shape, rng, share=0.6)
        for _ in range(3):
            nu, nv = R.run(u, v, 1, feed, kill, params=q, boundary=boundary, ftz=ftz)
            lu, lv = _loop(u, v, feed, kill, q, boundary, ftz)
            assert nu.tobytes() == lu.tobytes() and nv.tobytes() == lv.tobytes(), (shape, p)
            u, v = nu, nv


def test_planted_map_holds_every_edge_rate():
    feed, kill = R.planted_map((40, 50), np.random.default_rng(6))
    pairs = {(float(f).hex(), float(k).hex()) for f, k in zip(feed.ravel(), kill.ravel())}
    for f, k in R.EDGE_RATES:
        assert (float(np.float32(f)).hex(), float(np.float32(k)).hex()) in pairs, (f, k)
    with np.errstate(all="ignore"):
        fpk = feed + kill
    assert R.has_subnormal(feed) and R.has_subnormal(fpk)
    assert not R.has_subnormal(*R.planted_map((40, 50), np.random.default_rng(6), share=0.0))


@pytest.mark.parametrize("ftz", [True, False])
@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("p", PARAMS, ids=PARAM_IDS)
def test_uniform_map_is_the_oracle_at_any_parameters(p, boundary, ftz):
    for shape in ((1, 1), (1, 7), (7, 1), (3, 5), (17, 33)):
        u0, v0 = stress_fields(shape, 7)
        ref_u, ref_v = rule_run(u0, v0, 5, oracle_params(p), boundary, ftz=ftz)
        got_u, got_v = R.run(u0, v0, 5, p.feed_rate, p.kill_rate, params=R.params_of(p), boundary=boundary, ftz=ftz)
        assert got_u.tobytes() == ref_u.tobytes() and got_v.tobytes() == ref_v.tobytes(), shape


def test_the_map_property_strategy_draws_legal_cases_of_every_kind():
    """The cases tests/test_gpu_param_map_property.py draws (no library call): legal option sets after the refusals, and
    every rule, flavour, K, CPL, kernel, delivery and map kind among a few hundred of them."""
    from hypothesis import HealthCheck, given, settings

    from .test_gpu_param_map_property import EDGE_EXAMPLES, legal, map_cases

    seen = set()

    @settings(max_examples=400, deadline=None, database=None, suppress_health_check=list(HealthCheck))
    @given(map_cases())
    def draw(case):
        kernel, fuse, _, _, _, _, _ = legal(case)
        seen.update({("rule", case["boundary"]), ("math", case["math"]), ("k", fuse), ("cpl", case["cpl"]),
                     ("kernel", case["kernel"]), ("delivery", case["delivery"]), ("map", case["map"]),
                     ("ran", kernel)})

    draw()
    for case in EDGE_EXAMPLES:
        legal(case)
    want = ({("rule", b) for b in RULES} | {("math", m) for m in (capi.GS_MATH_STRICT, capi.GS_MATH_FUSED)}
            | {("k", k) for k in range(5)} | {("cpl", c) for c in (0, 1, 2, 4)}
            | {("kernel", k) for k in (capi.GS_KERNEL_AUTO, capi.GS_KERNEL_TB, capi.GS_KERNEL_STREAM, capi.GS_KERNEL_SIMPLE,
                                       capi.GS_KERNEL_TILE, capi.GS_KERNEL_WINDOW, capi.GS_KERNEL_LDS)}
            | {("delivery", d) for d in ("run", "calls", "step")}
            | {("map", m) for m in ("random", "uniform", "row-bands", "col-bands", "planted")})
    assert want <= seen, sorted(want - seen)
    assert not {("ran", k) for k in (capi.GS_KERNEL_TILE, capi.GS_KERNEL_WINDOW, capi.GS_KERNEL_LDS)} & seen


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
