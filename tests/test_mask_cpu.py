"""Domain masks without a GPU: the masked reference of tests/mask_ref.py held to the literal per-cell loop (random masks,
all four rules, small and degenerate shapes, FTZ on and off), to the unmasked references (an all-fluid mask) and to the
identity (an all-wall mask); the new symbol is exported and declared, the ABI version is unchanged; the simulate driver's
``--hip-mask`` option and its refusal next to the parameter map's options."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

import oracle
from grayscott_amd import capi, simulate

from . import mask_ref as R
from .helpers import rule_run, stress_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = [R.CLIPPED, R.ZERO_HALO, R.PERIODIC, R.NEUMANN]


def random_mask(shape, rng, share=0.3):
    """Walls in about ``share`` of the cells, written as 1, -2.5 or NaN; fluid as +0 or -0."""
    m = np.where(rng.random(shape) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    walls = rng.random(shape) < share
    m[walls] = np.array([1.0, -2.5, np.nan], np.float32)[rng.integers(0, 3, int(walls.sum()))]
    return m


@pytest.mark.parametrize("ftz", [True, False])
@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 3), (4, 4), (5, 7), (9, 6)])
def test_vectorised_reference_is_the_literal_loop(shape, boundary, ftz):
    rng = np.random.default_rng(11)
    u, v = stress_fields(shape, 4)
    for trial in range(3):
        mask = random_mask(shape, rng, share=(0.2, 0.5, 0.8)[trial])
        prev = oracle.set_ftz(ftz)
        try:
            want = R.loop_step(u, v, mask, boundary=boundary)
            got = R.step(u, v, mask, boundary=boundary)
        finally:
            oracle.set_ftz(prev)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (trial, shape, boundary)
        u, v = want


@pytest.mark.parametrize("boundary", RULES)
def test_literal_loop_at_other_parameters(boundary):
    """A centre weight, asymmetric weights and dt != 1: every tap's weight and position matters."""
    p = oracle.numpy_ref.default_params()
    p["w"] = np.array([[0.25, 0.5, 0.125], [1.0, -3.0, 0.75], [0.0625, 0.375, 0.0]], np.float32)
    p["dt"] = np.float32(0.5)
    rng = np.random.default_rng(5)
    u, v = stress_fields((6, 5), 6)
    mask = random_mask((6, 5), rng)
    want = R.loop_step(u, v, mask, p, boundary)
    got = R.step(u, v, mask, p, boundary)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (3, 5), (17, 33)])
def test_all_fluid_mask_is_the_unmasked_rule(shape, boundary):
    u0, v0 = stress_fields(shape, 1)
    ref_u, ref_v = rule_run(u0, v0, 5, boundary=boundary)
    fluid = np.where(np.random.default_rng(2).random(shape) < 0.5, np.float32(0.0), np.float32(-0.0))
    for mask in (fluid, 0.0):
        got_u, got_v = R.run(u0, v0, 5, mask, boundary=boundary)
        assert got_u.tobytes() == ref_u.tobytes() and got_v.tobytes() == ref_v.tobytes()


@pytest.mark.parametrize("boundary", RULES)
def test_all_wall_mask_is_the_identity(boundary):
    u0, v0 = stress_fields((9, 11), 2)
    u0[0, 0] = np.float32(np.nan)
    for mask in (np.full((9, 11), np.nan, np.float32), 1.0):
        got_u, got_v = R.run(u0, v0, 3, mask, boundary=boundary)
        assert got_u.tobytes() == u0.tobytes() and got_v.tobytes() == v0.tobytes()


def test_walls_are_nonzero_cells():
    m = np.array([[0.0, -0.0, np.nan, 1e-45, -1.0, np.inf]], np.float32)
    assert R.walls_of(m).tolist() == [[False, False, True, True, True, True]]


def test_maze_walls_about_a_quarter_of_the_cells():
    m = R.maze((256, 256), np.random.default_rng(0))
    assert 0.2 < float(m.mean()) < 0.3


def test_the_symbol_is_exported_and_declared(built):
    assert "gs_ctx_set_mask" in capi.EXPORTS
    lib = ctypes.CDLL(os.path.join(ROOT, "grayscott_amd", "libgs_hip.so"))
    assert hasattr(lib, "gs_ctx_set_mask")
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    assert re.search(r"int32_t gs_ctx_set_mask\(gs_ctx \*ctx, gs_field \*mask\);", header)
    assert "pub fn gs_ctx_set_mask(" in open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    assert "set_mask(" in open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    lib.gs_abi_version.restype = ctypes.c_int32
    assert lib.gs_abi_version() == 4


def test_detach_without_a_context_is_refused(built):
    lib = capi.load()
    assert lib.gs_ctx_set_mask(None, None) == capi.GS_ERR_INVALID


def test_driver_option(tmp_path):
    m = (np.arange(24).reshape(4, 6) % 5 == 0).astype(np.int8)
    npy = tmp_path / "m.npy"
    np.save(npy, m)
    args = simulate.parse(["-r", "4", "-c", "6", "--hip-mask", str(npy)])
    got = simulate.domain_mask(args, (4, 6))
    assert got.shape == (4, 6) and (got == m).all()
    npz = tmp_path / "m.npz"
    np.savez(npz, mask=m.astype(np.float32))
    args = simulate.parse(["-r", "4", "-c", "6", "--hip-mask", str(npz)])
    assert (simulate.domain_mask(args, (4, 6)) == m).all()
    # no option: no mask
    args = simulate.parse([])
    assert simulate.domain_mask(args, (args.nbrow, args.nbcol)) is None
    # the wrong shape, a .npz without `mask`
    args = simulate.parse(["-r", "5", "-c", "6", "--hip-mask", str(npy)])
    with pytest.raises(ValueError):
        simulate.domain_mask(args, (5, 6))
    bad = tmp_path / "bad.npz"
    np.savez(bad, walls=m)
    with pytest.raises(ValueError):
        simulate.domain_mask(simulate.parse(["-r", "4", "-c", "6", "--hip-mask", str(bad)]), (4, 6))


@pytest.mark.parametrize("extra", [["--hip-feed-map", "0.01:0.05"], ["--hip-kill-map", "0.06:0.04"], ["--hip-param-map", "x.npz"]])
def test_driver_refuses_a_mask_with_a_parameter_map(tmp_path, extra):
    npy = tmp_path / "m.npy"
    np.save(npy, np.zeros((4, 6), np.float32))
    args = simulate.parse(["-r", "4", "-c", "6", "--hip-mask", str(npy)] + extra)
    with pytest.raises(ValueError, match="--hip-mask excludes"):
        simulate.domain_mask(args, (4, 6))
