"""Ensembles without a GPU: the C ABI of gs_ensemble_* (declared, exported, null handles refused, no device = a loud
failure), the kernels' code objects (both flavours, register budget, no spills, no FMA in the strict ones, parameters
through scalar loads) and the sweep driver's member order."""
from __future__ import annotations

import ctypes
import json
import os
import re
import sys

import pytest

from tests.children import ROOT

HEADER = os.path.join(ROOT, "include", "gs_hip.h")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402


ENSEMBLE_SYMBOLS = {"gs_ensemble_create", "gs_ensemble_destroy", "gs_ensemble_shape", "gs_ensemble_set_params",
                    "gs_ensemble_seed", "gs_ensemble_upload", "gs_ensemble_download", "gs_ensemble_run"}


def test_every_ensemble_symbol_is_declared_and_exported(built):
    from grayscott_amd import capi

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(gs_ensemble_[a-z_]+)\s*\(", text))
    assert declared == ENSEMBLE_SYMBOLS
    assert ENSEMBLE_SYMBOLS <= set(capi.EXPORTS)
    lib = capi.load()
    for name in ENSEMBLE_SYMBOLS:
        assert hasattr(lib, name), name
    assert "typedef struct gs_ensemble gs_ensemble;" in text
    assert lib.gs_abi_version() == 4


def test_null_handles_are_refused(built):
    from grayscott_amd import capi

    lib = capi.load()
    INV = capi.GS_ERR_INVALID
    out = ctypes.c_void_p()
    p = capi.GsParams()
    buf = (ctypes.c_float * 16)()
    n = ctypes.c_uint64()
    assert lib.gs_ensemble_create(None, ctypes.byref(out), 4, 8, 16) == INV
    assert not out.value
    assert lib.gs_ensemble_shape(None, ctypes.byref(n), None, None) == INV
    assert lib.gs_ensemble_set_params(None, None, ctypes.byref(p), 1) == INV
    assert lib.gs_ensemble_seed(None, None) == INV
    assert lib.gs_ensemble_upload(None, None, 0, 1, buf, buf) == INV
    assert lib.gs_ensemble_download(None, None, 0, 1, 1, buf) == INV
    assert lib.gs_ensemble_run(None, None, 10) == INV
    assert b"null" in lib.gs_last_error()
    assert lib.gs_ensemble_destroy(None, None) == capi.GS_OK  # like gs_field_destroy: nothing to free


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_without_a_device_ensembles_fail_loudly(built):
    from grayscott_amd import GsError, Parameters, Simulation, capi

    with pytest.raises(GsError) as e:
        Simulation.new(Parameters()).make_ensemble((8, 16), [Parameters()] * 4)
    assert e.value.code == capi.GS_ERR_NO_DEVICE


@pytest.fixture(scope="module")
def kernels(built):
    return {k.name: k for k in codeobj.kernels()}


def ensemble_kernels(kernels, flavour):
    return {n: k for n, k in kernels.items() if n.startswith(("gs_ens_resident_k_" + flavour, "gs_ens_tile_k_" + flavour))}


def test_code_objects_hold_both_forms_in_both_flavours(kernels):
    strict, fused = ensemble_kernels(kernels, "strict"), ensemble_kernels(kernels, "fused")
    # resident: 1, 2, 4 cells per thread x both rules, 8 under the zero-halo rule; strict also the .op instances
    for n in ("gs_ens_resident_k_strict<1, 3, 0>", "gs_ens_resident_k_strict<4, 0, 0>", "gs_ens_resident_k_strict<8, 3, 1>",
              "gs_ens_tile_k_strict<2, 3>", "gs_ens_tile_k_strict<1, 0>", "gs_ens_tile_k_strict<4, 0>",
              "gs_ens_resident_k_fused<1, 0, 0>", "gs_ens_resident_k_fused<8, 0, 1>", "gs_ens_tile_k_fused<2, 0>"):
        assert any(k.startswith(n) for k in kernels), n
    assert len(strict) == 20 and len(fused) == 10, (sorted(strict), sorted(fused))


@pytest.mark.parametrize("flavour", ["strict", "fused"])
def test_guard_limits(kernels, flavour):
    for name, k in ensemble_kernels(kernels, flavour).items():
        assert k.vgpr <= 128 and k.agpr == 0, (name, k.vgpr)
        assert k.vgpr_spill == 0 and k.sgpr_spill == 0 and k.scratch == 0 and not k.dynamic_stack, name
        assert k.count(r"^scratch_") == 0, name
        assert k.count(r"^v_(readlane|writelane)_b32") == 0, name
        if flavour == "strict":
            assert k.count(codeobj.FLOAT_FMA) == 0, (name, k.matching(codeobj.FLOAT_FMA)[:3])
            assert k.denorm_mode_32 == 1, name
        else:
            assert k.count(codeobj.FLOAT_FMA) > 0 and k.denorm_mode_32 == 3, name


def test_member_parameters_come_through_scalar_loads(kernels):
    """A workgroup belongs to one member: its parameters are s_load'ed into SGPRs; the only vector loads are the cells
    (U and V, one per cell a thread or lane owns)."""
    for name, k in ensemble_kernels(kernels, "strict").items():
        m = re.match(r"gs_ens_(resident|tile)_k_strict<(\d+),", name)
        cells = int(m.group(2))  # cells per thread (resident) or rows per wave (tile)
        assert k.count(r"^global_load") == 2 * cells, (name, k.count(r"^global_load"))
        assert k.count(r"^s_load_dwordx(4|8)") >= 2, name


def test_sweep_members_are_kill_major(tmp_path):
    from grayscott_amd import sweep

    args = sweep.parse(["--feed", "0.01:0.03:3", "--kill", "0.05:0.06:2", "-r", "40", "-c", "64", "-s", "50", "-t", "0.5",
                        "--hip-boundary", "1", "-o", str(tmp_path / "s.h5")])
    got = sweep.members(args)
    assert [i for i, _, _ in got] == list(range(6))
    want = [(0.01, 0.05), (0.02, 0.05), (0.03, 0.05), (0.01, 0.06), (0.02, 0.06), (0.03, 0.06)]
    assert [f for _, f, _ in got] == pytest.approx([f for f, _ in want], rel=1e-12)
    assert [k for _, _, k in got] == pytest.approx([k for _, k in want], rel=1e-12)
    params = sweep.member_params(args)
    assert [(p.feed_rate, p.kill_rate, p.time_step) for p in params] == [(f, k, 0.5) for _, f, k in got]
    assert (args.steps, args.nbrow, args.nbcol) == (50, 40, 64)
    assert sweep.backend_args(args).boundary == 1
    assert sweep.sidecar_path(str(tmp_path / "s.h5")) == str(tmp_path / "s.json")
    assert sweep.value_range("0.1:0.2:1") == [0.1]
    for bad in ("0.1:0.2", "0.1:0.2:0"):
        with pytest.raises(Exception):
            sweep.value_range(bad)
    json.dumps(got)  # the sidecar's entries are plain numbers
