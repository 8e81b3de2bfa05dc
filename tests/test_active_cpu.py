"""Active sets of ensembles without a GPU: the C ABI of gs_members_set_active / gs_members_get_active (declared, exported,
null handles refused, no device = a loud failure), the listed forms of the ensemble kernels in the built code objects (both
flavours, each held to the limits of its twin), the mirror kernel, the sweep's --steady-retire flag and its retire mask, and
the C++ mirror's build."""
from __future__ import annotations

import ctypes
import os
import re
import sys

import numpy as np
import pytest

from tests.children import ROOT, build_program, run_program

HEADER = os.path.join(ROOT, "include", "gs_hip.h")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402


SYMBOLS = ("gs_members_set_active", "gs_members_get_active")
# listed family -> its twin
TWINS = {"gs_ens_resident_lk": "gs_ens_resident_k", "gs_ens_resident_lpk": "gs_ens_resident_pk",
         "gs_ens_resident_lnk": "gs_ens_resident_nk", "gs_ens_tile_lk": "gs_ens_tile_k", "gs_ens_tile_lpk": "gs_ens_tile_pk",
         "gs_ens_tile_lnk": "gs_ens_tile_nk"}


def test_both_entry_points_are_declared_and_exported(built):
    from grayscott_amd import capi

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = capi.load()
    for name in SYMBOLS:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", text), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
    assert lib.gs_abi_version() == 4
    # the comment beside them says what inactive means, what readers see and what writers do
    doc = open(HEADER).read()
    block = doc[doc.index("/* Active sets"):doc.index("int32_t gs_members_set_active")]
    for word in ("gs_ensemble_seed", "gs_ensemble_upload", "gs_ensemble_set_params", "gs_members_copy", "/listed",
                 "neither copied", "GS_ERR_UNSUPPORTED"):
        assert word in block, word


def test_null_handles_are_refused(built):
    from grayscott_amd import capi

    lib = capi.load()
    flags = (ctypes.c_uint8 * 4)(1, 0, 1, 0)
    steps = (ctypes.c_uint64 * 4)()
    total = ctypes.c_uint64(77)
    assert lib.gs_members_set_active(None, None, 0, 4, flags) == capi.GS_ERR_INVALID
    assert b"null" in lib.gs_last_error()
    assert lib.gs_members_get_active(None, None, 0, 4, flags, steps, ctypes.byref(total)) == capi.GS_ERR_INVALID
    assert b"null" in lib.gs_last_error()
    assert total.value == 77 and list(flags) == [1, 0, 1, 0]  # nothing written


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_without_a_device_active_sets_fail_loudly(built):
    """No context can exist, so no ensemble to retire members of: the way to one fails with GS_ERR_NO_DEVICE, not quietly."""
    from grayscott_amd import GsError, Parameters, Simulation, capi

    with pytest.raises(GsError) as e:
        ens = Simulation.new(Parameters()).make_ensemble((8, 16), [Parameters()] * 4)
        ens.retire([1])
    assert e.value.code == capi.GS_ERR_NO_DEVICE


@pytest.fixture(scope="module")
def kernels(built):
    return {re.sub(r"\(.*$", "", k.name): k for k in codeobj.kernels()}


def waves_per_simd(vgpr: int) -> int:
    """512 registers per lane and SIMD, allocated in steps of 8, at most 8 waves."""
    return min(8, 512 // (((vgpr + 7) // 8) * 8))


def listed(kernels, flavour):
    out = {}
    for name, k in kernels.items():
        m = re.match(r"(gs_ens_(?:resident|tile)_l[pn]?k)_" + flavour + r"(<.*>)$", name)
        if m:
            out[name] = (k, kernels[TWINS[m.group(1)] + "_" + flavour + m.group(2)])
    return out


def test_code_objects_hold_the_listed_forms_in_both_flavours(kernels):
    strict, fused = listed(kernels, "strict"), listed(kernels, "fused")
    for n in ("gs_ens_resident_lk_strict<1, 3, 0>", "gs_ens_resident_lk_strict<4, 0, 0>", "gs_ens_resident_lk_strict<8, 3, 1>",
              "gs_ens_resident_lpk_strict<8, 0>", "gs_ens_resident_lnk_strict<1, 3>", "gs_ens_tile_lk_strict<2, 3>",
              "gs_ens_tile_lpk_strict<1, 0>", "gs_ens_tile_lnk_strict<4, 0>"):
        assert n in strict, n
    for n in ("gs_ens_resident_lk_fused<1, 0, 0>", "gs_ens_resident_lk_fused<8, 0, 1>", "gs_ens_resident_lpk_fused<4, 0>",
              "gs_ens_resident_lnk_fused<8, 0>", "gs_ens_tile_lk_fused<2, 0>", "gs_ens_tile_lpk_fused<4, 0>",
              "gs_ens_tile_lnk_fused<1, 0>"):
        assert n in fused, n
    assert not any("<8, 0, 0>" in n or "<8, 3, 0>" in n for n in strict)  # no 8 cells per thread under the clipped rule
    # one listed form per twin: the same instance set
    for flavour, got in (("strict", strict), ("fused", fused)):
        twins = [n for n in kernels if re.match(r"gs_ens_(resident|tile)_[pn]?k_" + flavour + "<", n)]
        assert len(got) == len(twins) and len(got) == (48 if flavour == "strict" else 24), (flavour, len(got), len(twins))
    # the twins keep the names the ensemble tests count by prefix
    assert not any(n.startswith(("gs_ens_resident_k_", "gs_ens_tile_k_")) for n in list(strict) + list(fused))


@pytest.mark.parametrize("flavour", ["strict", "fused"])
def test_listed_forms_are_held_to_their_twins_limits(kernels, flavour):
    for name, (k, twin) in listed(kernels, flavour).items():
        assert k.vgpr <= 128 and k.agpr == 0, (name, k.vgpr)
        assert waves_per_simd(k.vgpr) == waves_per_simd(twin.vgpr), (name, k.vgpr, twin.vgpr)
        assert k.vgpr_spill == 0 and k.sgpr_spill == 0 and k.scratch == 0 and not k.dynamic_stack, name
        assert k.count(r"^scratch_") == 0, name
        assert k.count(r"^v_(readlane|writelane)_b32") == 0, name
        if flavour == "strict":
            assert k.count(codeobj.FLOAT_FMA) == 0, (name, k.matching(codeobj.FLOAT_FMA)[:3])
            assert k.denorm_mode_32 == 1, name
        else:
            assert k.count(codeobj.FLOAT_FMA) > 0 and k.denorm_mode_32 == 3, name
        # the cells are the only vector loads, as many as the twin's: the list entry and the parameters are scalar loads
        cells = int(re.search(r"<(\d+),", name).group(1))
        assert k.count(r"^global_load") == twin.count(r"^global_load") == 2 * cells, (name, k.count(r"^global_load"))
        assert k.count(r"^s_load_dword ") >= 1 and k.count(r"^s_load_dwordx(4|8)") >= 2, name
        assert k.lds == twin.lds, name


def test_mirror_kernel(kernels):
    found = {n: k for n, k in kernels.items() if n.startswith("gs_members_mirror_k")}
    assert len(found) == 2, sorted(found)  # 16 bytes per lane, and the dword path
    for name, k in found.items():
        assert k.scratch == 0 and k.vgpr_spill == 0 and k.sgpr_spill == 0 and not k.dynamic_stack, name
        assert k.lds == 0 and k.count(r"^ds_") == 0, name
        assert k.count(r"atomic") == 0 and not any("atomic" in i for i in k.insts), name
    wide = [k for k in found.values() if k.count(r"^global_load_dwordx4") and k.count(r"^global_store_dwordx4")]
    narrow = [k for k in found.values() if k.count(r"^global_load_dword ") and k.count(r"^global_store_dword ")]
    assert len(wide) == 1 and len(narrow) == 1 and wide[0] is not narrow[0]


BASE = ["--feed", "0.01:0.02:2", "--kill", "0.05:0.05:1"]


def test_sweep_steady_retire_flag():
    from grayscott_amd import sweep

    assert not sweep.parse(BASE + ["-s", "10"]).steady_retire
    assert not sweep.parse(BASE + ["--steady-every", "4"]).steady_retire
    a = sweep.parse(BASE + ["--steady-every", "4", "--steady-tol", "1e-3", "--steady-retire"])
    assert a.steady_retire and a.steady_every == 4 and a.steady_tol == 1e-3 and not a.steady_stop
    assert sweep.parse(BASE + ["--steady-every", "4", "--steady-retire", "--steady-stop"]).steady_stop
    for bad in (["--steady-retire"], ["--steady-retire", "--steady-tol", "1"], ["--steady-retire", "--summary-every", "5"]):
        with pytest.raises(SystemExit):
            sweep.parse(BASE + bad)
    assert "--steady-retire" in sweep.__doc__ and "Members do not stop one by one: all advance" not in sweep.__doc__


def test_sweep_retire_mask():
    from grayscott_amd import sweep
    from grayscott_amd.simulation import CHANGE_DTYPE

    rec = np.zeros((5, 2), CHANGE_DTYPE)
    rec["max_abs"] = [[0.0, 0.0],        # at rest
                      [0.5, 0.5],        # exactly the tolerance: settled
                      [0.5, 0.6],        # V still moves
                      [0.6, 0.0],        # U still moves
                      [np.nan, 0.0]]     # nothing comparable to say: not settled
    rec["differing"] = 7                 # (bits that differ do not matter, the values do)
    got = sweep.retire_mask(rec, 0.5)
    assert got.dtype == np.bool_ and got.tolist() == [True, True, False, False, False]
    assert sweep.retire_mask(rec, 0.0).tolist() == [True, False, False, False, False]
    assert sweep.retire_mask(rec, np.inf).tolist() == [True, True, True, True, False]
    # the mask of one check is the last column of what settled_steps reads
    steps = [5, 10]
    max_abs = np.stack([np.ones((5, 2)), rec["max_abs"]], axis=1)
    assert ((sweep.settled_steps(steps, max_abs, 0.5) == 10) == got).all()


def test_cpp_active_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("active_mirror", tmp_path)
    hpp = open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    for name in ("void set_active(", "std::vector<uint8_t> active()", "std::vector<uint64_t> steps_taken()"):
        assert name in hpp, name
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_active.py)
        r = run_program([str(exe), "4", "8", "16", "5", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
