"""Noise of ensembles without a GPU: the C ABI of gs_members_set_noise / gs_members_get_noise / gs_members_clear_noise
(declared, exported, bad arguments refused before any device work, no device = a loud failure), the noise forms of the
ensemble kernels in the built code objects (both flavours, all four rules, both forms, each within the budget of the kernels
without noise), the device-side step key's definition (tests/noise_ref.key against the restated generator), and the sweep's
--noise / --noise-seed / --realisations flags: parsing, the member order and the seeds."""
from __future__ import annotations

import ctypes
import os
import re
import sys

import numpy as np
import pytest

from tests.children import ROOT

from . import noise_ref as N

HEADER = os.path.join(ROOT, "include", "gs_hip.h")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

SYMBOLS = ("gs_members_set_noise", "gs_members_get_noise", "gs_members_clear_noise")


def test_entry_points_are_declared_and_exported(built):
    from grayscott_amd import capi

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = capi.load()
    for name in SYMBOLS:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", text), name
        assert name in capi.EXPORTS and hasattr(lib, name), name
    assert lib.gs_abi_version() == 4
    doc = open(HEADER).read()
    block = re.sub(r"\s*\n \*\s*", " ", doc[doc.index("/* Noise of an ensemble"):doc.index("int32_t gs_members_set_noise")])
    for word in ("gs_ctx_set_noise", "member-local", "wrapped", "gs_members_copy", "/noise", "/listed", "GS_ERR_UNSUPPORTED",
                 "-0 stays -0", "never contracted"):
        assert word in block, word
    assert "Ensembles ignore the noise" not in doc and "see gs_members_set_noise" in doc


def test_bad_arguments_are_refused_before_any_device_work(built):
    """Null handles fail first; with them nothing else is looked at, so the other INVALID cases of the header are reached
    on the GPU (tests/test_gpu_ensemble_noise.py)."""
    from grayscott_amd import capi

    lib = capi.load()
    n = (capi.GsNoise * 2)(capi.GsNoise(0.1, 0.2, 3, 4), capi.GsNoise(0.5, 0.6, 7, 8))
    attached = ctypes.c_int32(55)
    assert lib.gs_members_set_noise(None, None, 0, 2, n, 2) == capi.GS_ERR_INVALID
    assert b"null" in lib.gs_last_error()
    assert lib.gs_members_get_noise(None, None, 0, 2, n, ctypes.byref(attached)) == capi.GS_ERR_INVALID
    assert b"null" in lib.gs_last_error()
    assert lib.gs_members_clear_noise(None, None) == capi.GS_ERR_INVALID
    assert b"null" in lib.gs_last_error()
    assert attached.value == 55 and (n[0].sigma_u, n[1].seed, n[1].step) == (np.float32(0.1), 7, 8)  # nothing written
    assert ctypes.sizeof(capi.GsNoise) == 24


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_without_a_device_ensemble_noise_fails_loudly(built):
    from grayscott_amd import GsError, Parameters, Simulation, capi

    with pytest.raises(GsError) as e:
        ens = Simulation.new(Parameters()).make_ensemble((8, 16), [Parameters()] * 4)
        ens.set_noise(0.1)
    assert e.value.code == capi.GS_ERR_NO_DEVICE


def test_python_records_have_the_structs_layout():
    from grayscott_amd import capi
    from grayscott_amd.simulation import NOISE_DTYPE

    assert NOISE_DTYPE.itemsize == ctypes.sizeof(capi.GsNoise) == 24
    for name in NOISE_DTYPE.names:
        assert NOISE_DTYPE.fields[name][1] == getattr(capi.GsNoise, name).offset, name


def test_step_key_definition():
    """The key the kernels form on the device is gs_hip.h's key(s): the restatement on Python ints against the vectorised
    one, at steps on both sides of a carry into the high word and with seeds whose high word matters."""
    for (c0, c1, k), want in N.KNOWN_ANSWERS:
        assert N.philox_int(c0, c1, k) == want
    for seed in (0, 7, 0x1234567890ABCDEF, 2 ** 64 - 1):
        for s in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 64 - 1):
            x0, _ = N.philox(np.uint32(s & N.MASK32), np.uint32(s >> 32), np.uint32(seed & N.MASK32))
            assert N.key(seed, s) == int(x0) ^ (seed >> 32), (seed, s)
    assert N.key(5, 2 ** 64) == N.key(5, 0)  # the counter wraps


# ---- code objects ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels(built):
    return {re.sub(r"\(.*$", "", k.name): k for k in codeobj.kernels()}


# noise family -> the family without noise it is held against
PLAIN = {"gs_ens_resident_zk": "gs_ens_resident_k", "gs_ens_resident_zpk": "gs_ens_resident_pk",
         "gs_ens_resident_znk": "gs_ens_resident_nk", "gs_ens_tile_zk": "gs_ens_tile_k", "gs_ens_tile_zpk": "gs_ens_tile_pk",
         "gs_ens_tile_znk": "gs_ens_tile_nk"}


def noisy(kernels, flavour):
    out = {}
    for name, k in kernels.items():
        m = re.match(r"(gs_ens_(?:resident|tile)_z[pn]?k)_" + flavour + r"(<.*>)$", name)
        if m:
            out[name] = (k, kernels[PLAIN[m.group(1)] + "_" + flavour + m.group(2)])
    return out


def test_code_objects_hold_the_noise_forms_for_every_rule_form_and_flavour(kernels):
    strict, fused = noisy(kernels, "strict"), noisy(kernels, "fused")
    for n in ("gs_ens_resident_zk_strict<1, 3, 0>", "gs_ens_resident_zk_strict<4, 0, 0>", "gs_ens_resident_zk_strict<8, 3, 1>",
              "gs_ens_resident_zk_strict<8, 0, 1>", "gs_ens_resident_zpk_strict<8, 0>", "gs_ens_resident_znk_strict<1, 3>",
              "gs_ens_resident_znk_strict<8, 3>", "gs_ens_tile_zk_strict<2, 3>", "gs_ens_tile_zk_strict<1, 0>",
              "gs_ens_tile_zpk_strict<1, 0>", "gs_ens_tile_zpk_strict<4, 3>", "gs_ens_tile_znk_strict<4, 0>"):
        assert n in strict, n
    for n in ("gs_ens_resident_zk_fused<1, 0, 0>", "gs_ens_resident_zk_fused<8, 0, 1>", "gs_ens_resident_zpk_fused<4, 0>",
              "gs_ens_resident_znk_fused<8, 0>", "gs_ens_tile_zk_fused<2, 0>", "gs_ens_tile_zpk_fused<4, 0>",
              "gs_ens_tile_znk_fused<1, 0>"):
        assert n in fused, n
    # one noise form per kernel without noise (no listed twins: the list pointer is nullable), the resident capacity kept
    assert len(strict) == 48 and len(fused) == 24, (len(strict), len(fused))
    assert not any("<8, 0, 0>" in n or "<8, 3, 0>" in n for n in strict)  # no 8 cells per thread under the clipped rule
    # ... and the counts the other tests go by have not moved
    for flavour, plain, by_prefix in (("strict", 48, 20), ("fused", 24, 10)):
        assert len([n for n in kernels if re.match(r"gs_ens_(resident|tile)_[pn]?k_" + flavour + "<", n)]) == plain
        assert len([n for n in kernels if re.match(r"gs_ens_(resident|tile)_l[pn]?k_" + flavour + "<", n)]) == plain
        assert len([n for n in kernels if n.startswith(("gs_ens_resident_k_" + flavour, "gs_ens_tile_k_" + flavour))]) == by_prefix
    assert len([n for n in kernels if n.startswith("gs_members_mirror_k")]) == 2


@pytest.mark.parametrize("flavour", ["strict", "fused"])
def test_noise_forms_keep_the_budget(kernels, flavour):
    int_mul = r"^v_(mul_(lo|hi)_u32|mad_u64_u32)"
    for name, (k, plain) in noisy(kernels, flavour).items():
        assert k.vgpr <= 128 and k.agpr == 0, (name, k.vgpr)
        assert k.vgpr_spill == 0 and k.sgpr_spill == 0 and k.scratch == 0 and not k.dynamic_stack, name
        assert k.count(r"^scratch_") == 0, name
        assert k.count(r"^v_(readlane|writelane)_b32") == 0, name
        if flavour == "strict":
            assert k.count(codeobj.FLOAT_FMA) == 0, (name, k.matching(codeobj.FLOAT_FMA)[:3])
            assert k.denorm_mode_32 == 1, name
        else:  # no FMA that the kernel without noise lacks: the multiply and the add of the noise are not contracted
            assert 0 < k.count(codeobj.FLOAT_FMA) <= plain.count(codeobj.FLOAT_FMA) and k.denorm_mode_32 == 3, name
        # the cells are the only vector loads; the list entry, the parameters and the noise entry are scalar loads
        assert k.count(r"^global_load") == plain.count(r"^global_load"), (name, k.count(r"^global_load"))
        assert k.count(r"^s_load_dwordx(4|8)") >= 3, name
        assert k.lds == plain.lds, name
        # the generator is there, its rounds a loop (gs_cell.h), and the step key is formed with scalar multiplies
        assert k.count(int_mul) > plain.count(int_mul), name
        assert k.count(r"^s_mul_hi_u32") >= 1, name
        assert any(any(re.match(int_mul, i) for i in loop) for loop in k.loops()), name


# ---- the sweep's flags -----------------------------------------------------------------------------------------------
BASE = ["--feed", "0.01:0.02:2", "--kill", "0.05:0.06:2"]


def test_sweep_noise_flags():
    from grayscott_amd import sweep

    a = sweep.parse(BASE)
    assert a.noise is None and a.noise_seed == 0 and a.realisations == 1
    a = sweep.parse(BASE + ["--noise", "0.01"])
    assert a.noise == (0.01, 0.0) and a.realisations == 1
    a = sweep.parse(BASE + ["--noise", "0.01:0.005", "--noise-seed", "7", "--realisations", "3"])
    assert a.noise == (0.01, 0.005) and a.noise_seed == 7 and a.realisations == 3
    assert sweep.parse(BASE + ["--noise", "0:0"]).noise == (0.0, 0.0)  # zero sigmas are legal
    for bad in (["--realisations", "2"], ["--realisations", "0", "--noise", "0.1"], ["--noise", "-0.1"], ["--noise", "0.1:nan"],
                ["--noise", "inf"], ["--noise", "0.1:0.2:0.3"], ["--noise", "x"]):
        with pytest.raises(SystemExit):
            sweep.parse(BASE + bad)
    doc = " ".join(sweep.__doc__.split())
    for word in ("--noise SU[:SV]", "--noise-seed", "--realisations", "point * R + r", "common random numbers"):
        assert word in doc, word


def test_sweep_member_order_and_seeds():
    from grayscott_amd import sweep

    plain = sweep.parse(BASE)
    today = [(i * 2 + j, f, k) for i, k in enumerate(plain.kill) for j, f in enumerate(plain.feed)]
    assert sweep.members(plain) == today                                   # R = 1: the member list as it was
    assert sweep.members(sweep.parse(BASE + ["--noise", "0.1"])) == today  # ... with or without noise
    a = sweep.parse(BASE + ["--noise", "0.01:0.005", "--noise-seed", "7", "--realisations", "3"])
    got, seeds = sweep.members(a), sweep.member_seeds(a)
    assert len(got) == len(seeds) == 12 and [m[0] for m in got] == list(range(12))
    for point, (_, feed, kill) in enumerate(today):
        for r in range(3):
            assert got[point * 3 + r] == (point * 3 + r, feed, kill)
            assert seeds[point * 3 + r] == (r, 7 + r)
    assert len(sweep.member_params(a)) == 12
    # seeds are u64 and wrap
    a = sweep.parse(BASE + ["--noise", "0.1", "--noise-seed", str(2 ** 64 - 1), "--realisations", "2"])
    assert sweep.member_seeds(a)[:2] == [(0, 2 ** 64 - 1), (1, 0)]
