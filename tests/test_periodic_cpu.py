"""The periodic boundary rule without a GPU: the constant in capi, the --hip-boundary 2 flag of simulate and sweep, the
pad-and-crop reference against a literal per-cell modulo loop, and the rule's kernels in the code objects (present,
spill-free, scratch-free, no FMA in the strict flavour)."""
from __future__ import annotations

import os
import re
import sys

import numpy as np
import pytest

from oracle import numpy_ref

from . import periodic_ref
from .helpers import stress_fields
from tests.children import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402


def test_the_constant_is_in_capi_and_in_the_header():
    from grayscott_amd import capi

    assert (capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_PERIODIC) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    assert re.search(r"enum gs_boundary \{[^}]*GS_BOUNDARY_PERIODIC = 2", header)


def test_the_flag_goes_through_simulate_and_sweep(tmp_path):
    from grayscott_amd import simulate, sweep

    args = simulate.parse(["--hip-boundary", "2", "-r", "64", "-c", "128", "-n", "3", "-e", "32", "-o", str(tmp_path / "p.h5")])
    assert simulate.backend_args(args).boundary == 2
    args = sweep.parse(["--feed", "0.01:0.03:3", "--kill", "0.05:0.06:2", "-r", "40", "-c", "64", "-s", "50",
                        "--hip-boundary", "2", "-o", str(tmp_path / "s.h5")])
    assert sweep.backend_args(args).boundary == 2


def test_the_help_text_names_the_rule(capsys):
    from grayscott_amd import simulate

    with pytest.raises(SystemExit):
        simulate.parse(["--help"])
    assert "2 = periodic" in " ".join(capsys.readouterr().out.split())


SHAPES = [(r, c) for r in range(1, 6) for c in range(1, 8)]


@pytest.mark.parametrize("shape", SHAPES)
def test_pad_and_crop_is_the_modulo_rule(shape):
    u, v = stress_fields(shape, 7 + shape[0] * 10 + shape[1])
    steps = 4
    mu, mv = u, v
    for n in range(1, steps + 1):
        mu, mv = periodic_ref.mod_step(mu, mv)
        for got, what in ((periodic_ref.run_numpy(u, v, n), "numpy, pad 1 per step"),
                          (periodic_ref.run(u, v, n), "C oracle, pad 1 per step"),
                          (periodic_ref.run_padded(u, v, n), f"C oracle, pad {n}")):
            assert got[0].tobytes() == mu.tobytes() and got[1].tobytes() == mv.tobytes(), (shape, n, what)


def test_the_rule_differs_from_the_other_two_and_is_translation_invariant():
    import oracle

    u, v = stress_fields((9, 13), 3)
    pu, pv = periodic_ref.run(u, v, 5)
    for rule in (oracle.CLIPPED, oracle.ZERO_HALO):
        ru, rv = oracle.run(u, v, 5, ftz=True, boundary=rule)
        assert ru.tobytes() != pu.tobytes()
    su, sv = periodic_ref.run(np.roll(u, (4, -3), (0, 1)), np.roll(v, (4, -3), (0, 1)), 5)
    assert np.roll(su, (-4, 3), (0, 1)).tobytes() == pu.tobytes() and np.roll(sv, (-4, 3), (0, 1)).tobytes() == pv.tobytes()


# ---- the kernels in the code objects ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernels(built):
    return {k.name: k for k in codeobj.kernels()}


PERIODIC = re.compile(r"^gs_[a-z_]+_pk_(strict|fused)\b")


def periodic_kernels(kernels, flavour):
    return {n: k for n, k in kernels.items() if PERIODIC.match(n) and f"_pk_{flavour}" in n}


def test_every_periodic_kernel_is_there(kernels):
    strict, fused = periodic_kernels(kernels, "strict"), periodic_kernels(kernels, "fused")
    for n in ("gs_step_simple_pk_strict", "gs_step_stream_pk_strict<2>", "gs_run_resident_pk_strict<3>",
              "gs_run_resident_pk_strict<0>", "gs_run_tile_pk_strict<2, 3>", "gs_run_tile_pk_strict<1, 0>",
              "gs_run_tile_pk_strict<4, 0>", "gs_ens_resident_pk_strict<8, 3>", "gs_ens_resident_pk_strict<1, 0>",
              "gs_ens_tile_pk_strict<2, 3>", "gs_ens_tile_pk_strict<4, 0>",
              "gs_step_simple_pk_fused", "gs_step_stream_pk_fused<2>", "gs_run_resident_pk_fused<0>",
              "gs_run_tile_pk_fused<1, 0>", "gs_ens_resident_pk_fused<8, 0>", "gs_ens_tile_pk_fused<2, 0>",
              "gs_step_tb_pk_fused<4, 0, 1, 16>"):
        assert any(k == n or k.startswith(n + "(") for k in kernels), n
    # the marching kernel: K = 1..4 x 1, 2, 4 columns per lane, general and .op variants, the 16-wave forms and the
    # variants with full difference sharing (within and across lanes)
    for k in range(1, 5):
        for cpl in (1, 2, 4):
            for fast in (0, 1, 3):
                assert f"gs_step_tb_pk_strict<{k}, {fast}, {cpl}, 4>" in strict, (k, fast, cpl)
            assert f"gs_step_tb_pk_fused<{k}, 0, {cpl}, 4>" in fused, (k, cpl)
    for fast in (0, 1, 3):
        for cpl in (1, 2):
            assert f"gs_step_tb_pk_strict<4, {fast}, {cpl}, 16>" in strict
    for form in ("ds", "dx"):
        for k in (2, 3, 4):
            assert f"gs_step_tb_{form}_pk_strict<{k}, 4>" in kernels
        assert f"gs_step_tb_{form}_pk_strict<4, 16>" in kernels
    assert len(strict) == 74 and len(fused) == 26, (len(strict), len(fused))


@pytest.mark.parametrize("flavour", ["strict", "fused"])
def test_periodic_kernels_do_not_spill(kernels, flavour):
    ks = {n: k for n, k in kernels.items() if "_pk_" + flavour in n}
    assert ks
    for name, k in ks.items():
        assert k.vgpr_spill == 0 and k.sgpr_spill == 0 and k.scratch == 0 and not k.dynamic_stack, (name, k.vgpr_spill, k.sgpr_spill)
        assert k.count(r"^scratch_") == 0, name
        assert k.count(r"^v_(readlane|writelane)_b32") == 0, name
        if flavour == "strict":
            assert k.count(codeobj.FLOAT_FMA) == 0, (name, k.matching(codeobj.FLOAT_FMA)[:3])
            assert k.denorm_mode_32 == 1, name
        else:
            assert k.denorm_mode_32 == 3, name


def test_periodic_marching_kernels_keep_the_register_budget_of_their_clipped_twins(kernels):
    """The periodic march runs the interior cell code in its edge units: it runs as many waves per SIMD as the kernel of
    the other rules with the same template arguments (512 registers, allocated in steps of 8), and the forms built for
    four waves per SIMD stay at 128 registers."""
    def waves(vgpr):
        return min(8, 512 // ((vgpr + 7) // 8 * 8))

    seen = 0
    for name, k in kernels.items():
        m = re.match(r"^gs_step_tb(_ds|_dx)?_pk_(strict|fused)(<.*)$", name)
        if not m:
            continue
        twin = kernels[f"gs_step_tb{m.group(1) or ''}_k_{m.group(2)}{m.group(3)}"]
        assert waves(k.vgpr) >= waves(twin.vgpr), (name, k.vgpr, twin.vgpr)
        if m.group(1) or twin.vgpr <= 128:
            assert k.vgpr <= 128, (name, k.vgpr)
        seen += 1
    assert seen == 63, seen
