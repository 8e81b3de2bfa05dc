"""The quiet entries of the marching kernel (gs_step_tb_dx_qk: units at rest are not recomputed) in the gfx950 code objects
of the built ``libgs_hip.so`` (no GPU needed), beside tests/test_isa_guard.py: each is its production twin
(``gs_step_tb_dx_k_strict<K, 4>``) plus the words' reads, the check and one more instance of the interior march, and must
keep the twin's occupancy -- four waves per SIMD, nothing spilled -- and its LDS."""
from __future__ import annotations

import os
import sys

import pytest

from tests.children import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

# K fused steps -> LDS bytes of the production twin (the halo boards: tests/test_isa_guard.py, SHIPPED)
QUIET = {4: 16640, 3: 12480, 2: 8320}


@pytest.fixture(scope="module")
def kernels(built):
    return {k.name: k for k in codeobj.kernels()}


@pytest.mark.parametrize("k", sorted(QUIET))
def test_quiet_entries_keep_their_twins_occupancy(kernels, k):
    name, twin = f"gs_step_tb_dx_qk_strict<{k}>", f"gs_step_tb_dx_k_strict<{k}, 4>"
    q, t = kernels[name], kernels[twin]
    assert q.vgpr <= 128 and q.agpr == 0, (name, q.vgpr, q.agpr)
    assert q.vgpr_spill == 0 and q.sgpr_spill == 0, (name, q.vgpr_spill, q.sgpr_spill)
    assert q.scratch == 0 and not q.dynamic_stack and q.count(r"^scratch_") == 0, (name, q.scratch)
    assert q.count(r"^v_(readlane|writelane)_b32") == 0, name
    assert q.lds == QUIET[k] == t.lds, (name, q.lds, t.lds)
    assert q.denorm_mode_32 == 1 and q.count(codeobj.FLOAT_FMA) == 0, name
    # the check is there (integer compares of the stored words, gathered in scalar registers) and the skip count is one
    # vector atomic
    assert q.count(r"^v_cmp_(ne|eq)_u32") > t.count(r"^v_cmp_(ne|eq)_u32"), name
    assert q.count(r"^global_atomic_add_x2") == 1, name
