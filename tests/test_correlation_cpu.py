"""Correlations (gs_fields_correlation / gs_members_correlation) without a GPU: the numpy restatement of the pair-count rule
(tests/corr_ref.py) against the literal per-pair definition, the geometry, morphology's area at lag 0, the Correlation
object on planted stripes, the prototypes in header, capi.py and C++ mirror, every refusal that needs no device, the sweep's
flags, the kernel's resources and the C++ mirror's build."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

from tests import corr_ref, morph_ref
from tests.children import ROOT, build_program, run_program

HEADER = os.path.join(ROOT, "include", "gs_hip.h")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402


def small_planes():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    out = [np.array([[1.0]], np.float32), np.array([[0.0]], np.float32),
           np.array([[1, 0, 1, 1, 0, 1]], np.float32), np.array([[1], [1], [0], [1]], np.float32),
           np.ones((3, 4), np.float32), np.zeros((2, 2), np.float32),
           np.array([[nan, 1.0, 0.5], [0.5, nan, 1.0], [inf, -inf, 0.5]], np.float32)]
    for seed, shape in enumerate([(7, 13), (2, 9), (9, 2), (12, 12)]):
        out.append(morph_ref.planted(shape, 0.5, seed, 0.5))
    return out


@pytest.mark.parametrize("above", [True, False])
def test_restatement_matches_the_literal_definition(above):
    for a in small_planes():
        for t in (0.5, 0.0, float("inf")):
            for lag in (1, 5, 14):                      # 14 exceeds every plane here: those lags count 0
                got, want = corr_ref.pairs(a, t, above, lag), corr_ref.literal(a, t, above, lag)
                assert got.dtype == np.uint64 and got.shape == (4, lag + 1)
                assert np.array_equal(got, want), (a, t, lag, got, want)
                assert len(set(int(x) for x in got[:, 0])) == 1
    assert not corr_ref.pairs(np.zeros((0, 5), np.float32), 0.5, True, 3).any()
    assert not corr_ref.pairs(np.zeros((3, 0), np.float32), 0.5, True, 3).any()


def test_all_set_planes_give_the_pair_totals():
    from grayscott_amd.simulation import pairs_total

    for shape in ((1, 1), (1, 9), (8, 1), (6, 7), (13, 5), (70, 3)):
        for lag in (1, 7, 64):
            got = corr_ref.pairs(np.ones(shape, np.float32), 0.5, True, lag).astype(np.int64)
            want = corr_ref.totals(shape[0], shape[1], lag)
            assert np.array_equal(got, want), (shape, lag)
            assert np.array_equal(pairs_total(shape[0], shape[1], lag), want)
            assert want[1, min(lag, shape[0])] == 0 or lag < shape[0]


@pytest.mark.parametrize("seed", range(4))
def test_lag_0_is_morphologys_area(seed):
    shape = [(1, 9), (6, 7), (13, 5), (20, 21)][seed]
    for above in (True, False):
        for t in (0.3, 0.0, -1.0):
            a = morph_ref.planted(shape, t, seed, 0.4, above)
            area = morph_ref.measures(morph_ref.quads(a, t, above))["area"]
            assert [int(x) for x in corr_ref.pairs(a, t, above, 3)[:, 0]] == [area] * 4


@pytest.mark.parametrize("across", range(4))
@pytest.mark.parametrize("period", [8, 12])
def test_correlation_object_on_planted_stripes(across, period):
    """Stripes of period p whose value changes along e_across.  Along e_across the autocovariance has its first minimum at
    p / 2 and the maximum after it at p.  The direction ALONG the stripes -- rows for column stripes and the other way round,
    one diagonal for the other -- has a flat autocovariance: every pair along it is alike."""
    from grayscott_amd import Correlation

    shape = (96, 120)
    plane = corr_ref.stripes(shape, period, across)
    lag = 2 * period + 2
    c = Correlation.from_pairs(corr_ref.pairs(plane, 0.5, True, lag), 0.5, True, *shape)
    assert c.max_lag == lag and list(c.lags) == list(range(lag + 1)) and c.pairs.dtype == np.uint64
    assert abs(c.fraction - 0.5) < 0.03
    assert np.array_equal(c.pairs_total(across), corr_ref.totals(*shape, lag)[across])
    assert np.array_equal(c.pairs_set(across), c.pairs[across])
    assert c.first_minimum(across) == period // 2
    assert c.first_maximum_after_minimum(across) == period
    z = c.first_zero_crossing(across)
    assert z is not None and period / 4 - 1 <= z <= period / 4 + 1
    along = {0: 1, 1: 0, 2: 3, 3: 2}[across]
    flat = c.autocovariance(along)
    assert np.all(np.abs(flat - flat[0]) < 0.02), flat
    assert flat.min() > 0.2                                     # (no zero crossing: ~ 1/4 everywhere, up to edge effects)
    assert c.first_zero_crossing(along) is None
    assert np.array_equal(c.distance(0), c.lags.astype(float)) and np.allclose(c.distance(3), c.lags * math.sqrt(2.0))
    s2 = c.s2(across)
    assert s2[0] == c.fraction and np.array_equal(c.autocovariance(across), s2 - c.fraction ** 2)


def test_correlation_object_edges():
    from grayscott_amd import Correlation

    c = Correlation.from_pairs(corr_ref.pairs(np.ones((3, 5), np.float32), 0.5, True, 6), 0.5, True, 3, 5)
    assert c.fraction == 1.0 and list(c.pairs_total(1)) == [15, 10, 5, 0, 0, 0, 0]
    assert np.isnan(c.s2(1)[3:]).all() and list(c.s2(1)[:3]) == [1.0, 1.0, 1.0] and np.isnan(c.s2(0)[5:]).all()
    assert c.first_minimum(0) is None and c.first_maximum_after_minimum(0) is None and c.first_zero_crossing(1) is None
    e = Correlation.from_pairs(np.zeros((4, 3), np.uint64), 0.1, False, 0, 0)
    assert math.isnan(e.fraction) and np.isnan(e.s2(2)).all() and e.above is False


def _prototype(text, name):
    m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_prototypes_and_layout_agree(built):
    from grayscott_amd import capi

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    f, m = _prototype(text, "gs_fields_correlation"), _prototype(text, "gs_members_correlation")
    assert f == ["gs_ctx *ctx", "gs_field *const *fields", "int32_t n", "const float *thresholds", "const int32_t *above",
                 "int32_t nt", "int32_t max_lag", "uint64_t *out"]
    assert m == ["gs_ctx *ctx", "gs_ensemble *e", "uint64_t first", "uint64_t count", "const float *thresholds",
                 "const int32_t above[2]", "int32_t nt", "int32_t max_lag", "uint64_t *out"]
    # the morphology entries' conventions, with the lag and plain counters in place of gs_morphology
    assert f[:6] == _prototype(text, "gs_fields_morphology")[:6] and m[:7] == _prototype(text, "gs_members_morphology")[:7]
    lib = capi.load()
    i32, u64, vp, P = ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER
    for name in ("gs_fields_correlation", "gs_members_correlation"):
        assert name in capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).restype is i32
    assert lib.gs_fields_correlation.argtypes == [vp, P(vp), i32, P(ctypes.c_float), P(i32), i32, i32, P(u64)]
    assert lib.gs_members_correlation.argtypes == [vp, vp, u64, u64, P(ctypes.c_float), P(i32), i32, i32, P(u64)]
    assert lib.gs_abi_version() == 4
    full = open(HEADER).read()
    assert "out[((i * nt + j) * 4 + k) * (L + 1) + d]" in full and "NEVER wrap" in full
    hpp = open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    assert "gs_fields_correlation(context_->get(), planes, 2, t.data(), sense, (int32_t)nt, max_lag, out.data())" in hpp
    assert "gs_members_correlation(ctx_->get(), e_, first, count, t.data(), sense, (int32_t)nt, max_lag, c.data())" in hpp
    # one layout everywhere: [plane][threshold][direction][lag]
    assert "o.pairs[k].assign(c + k * (std::size_t)(max_lag + 1)" in hpp and "out.data() + (nt + k) * 4 * lags" in hpp
    py = open(os.path.join(ROOT, "grayscott_amd", "simulation.py")).read()
    assert "np.zeros((max(n, 1), max(nt, 1), 4, lags), np.uint64)" in py
    assert "np.zeros((max(count, 0), 2, max(nt, 1), 4, lags), np.uint64)" in py


def _f32(*values):
    return (ctypes.c_float * len(values))(*values)


def test_correlation_refusals_need_no_device(built):
    """Argument checks come before any device work, in morphology's order and then the lag: with a context pointer that is
    never looked at and null plane / ensemble handles, every refusal returns GS_ERR_INVALID with its own message."""
    from grayscott_amd import capi

    lib = capi.load()
    INV = capi.GS_ERR_INVALID
    out = (ctypes.c_uint64 * (16 * 4 * 65))()
    fields = (ctypes.c_void_p * 4)(None, None, None, None)
    dummy = ctypes.create_string_buffer(4096)                      # stands for a context; no check reads it
    ctx = ctypes.cast(dummy, ctypes.c_void_p)
    thr, sense = _f32(*([0.5] * 16)), (ctypes.c_int32 * 4)(1, 0, 1, 0)
    err = lambda: lib.gs_last_error().decode()  # noqa: E731
    F, M = lib.gs_fields_correlation, lib.gs_members_correlation

    assert F(None, fields, 1, thr, sense, 1, 8, out) == INV and "null" in err()
    assert F(ctx, None, 1, thr, sense, 1, 8, out) == INV and "null" in err()
    assert F(ctx, fields, 1, None, sense, 1, 8, out) == INV and "null" in err()
    assert F(ctx, fields, 1, thr, None, 1, 8, out) == INV and "null" in err()
    assert F(ctx, fields, 1, thr, sense, 1, 8, None) == INV and "null" in err()
    assert F(ctx, fields, 1, thr, sense, 1, 8, out) == INV and "field 0" in err()
    assert M(None, None, 0, 1, thr, sense, 1, 8, out) == INV and "null" in err()
    assert M(ctx, None, 0, 1, thr, sense, 1, 8, out) == INV and "null" in err()
    assert M(ctx, None, 0, 1, None, sense, 1, 8, out) == INV and "null" in err()
    assert M(ctx, None, 0, 1, thr, None, 1, 8, out) == INV and "null" in err()
    assert M(ctx, None, 0, 1, thr, sense, 1, 8, None) == INV and "null" in err()
    for n in (0, -1, 5):
        assert F(ctx, fields, n, thr, sense, 2, 8, out) == INV and "fields (1..4)" in err(), n
    for nt in (0, -2, 5, 1 << 20):
        assert F(ctx, fields, 1, thr, sense, nt, 8, out) == INV and "thresholds (1..4)" in err(), nt
        assert F(ctx, fields, 1, thr, sense, nt, 0, out) == INV and "thresholds (1..4)" in err(), nt   # nt before the lag
        assert M(ctx, None, 0, 1, thr, sense, nt, 8, out) == INV and "thresholds (1..4)" in err(), nt
    nan = math.nan
    assert F(ctx, fields, 1, _f32(nan), sense, 1, 0, out) == INV and "NaN" in err()                    # NaN before the lag
    assert F(ctx, fields, 2, _f32(0.1, 0.2, 0.3, nan), sense, 2, 8, out) == INV and "threshold 1 of plane 1" in err()
    assert M(ctx, None, 0, 1, _f32(0.1, nan), sense, 1, 8, out) == INV and "threshold 0 of plane 1" in err()
    for lag in (0, -1, 65, 1 << 20):
        assert F(ctx, fields, 1, thr, sense, 1, lag, out) == INV and "lag" in err() and "(1..64)" in err(), lag
        assert M(ctx, None, 0, 1, thr, sense, 1, lag, out) == INV and "(1..64)" in err(), lag
    for lag in (1, 64):                                                                                # then the handles
        assert F(ctx, fields, 4, thr, sense, 4, lag, out) == INV and "field 0" in err(), lag
        assert M(ctx, None, 0, 1, thr, sense, 4, lag, out) == INV and "null" in err(), lag
    assert F(ctx, fields, 2, _f32(math.inf, -math.inf), sense, 1, 8, out) == INV and "field 0" in err()


def test_sweep_correlation_flags():
    from grayscott_amd import sweep

    base = ["--feed", "0.01:0.02:2", "--kill", "0.05:0.05:1", "-s", "10", "-o", "out/run.h5"]
    a = sweep.parse(base)
    assert a.correlation_every == 0 and a.corr_threshold_v is None and a.corr_threshold_u is None and a.corr_lags == 32
    b = sweep.parse(base + ["--correlation-every", "4", "--corr-threshold-v", "0.25,0.1,0.05", "--summary-every", "5"])
    assert b.correlation_every == 4 and b.corr_threshold_v == [0.25, 0.1, 0.05] and b.corr_threshold_u == [0.5] * 3
    c = sweep.parse(base + ["--correlation-every", "4", "--corr-threshold-v", "0.25", "--corr-threshold-u=-0.5", "--corr-lags", "64"])
    assert c.corr_threshold_v == [0.25] and c.corr_threshold_u == [-0.5] and c.corr_lags == 64
    assert sweep.correlation_path("out/run.h5") == os.path.join("out", "run.correlation.npz")
    for wrong in (["--correlation-every", "-1"], ["--correlation-every", "2"],
                  ["--correlation-every", "2", "--corr-threshold-v", "0.1,0.2,0.3,0.4,0.5"],
                  ["--correlation-every", "2", "--corr-threshold-v", "0.1,0.2", "--corr-threshold-u", "0.5"],
                  ["--correlation-every", "2", "--corr-threshold-v", "nan"],
                  ["--correlation-every", "2", "--corr-threshold-v", "0.1", "--corr-lags", "0"],
                  ["--correlation-every", "2", "--corr-threshold-v", "0.1", "--corr-lags", "65"]):
        with pytest.raises(SystemExit):
            sweep.parse(base + wrong)


def test_restated_unit_height_is_the_kernels():
    """tests/corr_ref.py's UNIT_ROWS, around which the GPU tests plant their row shapes, is the kernel's unit height."""
    src = open(os.path.join(ROOT, "grayscott_amd", "csrc", "gs_correlation.hip")).read()
    assert "kPairRows = GS_PAIR_ROWS;" in src
    assert [int(x) for x in re.findall(r"^#define GS_PAIR_ROWS (\d+)\b", src, re.M)] == [corr_ref.UNIT_ROWS]


def test_pair_kernels_resources(built):
    """Every gs_plane_pairs_k instance: no scratch, no spills, the LDS bytes DESIGN.md states ([NT][4][65] u32)."""
    found = {re.sub(r"\(.*$", "", k.name): k for k in codeobj.kernels() if "gs_plane_pairs_k" in k.name}
    assert sorted(found) == [f"gs_plane_pairs_k<{nt}>" for nt in (1, 2, 3, 4)], sorted(found)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for nt in (1, 2, 3, 4):
        k = found[f"gs_plane_pairs_k<{nt}>"]
        assert k.scratch == 0 and k.vgpr_spill == 0 and k.sgpr_spill == 0 and not k.dynamic_stack, k.name
        assert k.agpr == 0 and k.vgpr <= 168, (k.name, k.vgpr)          # three waves per SIMD at least
        assert k.lds == nt * 4 * 65 * 4, (k.name, k.lds)
        assert f"{nt * 4 * 65 * 4} B" in design, nt
        assert k.denorm_mode_32 == 3, k.name                             # sub-normal cells are compared as they are


def test_cpp_correlation_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("correlation_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_correlation.py)
        r = run_program([str(exe), "3", "8", "16", "5", "4", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
