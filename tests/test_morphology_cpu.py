"""Morphology (gs_fields_morphology / gs_members_morphology) without a GPU: the numpy restatement of the bit-quad rule
(tests/morph_ref.py) against the literal per-quad definition and against direct counts of cells, sides and components, the
exports, every refusal that needs no device, the Morphology object's derived quantities, the sweep's flags and the C++
mirror's build."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import morph_ref
from tests.children import ROOT, build_program, run_program


def checkerboard(shape):
    r, c = np.indices(shape)
    return ((r + c) % 2).astype(np.float32)


def small_planes():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    out = [np.array([[1.0]], np.float32), np.array([[0.0]], np.float32),                       # 1 x 1, set and unset
           np.array([[1, 0, 1, 1, 0, 1]], np.float32), np.array([[1], [1], [0], [1]], np.float32),   # one row, one column
           checkerboard((5, 6)), checkerboard((1, 2)), np.ones((3, 4), np.float32), np.zeros((2, 2), np.float32),
           np.array([[nan, 1.0, 0.5], [0.5, nan, 1.0], [inf, -inf, 0.5]], np.float32)]         # NaN, cells equal to 0.5
    for seed, shape in enumerate([(7, 13), (2, 9), (9, 2), (12, 12)]):
        out.append(morph_ref.planted(shape, 0.5, seed, 0.5))
    return out


@pytest.mark.parametrize("above", [True, False])
def test_restatement_matches_the_literal_definition(above):
    for a in small_planes():
        for t in (0.5, 0.0, -1.0, float("inf")):
            got, want = morph_ref.quads(a, t, above), morph_ref.literal(a, t, above)
            assert got.dtype == np.uint64 and got.shape == (6,)
            assert np.array_equal(got, want), (a, t, got, want)
            assert int(got.sum()) == (a.shape[0] + 1) * (a.shape[1] + 1)
    assert list(morph_ref.quads(np.zeros((0, 5), np.float32), 0.5)) == [0] * 6
    assert list(morph_ref.literal(np.zeros((3, 0), np.float32), 0.5)) == [0] * 6


def test_rule_consequences():
    nan = np.float32(np.nan)
    one = lambda x, t, above: int(morph_ref.quads(np.array([[x]], np.float32), t, above)[1]) == 4  # noqa: E731  (a set cell: 4 x Q1)
    assert one(0.6, 0.5, True) and not one(0.5, 0.5, True) and not one(0.5, 0.5, False) and one(0.4, 0.5, False)
    assert not one(nan, 0.5, True) and not one(nan, 0.5, False)
    assert one(np.inf, 3e38, True) and one(-np.inf, -3e38, False) and not one(np.inf, np.inf, True)
    assert one(1e-45, 0.0, True) and one(-1e-45, 0.0, False) and not one(-0.0, 0.0, False) and not one(0.0, -0.0, True)
    assert list(morph_ref.quads(checkerboard((2, 2)), 0.5)) == [2, 6, 0, 0, 0, 1]


@pytest.mark.parametrize("seed", range(6))
def test_area_and_perimeter_are_direct_counts(seed):
    shape = [(1, 1), (1, 9), (8, 1), (6, 7), (13, 5), (20, 21)][seed]
    for density in (0.1, 0.5, 0.9):
        a = morph_ref.planted(shape, 0.3, seed, density)
        b = np.pad(morph_ref.set_cells(a, 0.3, True), 1)
        m = morph_ref.measures(morph_ref.quads(a, 0.3))
        assert m["area"] == int(b.sum())
        sides = int(np.count_nonzero(b[1:] != b[:-1])) + int(np.count_nonzero(b[:, 1:] != b[:, :-1]))
        assert m["perimeter"] == sides


@pytest.mark.parametrize("seed", range(8))
def test_euler_numbers_are_components_minus_holes(seed):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(seed)
    shape = [(1, 1), (3, 3), (9, 14), (16, 16), (30, 7), (25, 40), (40, 40), (5, 60)][seed]
    four, eight = ndimage.generate_binary_structure(2, 1), ndimage.generate_binary_structure(2, 2)
    for density in (0.2, 0.5, 0.8):
        a = (rng.random(shape) < density).astype(np.float32)
        b = np.pad(a > 0.5, 2)                                  # (room for the background to be one component)
        m = morph_ref.measures(morph_ref.quads(a, 0.5))
        # holes of an 8-connected foreground are the 4-connected background components but the outer one, and vice versa
        assert m["euler8"] == ndimage.label(b, eight)[1] - (ndimage.label(~b, four)[1] - 1)
        assert m["euler4"] == ndimage.label(b, four)[1] - (ndimage.label(~b, eight)[1] - 1)


def test_morphology_object():
    from grayscott_amd import Morphology
    from grayscott_amd.simulation import quad_measures

    ring = np.zeros((7, 9), np.float32)
    ring[1:6, 2:7] = 1
    ring[2:5, 3:6] = 0                                          # a ring with one hole
    m = Morphology.from_quads(morph_ref.quads(ring, 0.5), 0.5, True, ring.size)
    assert m.euler8 == 0 and m.euler4 == 0 and m.area == 16 and m.perimeter == 20 + 12 and m.cells == 63
    assert m.area_fraction == 16 / 63 and m.threshold == 0.5 and m.above is True and m.quads.dtype == np.uint64
    for k in (1, 5):
        spots = np.zeros((9, 4 * k), np.float32)
        spots[4, 1::4] = 1                                      # k isolated cells
        s = Morphology.from_quads(morph_ref.quads(spots, 0.5), 0.5, True, spots.size)
        assert s.euler8 == k and s.euler4 == k and s.perimeter == 4 * k and s.area == k
    d = Morphology.from_quads(morph_ref.quads(checkerboard((2, 2)), 0.5), 0.5, True, 4)
    assert (d.euler8, d.euler4, d.area, d.perimeter) == (1, 2, 2, 8)
    assert math.isnan(Morphology.from_quads([0] * 6, 0.1, False, 0).area_fraction)
    stack = np.stack([m.quads, d.quads]).reshape(2, 1, 6)
    area, perimeter, euler4, euler8 = quad_measures(stack)
    assert area.shape == (2, 1) and list(area[:, 0]) == [16, 2] and list(perimeter[:, 0]) == [32, 8]
    assert list(euler4[:, 0]) == [0, 2] and list(euler8[:, 0]) == [0, 1]


def test_morphology_entry_points_are_exported(built):
    from grayscott_amd import capi

    lib = capi.load()
    for name in ("gs_fields_morphology", "gs_members_morphology"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    assert "int32_t gs_fields_morphology(" in header and "int32_t gs_members_morphology(" in header
    assert "typedef struct gs_morphology" in header and ctypes.sizeof(capi.GsMorphology) == 48
    assert lib.gs_abi_version() == 4


def _f32(*values):
    return (ctypes.c_float * len(values))(*values)


def test_morphology_refusals_need_no_device(built):
    """Argument checks come before any device work: with a context pointer that is never looked at and null plane /
    ensemble handles, every refusal of the header returns GS_ERR_INVALID with its own message."""
    from grayscott_amd import capi

    lib = capi.load()
    INV = capi.GS_ERR_INVALID
    out = (capi.GsMorphology * 16)()
    fields = (ctypes.c_void_p * 4)(None, None, None, None)
    dummy = ctypes.create_string_buffer(4096)                      # stands for a context; no check reads it
    ctx = ctypes.cast(dummy, ctypes.c_void_p)
    thr, sense = _f32(*([0.5] * 16)), (ctypes.c_int32 * 4)(1, 0, 1, 0)
    err = lambda: lib.gs_last_error().decode()  # noqa: E731

    assert lib.gs_fields_morphology(None, fields, 1, thr, sense, 1, out) == INV and "null" in err()
    assert lib.gs_fields_morphology(ctx, None, 1, thr, sense, 1, out) == INV and "null" in err()
    assert lib.gs_fields_morphology(ctx, fields, 1, None, sense, 1, out) == INV and "null" in err()
    assert lib.gs_fields_morphology(ctx, fields, 1, thr, None, 1, out) == INV and "null" in err()
    assert lib.gs_fields_morphology(ctx, fields, 1, thr, sense, 1, None) == INV and "null" in err()
    assert lib.gs_fields_morphology(ctx, fields, 1, thr, sense, 1, out) == INV and "field 0" in err()
    assert lib.gs_members_morphology(None, None, 0, 1, thr, sense, 1, out) == INV and "null" in err()
    assert lib.gs_members_morphology(ctx, None, 0, 1, thr, sense, 1, out) == INV and "null" in err()
    assert lib.gs_members_morphology(ctx, None, 0, 1, None, sense, 1, out) == INV and "null" in err()
    assert lib.gs_members_morphology(ctx, None, 0, 1, thr, None, 1, out) == INV and "null" in err()
    for n in (0, -1, 5):
        assert lib.gs_fields_morphology(ctx, fields, n, thr, sense, 2, out) == INV and "fields (1..4)" in err(), n
    for nt in (0, -2, 5, 1 << 20):
        assert lib.gs_fields_morphology(ctx, fields, 1, thr, sense, nt, out) == INV and "thresholds (1..4)" in err(), nt
        assert lib.gs_fields_morphology(ctx, fields, 7, thr, sense, nt, out) == INV and "thresholds (1..4)" in err(), nt
        assert lib.gs_members_morphology(ctx, None, 0, 1, thr, sense, nt, out) == INV and "thresholds (1..4)" in err(), nt
    for nt in (1, 4):
        assert lib.gs_fields_morphology(ctx, fields, 4, thr, sense, nt, out) == INV and "field 0" in err(), nt
    nan = math.nan
    assert lib.gs_fields_morphology(ctx, fields, 1, _f32(nan), sense, 1, out) == INV and "NaN" in err()
    assert lib.gs_fields_morphology(ctx, fields, 2, _f32(0.1, 0.2, 0.3, nan), sense, 2, out) == INV and "NaN" in err()
    assert "threshold 1 of plane 1" in err()
    assert lib.gs_members_morphology(ctx, None, 0, 1, _f32(0.1, nan), sense, 1, out) == INV and "threshold 0 of plane 1" in err()
    assert lib.gs_members_morphology(ctx, None, 0, 1, _f32(nan, 0.1, 0.2, 0.3), sense, 2, out) == INV and "NaN" in err()
    # infinities are thresholds like any other: the refusal is the handle's
    assert lib.gs_fields_morphology(ctx, fields, 2, _f32(math.inf, -math.inf), sense, 1, out) == INV and "field 0" in err()


def test_sweep_morphology_flags():
    from grayscott_amd import sweep

    base = ["--feed", "0.01:0.02:2", "--kill", "0.05:0.05:1", "-s", "10", "-o", "out/run.h5"]
    a = sweep.parse(base)
    assert a.morphology_every == 0 and a.morph_threshold_v is None and a.morph_threshold_u is None
    b = sweep.parse(base + ["--morphology-every", "4", "--morph-threshold-v", "0.25,0.1,0.05", "--summary-every", "5"])
    assert b.morphology_every == 4 and b.morph_threshold_v == [0.25, 0.1, 0.05] and b.morph_threshold_u == [0.5] * 3
    c = sweep.parse(base + ["--morphology-every", "4", "--morph-threshold-v", "0.25", "--morph-threshold-u=-0.5"])
    assert c.morph_threshold_v == [0.25] and c.morph_threshold_u == [-0.5]
    assert sweep.morphology_path("out/run.h5") == os.path.join("out", "run.morphology.npz")
    for wrong in (["--morphology-every", "-1"], ["--morphology-every", "2"],
                  ["--morphology-every", "2", "--morph-threshold-v", "0.1,0.2,0.3,0.4,0.5"],
                  ["--morphology-every", "2", "--morph-threshold-v", "0.1", "--morph-threshold-u", "1,2,3,4,5"],
                  ["--morphology-every", "2", "--morph-threshold-v", "0.1,0.2", "--morph-threshold-u", "0.5"],
                  ["--morphology-every", "2", "--morph-threshold-v", "nan"], ["--morphology-every", "2", "--morph-threshold-v", "a,b"]):
        with pytest.raises(SystemExit):
            sweep.parse(base + wrong)


def test_cpp_morphology_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("morphology_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_morphology.py)
        r = run_program([str(exe), "3", "8", "16", "5", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
