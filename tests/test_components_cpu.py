"""Connected components (gs_fields_components / gs_members_components) without a GPU: the union-find restatement of the
rule (tests/components_ref.py) against hand-counted planes and against scipy.ndimage.label, components - Euler number ==
holes, the exports, every refusal that needs no device, the Components object's derived values, and the stand-alone C++
program that checks the seam merge and replays the kernels' phases on the host (plain and under sanitizers)."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import components_ref as ref
from tests import morph_ref
from tests.children import ROOT, build_program, run_program


def triple(a, t=0.5, above=True, connectivity=8):
    r = ref.result(np.asarray(a, np.float32), t, above, connectivity)
    return r["components"], r["set_cells"], r["largest"]


def test_hand_counted_planes():
    for conn in (4, 8):
        assert triple([[1.0]], connectivity=conn) == (1, 1, 1) and triple([[0.0]], connectivity=conn) == (0, 0, 0)
        assert triple([[1, 0, 1, 1, 0, 1]], connectivity=conn) == (3, 4, 2)                  # one row
        assert triple([[1], [1], [0], [1]], connectivity=conn) == (2, 3, 2)                  # one column
        ring = np.zeros((7, 9), np.float32)
        ring[1:6, 2:7] = 1
        ring[2:5, 3:6] = 0
        assert triple(ring, connectivity=conn) == (1, 16, 16)
        assert not ref.counters(np.zeros((0, 5), np.float32), 0.5, True, conn).any()
    board = ref.checkerboard((5, 6))
    assert triple(board, connectivity=4) == (15, 15, 1) and triple(board, connectivity=8) == (1, 15, 15)
    assert int(ref.result(board, 0.5, True, 4)["by_size"][0]) == 15
    corner = [[1, 0], [0, 1]]                                                                # two cells touching at a corner
    assert triple(corner, connectivity=4) == (2, 2, 1) and triple(corner, connectivity=8) == (1, 2, 2)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    special = np.array([[nan, 1.0, 0.5], [0.5, nan, 1.0], [inf, -inf, 0.5]], np.float32)     # NaN, +-inf, cells equal to 0.5
    assert triple(special, 0.5, True, 4) == (3, 3, 1) and triple(special, 0.5, True, 8) == (2, 3, 2)
    assert triple(special, 0.5, False, 8) == (1, 1, 1) and triple(special, inf, True, 8) == (0, 0, 0)
    assert triple(special, inf, False, 4) == (2, 6, 5)                                       # all but NaN and +inf: a C and a cell
    by = ref.result(np.ones((3, 4), np.float32), 0.5)["by_size"]
    assert by.dtype == np.uint64 and by.shape == (32,) and int(by[3]) == 1 and int(by.sum()) == 1   # 8 <= 12 < 16


@pytest.mark.parametrize("seed", range(8))
def test_reference_against_scipy_label(seed):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(seed)
    shape = [(1, 1), (3, 3), (9, 14), (16, 16), (30, 7), (25, 40), (40, 40), (5, 60)][seed]
    structure = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}
    for density in (0.2, 0.5, 0.593, 0.8):
        a = (rng.random(shape) < density).astype(np.float32)
        b = np.pad(a > 0.5, 2)                                  # (room for the background to be one component)
        m = morph_ref.measures(morph_ref.quads(a, 0.5))
        for conn in (4, 8):
            labels, n = ndimage.label(a > 0.5, structure[conn])
            sizes = np.bincount(labels.ravel())[1:]
            r = ref.result(a, 0.5, True, conn)
            assert r["components"] == n and r["set_cells"] == int(sizes.sum()) == m["area"]
            assert r["largest"] == (int(sizes.max()) if n else 0)
            assert np.array_equal(np.bincount(sizes), np.bincount(ref.sizes(a, 0.5, True, conn)))
            want = np.zeros(32, np.uint64)
            for s in sizes:
                want[int(s).bit_length() - 1] += np.uint64(1)
            assert np.array_equal(r["by_size"], want)
            # holes of an 8-connected foreground are the 4-connected background components but the outer one, and vice versa
            holes = ndimage.label(~b, structure[4 if conn == 8 else 8])[1] - 1
            assert r["components"] - m["euler8" if conn == 8 else "euler4"] == holes


def test_components_object():
    from grayscott_amd import Components, Morphology

    ring = np.zeros((7, 9), np.float32)
    ring[1:6, 2:7] = 1
    ring[2:5, 3:6] = 0
    ring[0, 0] = 1                                                # a ring with one hole and a lone cell
    for conn in (4, 8):
        c = Components.from_counters(ref.counters(ring, 0.5, True, conn), 0.5, True, conn)
        assert (c.count, c.set_cells, c.largest, c.connectivity, c.threshold, c.above) == (2, 17, 16, conn, 0.5, True)
        assert c.by_size.dtype == np.uint64 and c.by_size.shape == (32,) and int(c.by_size[0]) == 1 and int(c.by_size[4]) == 1
        assert c.mean_size == 17 / 2 and c.largest_fraction == 16 / 17
        m = Morphology.from_quads(morph_ref.quads(ring, 0.5), 0.5, True, ring.size)
        assert c.holes(m) == 1
        for wrong in (Morphology.from_quads(morph_ref.quads(ring, 0.25), 0.25, True, ring.size),
                      Morphology.from_quads(morph_ref.quads(ring, 0.5, False), 0.5, False, ring.size)):
            with pytest.raises(ValueError):
                c.holes(wrong)
    board = ref.checkerboard((2, 2))
    m = Morphology.from_quads(morph_ref.quads(board, 0.5), 0.5, True, 4)
    assert Components.from_counters(ref.counters(board, 0.5, True, 4), 0.5, True, 4).holes(m) == 0
    assert Components.from_counters(ref.counters(board, 0.5, True, 8), 0.5, True, 8).holes(m) == 0
    none = Components.from_counters([0] * 35, 0.1, False, 8)
    assert math.isnan(none.mean_size) and math.isnan(none.largest_fraction) and none.count == 0


def test_components_entry_points_are_exported(built):
    from grayscott_amd import capi

    lib = capi.load()
    for name in ("gs_fields_components", "gs_members_components"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    assert "int32_t gs_fields_components(" in header and "int32_t gs_members_components(" in header
    assert "typedef struct gs_components" in header and "GS_COMPONENTS_BATCH_BYTES" in header
    assert ctypes.sizeof(capi.GsComponents) == 280 and capi.GsComponents.by_size.offset == 24
    assert lib.gs_abi_version() == 4
    kernels = open(os.path.join(ROOT, "grayscott_amd", "csrc", "gs_kernels.h")).read()
    assert f"kCompTileRows = {ref.TILE_ROWS}, kCompTileCols = {ref.TILE_COLS};" in kernels   # the restated tile shape


def _f32(*values):
    return (ctypes.c_float * len(values))(*values)


def test_components_refusals_need_no_device(built):
    """Argument checks come before any device work, in the header's order: a null argument, nt, a NaN threshold, the
    connectivity -- with a context pointer that is never looked at and null plane / ensemble handles -- and only then the
    handles."""
    from grayscott_amd import capi

    lib = capi.load()
    INV = capi.GS_ERR_INVALID
    out = (capi.GsComponents * 16)()
    fields = (ctypes.c_void_p * 4)(None, None, None, None)
    dummy = ctypes.create_string_buffer(4096)                      # stands for a context; no check reads it
    ctx = ctypes.cast(dummy, ctypes.c_void_p)
    thr, sense = _f32(*([0.5] * 16)), (ctypes.c_int32 * 4)(1, 0, 1, 0)
    err = lambda: lib.gs_last_error().decode()  # noqa: E731
    nan = math.nan

    assert lib.gs_fields_components(None, fields, 1, thr, sense, 1, 8, out) == INV and "null" in err()
    assert lib.gs_fields_components(ctx, None, 1, thr, sense, 1, 8, out) == INV and "null" in err()
    assert lib.gs_fields_components(ctx, fields, 1, None, sense, 1, 8, out) == INV and "null" in err()
    assert lib.gs_fields_components(ctx, fields, 1, thr, None, 1, 8, out) == INV and "null" in err()
    assert lib.gs_fields_components(ctx, fields, 1, thr, sense, 1, 8, None) == INV and "null" in err()
    assert lib.gs_fields_components(ctx, fields, 1, thr, sense, 9, 5, None) == INV and "null" in err()        # null comes first
    assert lib.gs_members_components(None, None, 0, 1, thr, sense, 1, 8, out) == INV and "null" in err()
    assert lib.gs_members_components(ctx, None, 0, 1, None, sense, 1, 8, out) == INV and "null" in err()
    assert lib.gs_members_components(ctx, None, 0, 1, thr, None, 1, 8, out) == INV and "null" in err()
    assert lib.gs_members_components(ctx, None, 0, 1, thr, sense, 1, 8, None) == INV and "null" in err()
    for nt in (0, -2, 5, 1 << 20):                                  # nt before a NaN threshold and the connectivity
        assert lib.gs_fields_components(ctx, fields, 1, _f32(nan), sense, nt, 5, out) == INV and "thresholds (1..4)" in err(), nt
        assert lib.gs_fields_components(ctx, fields, 7, thr, sense, nt, 8, out) == INV and "thresholds (1..4)" in err(), nt
        assert lib.gs_members_components(ctx, None, 0, 1, thr, sense, nt, 5, out) == INV and "thresholds (1..4)" in err(), nt
    # a NaN threshold before the connectivity
    assert lib.gs_fields_components(ctx, fields, 1, _f32(nan), sense, 1, 5, out) == INV and "NaN" in err()
    assert lib.gs_fields_components(ctx, fields, 2, _f32(0.1, 0.2, 0.3, nan), sense, 2, 8, out) == INV and "threshold 1 of plane 1" in err()
    assert lib.gs_members_components(ctx, None, 0, 1, _f32(0.1, nan), sense, 1, 3, out) == INV and "threshold 0 of plane 1" in err()
    for conn in (0, 1, 5, 6, 16, -8):                               # the connectivity before any handle
        assert lib.gs_fields_components(ctx, fields, 1, thr, sense, 1, conn, out) == INV and "connectivity" in err(), conn
        assert lib.gs_members_components(ctx, None, 0, 1, thr, sense, 2, conn, out) == INV and "connectivity" in err(), conn
    for conn in (4, 8):                                             # then the handles, as morphology checks them
        assert lib.gs_fields_components(ctx, fields, 1, thr, sense, 1, conn, out) == INV and "field 0" in err()
        assert lib.gs_fields_components(ctx, fields, 4, thr, sense, 4, conn, out) == INV and "field 0" in err()
        assert lib.gs_members_components(ctx, None, 0, 1, thr, sense, 1, conn, out) == INV and "null" in err()
        for n in (0, -1, 5):
            assert lib.gs_fields_components(ctx, fields, n, thr, sense, 2, conn, out) == INV and "fields (1..4)" in err(), n
    # infinities are thresholds like any other: the refusal is the handle's
    assert lib.gs_fields_components(ctx, fields, 2, _f32(math.inf, -math.inf), sense, 1, 8, out) == INV and "field 0" in err()


def test_sweep_components_flags():
    from grayscott_amd import sweep

    base = ["--feed", "0.01:0.02:2", "--kill", "0.05:0.05:1", "-s", "10", "-o", "out/run.h5"]
    a = sweep.parse(base)
    assert a.components_every == 0 and a.comp_threshold_v is None and a.comp_threshold_u is None and a.comp_connectivity == 8
    b = sweep.parse(base + ["--components-every", "4", "--comp-threshold-v", "0.25,0.1,0.05", "--summary-every", "5"])
    assert b.components_every == 4 and b.comp_threshold_v == [0.25, 0.1, 0.05] and b.comp_threshold_u == [0.5] * 3
    c = sweep.parse(base + ["--components-every", "4", "--comp-threshold-v", "0.25", "--comp-threshold-u=-0.5",
                            "--comp-connectivity", "4", "--no-fields"])
    assert c.comp_threshold_v == [0.25] and c.comp_threshold_u == [-0.5] and c.comp_connectivity == 4
    assert sweep.components_path("out/run.h5") == os.path.join("out", "run.components.npz")
    for wrong in (["--components-every", "-1"], ["--components-every", "2"],
                  ["--components-every", "2", "--comp-threshold-v", "0.1,0.2,0.3,0.4,0.5"],
                  ["--components-every", "2", "--comp-threshold-v", "0.1", "--comp-threshold-u", "1,2,3,4,5"],
                  ["--components-every", "2", "--comp-threshold-v", "0.1,0.2", "--comp-threshold-u", "0.5"],
                  ["--components-every", "2", "--comp-threshold-v", "nan"], ["--components-every", "2", "--comp-threshold-v", "a,b"],
                  ["--components-every", "2", "--comp-threshold-v", "0.1", "--comp-connectivity", "6"]):
        with pytest.raises(SystemExit):
            sweep.parse(base + wrong)


@pytest.mark.parametrize("sanitize", [False, True])
def test_seam_merge_and_kernel_phases_on_the_host(tmp_path, sanitize):
    """tests/cpp/components_merge.cpp: planes cut into 1..5 slabs (one-row slabs included) through the merge function, and
    the tile, border and flatten phases replayed through the shared find / unite -- a stand-alone program, also built with
    the address and undefined-behaviour sanitizers."""
    exe = build_program("components_merge", tmp_path, library=False, sanitize=sanitize)
    r = run_program([str(exe)])
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_cpp_components_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("components_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_components.py)
        r = run_program([str(exe), "3", "8", "16", "5", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
