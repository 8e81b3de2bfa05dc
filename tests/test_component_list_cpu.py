"""Component lists (gs_field_component_list / gs_members_component_list) without a GPU: the scipy restatement of the rule
(tests/component_list_ref.py) against a literal flood fill and against the counters of tests/components_ref.py, the exports,
the record's layout, every refusal that needs no device, the ComponentList object's derived values, the sweep's flags, and the
stand-alone C++ program that checks the seam merge (plain and under sanitizers)."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import component_list_ref as ref
from tests import components_ref
from tests import morph_ref
from tests.children import ROOT, build_program, run_program


def test_hand_counted_planes():
    ring = np.zeros((7, 9), np.float32)
    ring[1:6, 2:7] = 1
    ring[2:5, 3:6] = 0
    ring[0, 0] = 1                                                # a lone cell, then a ring with one hole
    for conn in (4, 8):
        got = ref.records(ring, 0.5, True, conn)
        want = np.array([(1, 0, 0, 0, 0, 0, 0, 0, 0), (16, 16 * 3, 16 * 4, 1, 2, 1, 5, 2, 6)], ref.DTYPE)
        assert np.array_equal(got, want)
        assert np.array_equal(ref.records(ring, 0.5, True, conn, 2), want[1:]) and ref.records(ring, 0.5, True, conn, 17).shape == (0,)
    corner = np.array([[0, 1], [1, 0]], np.float32)              # two cells touching at a corner
    assert np.array_equal(ref.records(corner, 0.5, True, 4), np.array([(1, 0, 1, 0, 1, 0, 0, 1, 1), (1, 1, 0, 1, 0, 1, 1, 0, 0)], ref.DTYPE))
    assert np.array_equal(ref.records(corner, 0.5, True, 8), np.array([(2, 1, 1, 0, 1, 0, 1, 0, 1)], ref.DTYPE))
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    special = np.array([[nan, 1.0, 0.5], [0.5, nan, 1.0], [inf, -inf, 0.5]], np.float32)     # NaN, +-inf, cells equal to 0.5
    assert [int(x) for x in ref.records(special, 0.5, True, 4)["size"]] == [1, 1, 1]
    assert [int(x) for x in ref.records(special, 0.5, True, 8)["size"]] == [2, 1]
    assert ref.records(special, inf, True, 8).shape == (0,) and ref.records(np.zeros((0, 5), np.float32), 0.5).shape == (0,)
    # a component whose first cell is not in its box's first column
    hook = np.array([[0, 0, 1], [1, 1, 1]], np.float32)
    assert np.array_equal(ref.records(hook, 0.5), np.array([(4, 3, 5, 0, 2, 0, 1, 0, 2)], ref.DTYPE))


@pytest.mark.parametrize("seed", range(8))
def test_reference_against_the_literal_loop_and_the_counters(seed):
    rng = np.random.default_rng(seed)
    shape = [(1, 1), (3, 3), (9, 14), (16, 16), (30, 7), (25, 40), (40, 40), (5, 60)][seed]
    for density in (0.2, 0.5, 0.593, 0.8):
        a = (rng.random(shape) < density).astype(np.float32)
        for conn in (4, 8):
            full = ref.records(a, 0.5, True, conn)
            assert full.dtype == ref.DTYPE and full.dtype.itemsize == 48
            for min_size in (1, 2, 7):
                got = ref.records(a, 0.5, True, conn, min_size)
                assert np.array_equal(got, ref.literal(a, 0.5, True, conn, min_size))
                assert np.array_equal(got, full[full["size"] >= min_size])
            # the four identities with the components' counters: number, sum, maximum and bins of the sizes
            assert np.array_equal(ref.counters(full), components_ref.counters(a, 0.5, True, conn))
            first = full["first_row"].astype(np.int64) * shape[1] + full["first_col"]
            assert np.all(np.diff(first) > 0)
            assert np.all(full["row_min"] == full["first_row"]) and np.all(full["col_min"] <= full["first_col"])
    for name in ("serpentine", "comb", "rings", "checkerboard", "staircase"):
        a = getattr(components_ref, name)((9, 14))
        for conn in (4, 8):
            assert np.array_equal(ref.records(a, 0.5, True, conn), ref.literal(a, 0.5, True, conn)), name
            assert np.array_equal(ref.counters(ref.records(a, 0.5, True, conn)), components_ref.counters(a, 0.5, True, conn)), name
    p = morph_ref.planted((17, 40), 2.0 ** -130, 3, 0.5, False)   # NaN, infinities, sub-normals, cells equal to t
    for conn in (4, 8):
        assert np.array_equal(ref.records(p, 2.0 ** -130, False, conn), ref.literal(p, 2.0 ** -130, False, conn))
    assert np.array_equal(ref.shifted(ref.records(a, 0.5), 5), ref.records(np.vstack([np.zeros((5, 14), np.float32), a]), 0.5))


def test_component_list_object():
    from grayscott_amd import ComponentList
    from grayscott_amd.simulation import COMPONENT_RECORD_DTYPE

    assert COMPONENT_RECORD_DTYPE == ref.DTYPE
    a = np.zeros((6, 8), np.float32)
    a[0, 0] = a[2, 3] = a[2, 4] = a[3, 3] = a[5, 6] = a[5, 7] = 1
    c = ComponentList(ref.records(a, 0.5), 6, 8, 0.5, True, 8, 1)
    assert c.count == 3 and [int(x) for x in c.sizes] == [1, 3, 2]
    assert np.array_equal(c.centroids(), [[0, 0], [7 / 3, 10 / 3], [5, 6.5]]) and c.centroids().dtype == np.float64
    assert np.array_equal(c.boxes(), [[0, 0, 0, 0], [2, 3, 3, 4], [5, 5, 6, 7]])
    assert np.array_equal(c.first_cells(), [[0, 0], [2, 3], [5, 6]])
    assert list(c.touches_edge()) == [True, False, True]
    none = ComponentList(np.zeros(0, ref.DTYPE), 6, 8, 0.5, True, 8, 1)
    assert none.count == 0 and none.centroids().shape == (0, 2) and none.boxes().shape == (0, 4) and none.touches_edge().shape == (0,)


def test_component_list_entry_points_are_exported(built):
    from grayscott_amd import capi
    import grayscott_amd

    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    for name in ("gs_field_component_list", "gs_members_component_list", "gs_component_list_view", "gs_component_list_destroy"):
        assert name in capi.EXPORTS and hasattr(lib, name) and f"int32_t {name}(" in header
    assert "typedef struct gs_component_record" in header and "typedef struct gs_component_list gs_component_list;" in header
    assert "centroids or bounding boxes" not in header and "label planes for the caller" in header
    assert "ComponentList" in grayscott_amd.__all__
    assert lib.gs_abi_version() == 4
    R = capi.GsComponentRecord
    assert ctypes.sizeof(R) == 48 == ref.DTYPE.itemsize
    offsets = {"size": 0, "sum_row": 8, "sum_col": 16, "first_row": 24, "first_col": 28, "row_min": 32, "row_max": 36,
               "col_min": 40, "col_max": 44}
    for name, at in offsets.items():
        assert getattr(R, name).offset == at == ref.DTYPE.fields[name][1], name


def test_component_list_refusals_need_no_device(built):
    """Argument checks come before any device work, in the header's order: a null argument, a NaN threshold, the connectivity,
    min_size, the species -- with a context pointer that is never looked at and null handles -- and only then the handles."""
    from grayscott_amd import capi

    lib = capi.load()
    INV = capi.GS_ERR_INVALID
    dummy = ctypes.create_string_buffer(4096)                      # stands for a context; no check reads it
    ctx = ctypes.cast(dummy, ctypes.c_void_p)
    out = ctypes.c_void_p()
    ref_out = ctypes.byref(out)
    err = lambda: lib.gs_last_error().decode()  # noqa: E731
    nan = math.nan
    field, members = lib.gs_field_component_list, lib.gs_members_component_list

    assert field(None, None, 0.5, 1, 8, 1, ref_out) == INV and "null" in err()
    assert field(ctx, None, 0.5, 1, 8, 1, None) == INV and "null argument" in err()
    assert field(ctx, None, nan, 1, 5, 0, None) == INV and "null argument" in err()                  # null comes first
    assert members(None, None, 0, 1, 1, 0.5, 1, 8, 1, ref_out) == INV and "null" in err()
    assert members(ctx, None, 0, 1, 7, nan, 1, 5, 0, None) == INV and "null argument" in err()
    assert field(ctx, None, nan, 1, 5, 0, ref_out) == INV and "NaN" in err()                           # NaN before the rest
    assert members(ctx, None, 0, 1, 7, nan, 1, 5, 0, ref_out) == INV and "NaN" in err()
    for conn in (0, 1, 5, 6, 16, -8):                                                                  # then the connectivity
        assert field(ctx, None, 0.5, 1, conn, 0, ref_out) == INV and "connectivity" in err(), conn
        assert members(ctx, None, 0, 1, 7, 0.5, 1, conn, 0, ref_out) == INV and "connectivity" in err(), conn
    for conn in (4, 8):
        assert field(ctx, None, 0.5, 1, conn, 0, ref_out) == INV and "min_size" in err()               # then min_size
        assert members(ctx, None, 0, 1, 7, 0.5, 0, conn, 0, ref_out) == INV and "min_size" in err()
        for species in (-1, 2, 7):                                                                     # then the species
            assert members(ctx, None, 0, 1, species, 0.5, 1, conn, 1, ref_out) == INV and "species" in err(), species
        assert field(ctx, None, 0.5, 1, conn, 1, ref_out) == INV and "field: null" in err()            # and only then the handles
        assert field(ctx, None, math.inf, 0, conn, 1 << 40, ref_out) == INV and "field: null" in err()
        for species in (0, 1):
            assert members(ctx, None, 0, 1, species, -math.inf, 1, conn, 1, ref_out) == INV and "null argument" in err()
    assert not out                                                 # no refusal returns a list
    assert lib.gs_component_list_destroy(None) == capi.GS_OK
    planes, offsets, records = ctypes.c_uint64(0), ctypes.POINTER(ctypes.c_uint64)(), ctypes.POINTER(capi.GsComponentRecord)()
    assert lib.gs_component_list_view(None, ctypes.byref(planes), ctypes.byref(offsets), ctypes.byref(records)) == INV


def test_sweep_spots_flags():
    from grayscott_amd import sweep

    base = ["--feed", "0.01:0.02:2", "--kill", "0.05:0.05:1", "-s", "10", "-o", "out/run.h5"]
    a = sweep.parse(base)
    assert a.spots_every == 0 and a.spot_threshold_v is None and a.spot_min_size == 1 and a.spot_connectivity == 8
    b = sweep.parse(base + ["--spots-every", "4", "--spot-threshold-v", "0.25", "--summary-every", "5"])
    assert b.spots_every == 4 and b.spot_threshold_v == 0.25
    c = sweep.parse(base + ["--spots-every", "4", "--spot-threshold-v=-0.5", "--spot-min-size", "9", "--spot-connectivity", "4",
                            "--no-fields"])
    assert c.spot_threshold_v == -0.5 and c.spot_min_size == 9 and c.spot_connectivity == 4
    assert sweep.spots_path("out/run.h5") == os.path.join("out", "run.spots.npz")
    for wrong in (["--spots-every", "-1"], ["--spots-every", "2"], ["--spots-every", "2", "--spot-threshold-v", "nan"],
                  ["--spots-every", "2", "--spot-threshold-v", "a"],
                  ["--spots-every", "2", "--spot-threshold-v", "0.1", "--spot-min-size", "0"],
                  ["--spots-every", "2", "--spot-threshold-v", "0.1", "--spot-connectivity", "6"]):
        with pytest.raises(SystemExit):
            sweep.parse(base + wrong)


def test_write_spots(tmp_path):
    from grayscott_amd import ComponentList, sweep

    a = np.zeros((4, 5), np.float32)
    a[1, 1] = a[3, 4] = 1
    lists = [[ComponentList(ref.records(a, 0.5), 4, 5, 0.5, True, 8, 1), ComponentList(np.zeros(0, ref.DTYPE), 4, 5, 0.5, True, 8, 1)],
             [ComponentList(ref.records(a.T.copy(), 0.5)[:1], 5, 4, 0.5, True, 8, 1), ComponentList(ref.records(a, 0.5), 4, 5, 0.5, True, 8, 1)]]
    sweep.write_spots(str(tmp_path / "s.npz"), [3, 6], lists, 0.5, 8, 1)
    z = np.load(tmp_path / "s.npz")
    assert list(z["steps"]) == [3, 6] and list(z["offsets"]) == [0, 2, 2, 3, 5] and z["records"].dtype == ref.DTYPE
    assert np.array_equal(z["records"][3:5], ref.records(a, 0.5)) and int(z["min_size"]) == 1 and int(z["connectivity"]) == 8


@pytest.mark.parametrize("sanitize", [False, True])
def test_list_seam_merge_on_the_host(tmp_path, sanitize):
    """tests/cpp/component_list_merge.cpp: planes cut into 1..5 slabs (one-row slabs included), each labelled on the host with
    the shared find / unite, through the merge function against the whole plane's list -- a stand-alone program, also built
    with the address and undefined-behaviour sanitizers."""
    exe = build_program("component_list_merge", tmp_path, library=False, sanitize=sanitize)
    r = run_program([str(exe)])
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_cpp_component_list_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("component_list_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_component_list.py)
        r = run_program([str(exe), "3", "8", "16", "5", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
