"""Component matches without a device: the scipy restatement of their rule (tests/match_ref.py) against a literal loop and
hand-counted planes, the generator of the GPU tests' planes, the ``ComponentMatch`` object, the exports, layouts and refusals
of the C ABI, the sweep driver's flags and writer, and the host side of the seam merge as a stand-alone program."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import component_list_ref
from tests import components_ref
from tests import match_ref as ref
from tests.children import ROOT, build_program, run_program

T = components_ref.TILE_ROWS
# the shapes of tests/test_gpu_match.py's planted planes
GPU_SHAPES = [(1, 1), (2, 3), (5, 253), (3, 255), (4, 256), (3, 257), (2, 1023), (6, 1025),
              (T - 1, 300), (T, 300), (T + 1, 300), (2 * T + 1, 300)]


def plane(rows):
    return np.array([[1.0 if ch == "#" else 0.0 for ch in row] for row in rows], np.float32)


def triples(overlaps):
    return [(int(o["before"]), int(o["after"]), int(o["cells"])) for o in overlaps]


def the_match(before, after, t=0.5, above=True, connectivity=8, min_size=1):
    from grayscott_amd import ComponentList, ComponentMatch

    rb, ra, ov = ref.match(before, after, t, above, connectivity, min_size)
    lb, la, ol = ref.literal(before, after, t, above, connectivity, min_size)
    assert np.array_equal(rb, lb) and np.array_equal(ra, la) and np.array_equal(ov, ol)
    shape = np.asarray(before).shape
    rule = (shape[0], shape[1], float(np.float32(t)), above, connectivity, min_size)
    return ComponentMatch(ComponentList(rb, *rule), ComponentList(ra, *rule), ov)


# ---- hand-counted cases ------------------------------------------------------------------------------------------------------

def test_identity_and_disjoint_planes():
    a = plane(["##...",
               "#..#.",
               "...##",
               "#...."])
    m = the_match(a, a, connectivity=4)
    assert list(m.before.sizes) == [3, 3, 1] and triples(m.overlaps) == [(0, 0, 3), (1, 1, 3), (2, 2, 1)]
    assert m.counts() == {"continued": 3, "split": 0, "merged": 0, "born": 0, "died": 0}
    assert np.array_equal(m.displacements(), np.zeros((3, 2)))
    b = plane(["..##.",
               ".#...",
               "##...",
               ".###."])
    d = the_match(a, b, connectivity=4)
    assert d.overlaps.shape == (0,) and d.overlaps.dtype == ref.OVERLAP
    assert list(d.after.sizes) == [2, 6] and d.counts() == {"continued": 0, "split": 0, "merged": 0, "born": 2, "died": 3}
    assert list(d.born()) == [0, 1] and list(d.died()) == [0, 1, 2] and d.displacements().shape == (0, 2)


def test_a_bar_cut_in_two_and_its_reverse():
    bar = plane([".......",
                 ".#####.",
                 "......."])
    cut = plane([".......",
                 ".##.##.",
                 "......."])
    s = the_match(bar, cut)
    assert triples(s.overlaps) == [(0, 0, 2), (0, 1, 2)]
    assert s.counts() == {"continued": 0, "split": 1, "merged": 0, "born": 0, "died": 0}
    assert list(s.split()) == [0] and list(s.children(0)) == [0, 1] and list(s.degree_before()) == [2] and list(s.degree_after()) == [1, 1]
    m = the_match(cut, bar)
    assert triples(m.overlaps) == [(0, 0, 2), (1, 0, 2)]
    assert m.counts() == {"continued": 0, "split": 0, "merged": 1, "born": 0, "died": 0}
    assert list(m.merged()) == [0] and list(m.parents(0)) == [0, 1]


def test_two_pieces_of_one_pair_are_one_overlap():
    u = plane(["#...#",
               "#...#",
               "#...#",
               "#####"])
    bar = plane([".....",
                 "#####",
                 ".....",
                 "....."])
    for conn in (4, 8):
        m = the_match(u, bar, connectivity=conn)
        assert triples(m.overlaps) == [(0, 0, 2)] and list(ref.pieces(u, bar, 0.5, True, conn)) == [2]
        assert m.counts() == {"continued": 1, "split": 0, "merged": 0, "born": 0, "died": 0}


def test_a_shifted_copy_continues_every_pair():
    a = np.zeros((12, 16), np.float32)
    a[1:4, 1:5] = a[6:9, 8:12] = a[2:4, 10:13] = 1
    b = np.zeros_like(a)
    b[1:, 2:] = a[:-1, :-2]
    m = the_match(a, b, connectivity=4)
    assert m.before.count == 3 and triples(m.overlaps) == [(0, 0, 4), (1, 1, 1), (2, 2, 4)]
    assert np.array_equal(m.continued(), [[0, 0], [1, 1], [2, 2]])
    assert np.array_equal(m.displacements(), [[1.0, 2.0]] * 3)
    assert m.counts() == {"continued": 3, "split": 0, "merged": 0, "born": 0, "died": 0}


def test_nan_infinite_and_threshold_cells():
    nan, inf = np.nan, np.inf
    before = np.array([[0.7, nan, 0.5, inf],
                       [0.7, 0.2, 0.5, inf]], np.float32)
    after = np.array([[0.7, 0.9, 0.6, -inf],
                      [nan, 0.5, 0.5, inf]], np.float32)
    m = the_match(before, after, connectivity=4)        # before: {(0,0), (1,0)}, {(0,3), (1,3)}; after: {(0,0), (0,1), (0,2)}, {(1,3)}
    assert list(m.before.sizes) == [2, 2] and list(m.after.sizes) == [3, 1]
    assert triples(m.overlaps) == [(0, 0, 1), (1, 1, 1)]
    below = the_match(before, after, above=False, connectivity=4)   # before: {(1,1)}; after: {(0,3)}: NaN and 0.5 are never set
    assert list(below.before.sizes) == [1] and list(below.after.sizes) == [1] and triples(below.overlaps) == []
    at_inf = the_match(before, after, t=inf, above=False, connectivity=8)  # below +inf: everything finite or -inf
    assert list(at_inf.before.sizes) == [5] and list(at_inf.after.sizes) == [6] and triples(at_inf.overlaps) == [(0, 0, 4)]
    corner = the_match(before, after, connectivity=8)   # (0,2) and (1,3) touch at a corner: one component under 8
    assert list(corner.after.sizes) == [4] and triples(corner.overlaps) == [(0, 0, 1), (1, 0, 1)]


def test_min_size_removes_one_partner_of_a_split():
    bar = plane(["#######"])
    cut = plane(["#.#####"])
    assert triples(the_match(bar, cut).overlaps) == [(0, 0, 1), (0, 1, 5)]
    m = the_match(bar, cut, min_size=2)
    assert list(m.after.sizes) == [5] and triples(m.overlaps) == [(0, 0, 5)]
    assert m.counts() == {"continued": 1, "split": 0, "merged": 0, "born": 0, "died": 0}
    gone = the_match(bar, cut, min_size=6)
    assert gone.after.count == 0 and gone.before.count == 1 and triples(gone.overlaps) == [] and list(gone.died()) == [0]


# ---- the restatement against the literal loop ----------------------------------------------------------------------------------

CPU_SHAPES = [(1, 1), (3, 3), (9, 14), (16, 16), (30, 7), (25, 40), (40, 40), (5, 60)]


@pytest.mark.parametrize("seed", range(3))
def test_reference_against_the_literal_loop(seed):
    rng = np.random.default_rng(seed)
    shared = 0
    for shape in CPU_SHAPES:
        for density in (0.2, 0.5, 0.593, 0.8):
            before = rng.random(shape, dtype=np.float32)
            after = rng.random(shape, dtype=np.float32)
            t = 1.0 - density
            for conn in (4, 8):
                for min_size in (1, 2, 7):
                    rb, ra, ov = ref.match(before, after, t, True, conn, min_size)
                    lb, la, ol = ref.literal(before, after, t, True, conn, min_size)
                    assert np.array_equal(rb, lb) and np.array_equal(ra, la), (shape, density, conn, min_size)
                    assert np.array_equal(ov, ol), (shape, density, conn, min_size)
                    assert np.all(ov["cells"] >= 1)
                    keys = ov["before"].astype(np.int64) * (len(ra) + 1) + ov["after"].astype(np.int64)
                    assert np.all(np.diff(keys) > 0), "ascending (before, after), every pair once"
                    for side, rec in (("before", rb), ("after", ra)):          # a record's overlaps: at most its size
                        held = np.bincount(ov[side].astype(np.int64), weights=ov["cells"].astype(np.float64), minlength=len(rec))
                        assert np.all(held <= rec["size"])
                    if min_size == 1:
                        both = (before > np.float32(t)) & (after > np.float32(t))
                        assert int(ov["cells"].sum()) == int(both.sum())
                        assert int(ref.pieces(before, after, t, True, conn).sum()) >= len(ov)
                        shared += len(ov)
    assert shared > 100


# ---- the generator of the GPU tests' planes ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ref.KINDS)
def test_pair_of_planes_shows_its_events(kind):
    """Summed over the shapes the GPU tests use, every kind shows each event it is meant to show -- for both connectivities
    and both min_sizes of those tests --, and some pair is made of two pieces: the GPU parity does not pass on matches with
    nothing in them."""
    for conn in (4, 8):
        for min_size in (1, 3):
            total = dict.fromkeys(("continued", "split", "merged", "born", "died"), 0)
            several = 0
            for shape in GPU_SHAPES:
                before, after = ref.pair_of_planes(shape, 1, kind)
                assert before.shape == after.shape == shape and before.dtype == after.dtype == np.float32
                again = ref.pair_of_planes(shape, 1, kind)
                assert before.tobytes() == again[0].tobytes() and after.tobytes() == again[1].tobytes()
                rb, ra, ov = ref.match(before, after, ref.THRESHOLD, True, conn, min_size)
                for name, n in ref.events(rb, ra, ov).items():
                    total[name] += n
                several += int((ref.pieces(before, after, ref.THRESHOLD, True, conn, min_size) >= 2).sum())
            print(kind, conn, min_size, total, several)
            for name in ref.EVENTS[kind]:
                assert total[name] > 0, (kind, conn, min_size, name, total)
            if kind in ("noise", "flip"):
                assert several > 0, (kind, conn, min_size)
    everything = set()
    for k in ref.KINDS:
        everything |= set(ref.EVENTS[k])
    assert everything == {"continued", "split", "merged", "born", "died"}


def test_planes_hold_awkward_values():
    before, after = ref.pair_of_planes((40, 300), 2, "noise")
    for p in (before, after):
        assert np.isnan(p).any() and (p == np.float32(0.5)).any() and np.isposinf(p).any() and np.isneginf(p).any()


# ---- the object ------------------------------------------------------------------------------------------------------------------

def test_component_match_object():
    from grayscott_amd import ComponentList, ComponentMatch
    from grayscott_amd.simulation import COMPONENT_OVERLAP_DTYPE

    assert COMPONENT_OVERLAP_DTYPE == ref.OVERLAP and COMPONENT_OVERLAP_DTYPE.itemsize == 16

    def a_list(sizes, rows, cols):
        rec = np.zeros(len(sizes), component_list_ref.DTYPE)
        rec["size"], rec["sum_row"], rec["sum_col"] = sizes, np.multiply(sizes, rows), np.multiply(sizes, cols)
        return ComponentList(rec, 64, 64, 0.5, True, 8, 1)

    # before: 0 continues as 0; 1 splits into 1 and 2; 2 and 3 merge into 3; 4 dies.  after 4 is born; after 5 takes part in a
    # many-to-many: before 5 -> 5, 6 and before 6 -> 6.
    before = a_list([4, 9, 3, 3, 1, 8, 2], [1, 5, 9, 9, 20, 30, 33], [1, 5, 9, 13, 20, 30, 30])
    after = a_list([4, 4, 4, 6, 2, 3, 6], [2.5, 5, 5, 9, 40, 30, 32], [1, 3, 8, 11, 40, 29, 31])
    pairs = [(0, 0, 3), (1, 1, 4), (1, 2, 3), (2, 3, 3), (3, 3, 2), (5, 5, 3), (5, 6, 4), (6, 6, 2)]
    m = ComponentMatch(before, after, np.array(pairs, COMPONENT_OVERLAP_DTYPE))
    assert list(m.degree_before()) == [1, 2, 1, 1, 0, 2, 1] and list(m.degree_after()) == [1, 1, 1, 2, 0, 1, 2]
    assert m.degree_before().dtype == np.int64 and m.degree_after().dtype == np.int64
    assert np.array_equal(m.continued(), [[0, 0]]) and m.continued().dtype == np.int64
    assert list(m.split()) == [1, 5] and list(m.children(1)) == [1, 2] and list(m.children(5)) == [5, 6] and list(m.children(4)) == []
    assert list(m.merged()) == [3, 6] and list(m.parents(3)) == [2, 3] and list(m.parents(6)) == [5, 6] and list(m.parents(4)) == []
    assert list(m.born()) == [4] and list(m.died()) == [4]
    assert np.array_equal(m.displacements(), [[1.5, 0.0]]) and m.displacements().dtype == np.float64
    assert m.counts() == {"continued": 1, "split": 2, "merged": 2, "born": 1, "died": 1}
    none = ComponentMatch(a_list([], [], []), a_list([], [], []), np.zeros(0, COMPONENT_OVERLAP_DTYPE))
    assert none.counts() == dict.fromkeys(("continued", "split", "merged", "born", "died"), 0)
    assert none.continued().shape == (0, 2) and none.displacements().shape == (0, 2) and none.degree_before().shape == (0,)
    assert none.split().shape == none.merged().shape == none.born().shape == none.died().shape == (0,)
    lone = ComponentMatch(before, a_list([], [], []), np.zeros(0, COMPONENT_OVERLAP_DTYPE))
    assert lone.counts() == {"continued": 0, "split": 0, "merged": 0, "born": 0, "died": 7}


# ---- exports, layouts, refusals ---------------------------------------------------------------------------------------------------

NAMES = ("gs_fields_match", "gs_members_match", "gs_component_match_view", "gs_component_match_destroy")


def test_match_entry_points_are_exported(built):
    from grayscott_amd import capi
    import grayscott_amd

    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(lib, name) and f"int32_t {name}(" in header and f"pub fn {name}(" in ffi, name
    assert "typedef struct gs_component_overlap" in header and "typedef struct gs_component_match gs_component_match;" in header
    assert "pub struct gs_component_overlap" in ffi and "pub struct gs_component_match" in ffi
    assert "matching of spots across time" not in header and "label planes for the caller" in header
    assert "matching of spots across time" not in open(os.path.join(ROOT, "DESIGN.md")).read()
    for gap in ("multi-process contexts", "wrapped components", "matching by distance where nothing overlaps",
                "tracks over more than", "float-weighted overlaps"):
        assert gap in " ".join(header.split("gs_component_match_destroy  frees")[1].split("typedef struct gs_component_overlap")[0]
                               .replace(" * ", " ").split()), gap
    assert "ComponentMatch" in grayscott_amd.__all__
    assert lib.gs_abi_version() == 4
    O = capi.GsComponentOverlap
    assert ctypes.sizeof(O) == 16 == ref.OVERLAP.itemsize
    for name, at in {"before": 0, "after": 4, "cells": 8}.items():
        assert getattr(O, name).offset == at == ref.OVERLAP.fields[name][1], name


def test_match_refusals_need_no_device(built):
    """Argument checks come before any device work, in the lists' order: a null argument, a NaN threshold, the connectivity,
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
    field, members = lib.gs_fields_match, lib.gs_members_match

    assert field(None, None, None, 0.5, 1, 8, 1, ref_out) == INV and "null" in err()
    assert field(ctx, None, None, 0.5, 1, 8, 1, None) == INV and "null argument" in err()
    assert field(ctx, None, None, nan, 1, 5, 0, None) == INV and "null argument" in err()                  # null comes first
    assert members(None, None, None, 0, 1, 1, 0.5, 1, 8, 1, ref_out) == INV and "null" in err()
    assert members(ctx, None, None, 0, 1, 7, nan, 1, 5, 0, None) == INV and "null argument" in err()
    assert field(ctx, None, None, nan, 1, 5, 0, ref_out) == INV and "NaN" in err()                           # NaN before the rest
    assert members(ctx, None, None, 0, 1, 7, nan, 1, 5, 0, ref_out) == INV and "NaN" in err()
    for conn in (0, 1, 5, 6, 16, -8):                                                                        # then the connectivity
        assert field(ctx, None, None, 0.5, 1, conn, 0, ref_out) == INV and "connectivity" in err(), conn
        assert members(ctx, None, None, 0, 1, 7, 0.5, 1, conn, 0, ref_out) == INV and "connectivity" in err(), conn
    for conn in (4, 8):
        assert field(ctx, None, None, 0.5, 1, conn, 0, ref_out) == INV and "min_size" in err()               # then min_size
        assert members(ctx, None, None, 0, 1, 7, 0.5, 0, conn, 0, ref_out) == INV and "min_size" in err()
        for species in (-1, 2, 7):                                                                           # then the species
            assert members(ctx, None, None, 0, 1, species, 0.5, 1, conn, 1, ref_out) == INV and "species" in err(), species
        assert field(ctx, None, None, 0.5, 1, conn, 1, ref_out) == INV and "field: null" in err()            # and only then the handles
        assert field(ctx, None, None, math.inf, 0, conn, 1 << 40, ref_out) == INV and "field: null" in err()
        for species in (0, 1):
            assert members(ctx, None, None, 0, 1, species, -math.inf, 1, conn, 1, ref_out) == INV and "null argument" in err()
    assert not out                                                 # no refusal returns a match
    assert lib.gs_component_match_destroy(None) == capi.GS_OK
    before, after = ctypes.c_void_p(), ctypes.c_void_p()
    planes, offsets, overlaps = ctypes.c_uint64(0), ctypes.POINTER(ctypes.c_uint64)(), ctypes.POINTER(capi.GsComponentOverlap)()
    assert lib.gs_component_match_view(None, ctypes.byref(before), ctypes.byref(after), ctypes.byref(planes), ctypes.byref(offsets),
                                       ctypes.byref(overlaps)) == INV


# ---- the sweep driver --------------------------------------------------------------------------------------------------------------

def test_sweep_track_flags():
    from grayscott_amd import sweep

    base = ["--feed", "0.01:0.02:2", "--kill", "0.05:0.05:1", "-s", "10", "-o", "out/run.h5"]
    a = sweep.parse(base)
    assert a.track_every == 0 and a.track_threshold_v is None and a.track_min_size == 1 and a.track_connectivity == 8
    b = sweep.parse(base + ["--track-every", "4", "--track-threshold-v", "0.25", "--summary-every", "5"])
    assert b.track_every == 4 and b.track_threshold_v == 0.25
    c = sweep.parse(base + ["--track-every", "4", "--track-threshold-v=-0.5", "--track-min-size", "9", "--track-connectivity", "4",
                            "--no-fields"])
    assert c.track_threshold_v == -0.5 and c.track_min_size == 9 and c.track_connectivity == 4
    assert sweep.tracks_path("out/run.h5") == os.path.join("out", "run.tracks.npz")
    for wrong in (["--track-every", "-1"], ["--track-every", "2"], ["--track-every", "2", "--track-threshold-v", "nan"],
                  ["--track-every", "2", "--track-threshold-v", "a"],
                  ["--track-every", "2", "--track-threshold-v", "0.1", "--track-min-size", "0"],
                  ["--track-every", "2", "--track-threshold-v", "0.1", "--track-connectivity", "6"]):
        with pytest.raises(SystemExit):
            sweep.parse(base + wrong)


def test_write_tracks(tmp_path):
    from grayscott_amd import sweep

    bar = plane(["......", ".####.", "......"])
    cut = plane(["......", ".#.##.", "......"])
    moved = plane(["......", "......", "..####"])
    empty = np.zeros_like(bar)
    samples = [[the_match(bar, cut), the_match(empty, empty)], [the_match(cut, bar), the_match(bar, moved, connectivity=4)]]
    sweep.write_tracks(str(tmp_path / "t.npz"), [3, 6], samples, 0.5, 8, 1)
    z = np.load(tmp_path / "t.npz")
    assert list(z["steps"]) == [3, 6] and float(z["threshold"]) == 0.5 and int(z["connectivity"]) == 8 and int(z["min_size"]) == 1
    assert list(z["offsets"]) == [0, 2, 2, 4, 4] and z["overlaps"].dtype == ref.OVERLAP
    assert triples(z["overlaps"]) == [(0, 0, 1), (0, 1, 2), (0, 0, 1), (1, 0, 2)]
    assert z["split"].tolist() == [[1, 0], [0, 0]] and z["merged"].tolist() == [[0, 0], [1, 0]]
    assert z["born"].tolist() == [[0, 0], [0, 1]] and z["died"].tolist() == [[0, 0], [0, 1]] and z["continued"].tolist() == [[0, 0], [0, 0]]
    assert list(z["displacement_offsets"]) == [0, 0, 0, 0, 0] and z["displacements"].shape == (0, 2)
    sweep.write_tracks(str(tmp_path / "u.npz"), [5], [[the_match(bar, bar)]], 0.5, 8, 1)
    z = np.load(tmp_path / "u.npz")
    assert list(z["displacement_offsets"]) == [0, 1] and z["displacements"].tolist() == [[0.0, 0.0]] and z["continued"].tolist() == [[1]]


# ---- the host side of the seam merge ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitize", [False, True])
def test_match_merge_on_the_host(tmp_path, sanitize):
    """tests/cpp/match_merge.cpp: pairs of planes cut into 1..5 slabs (one-row slabs included), each labelled on the host with
    the shared find / unite, through the index map of the list merge and the overlap fold against the whole planes' match -- a
    stand-alone program, also built with the address and undefined-behaviour sanitizers."""
    exe = build_program("match_merge", tmp_path, library=False, sanitize=sanitize)
    r = run_program([str(exe)])
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_cpp_match_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("match_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_match.py)
        r = run_program([str(exe), "3", "8", "16", "5", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
