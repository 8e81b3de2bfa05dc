"""Comparisons of two states (gs_fields_compare / gs_members_compare) and device copies (gs_fields_copy / gs_members_copy)
without a GPU: the numpy restatement of the rule (tests/change_ref.py) against the literal per-cell definition, the rule's
special cases, the gs_change layout in every binding, the exports, null handles, the sweep's flags, and the C++ mirror's
build."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import change_ref
from tests.children import ROOT, build_program, run_program

SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -3e-39, 3.4028235e38,
                     -3.4028235e38], np.float32)


def planted(shape, seed):
    """Two planes of random cells with the special values planted in either and in both."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(shape) * 3).astype(np.float32)
    b = a + (rng.standard_normal(shape) * 1e-3).astype(np.float32)
    b.flat[rng.choice(a.size, size=a.size // 3, replace=False)] = 0.0
    b = np.where(b == 0.0, a, b)                                    # a third of the cells equal
    n = a.size
    for plane, k in ((a, 1), (b, 2), (a, 3), (b, 3)):
        r = np.random.default_rng(seed * 10 + k)
        idx = r.choice(n, size=min(n, 2 * len(SPECIALS)), replace=False)
        plane.flat[idx] = np.resize(SPECIALS, len(idx))
    return a, b


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (7, 13), (3, 256), (2, 257), (5, 600), (2, 1030)])
@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_matches_the_literal_definition(shape, seed):
    a, b = planted(shape, seed)
    got, want = change_ref.change(a, b), change_ref.literal(a, b)
    assert change_ref.same(got, want), (got, want)
    # blocks of rows change nothing: the row fold is sequential
    assert change_ref.same(change_ref.change(a, b, block_rows=2), want)
    a, b = change_ref.order_sensitive(shape, seed)
    assert change_ref.same(change_ref.change(a, b), change_ref.literal(a, b))


def f32(*values):
    return np.array([values], np.float32)


def test_restatement_special_cases():
    nan, inf = np.nan, np.inf
    zero = {"sum_abs": 0.0, "sum_sq": 0.0, "max_abs": 0.0, "differing": 0, "nonfinite": 0}
    assert change_ref.change(np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32)) == zero
    # NaN in a only, in b only, in both: not comparable, add nothing; the finite cell beside them counts
    c = change_ref.change(f32(nan, 1.0, nan, 3.0), f32(2.0, nan, nan, 1.0))
    assert c == {"sum_abs": 2.0, "sum_sq": 4.0, "max_abs": 2.0, "differing": 3, "nonfinite": 3}
    # inf - inf is not NaN here: the cell is not comparable; nor is inf against a finite cell
    c = change_ref.change(f32(inf, inf, -inf, 5.0), f32(inf, -inf, 1.0, inf))
    assert c["nonfinite"] == 4 and c["differing"] == 3
    assert all(change_ref.bits(c[f]) == 0 for f in ("sum_abs", "sum_sq", "max_abs"))
    # +0 against -0: differing bits, d = 0
    c = change_ref.change(f32(0.0, -0.0), f32(-0.0, 0.0))
    assert c["differing"] == 2 and c["nonfinite"] == 0
    assert all(change_ref.bits(c[f]) == 0 for f in ("sum_abs", "sum_sq", "max_abs"))
    # sub-normal cells count as the values they are: d = 2^-148, d * d = 2^-296, both exact in f64
    c = change_ref.change(f32(1e-45), f32(-1e-45))
    assert c["max_abs"] == c["sum_abs"] == 2.0 ** -148 and c["sum_sq"] == 2.0 ** -296 and c["differing"] == 1
    # NaN payloads: the same bits do not differ, other payloads do
    a = np.array([[0x7fc00000, 0x7fc00001, 0xffc00000]], np.uint32).view(np.float32)
    b = np.array([[0x7fc00000, 0x7fc00002, 0x7fc00000]], np.uint32).view(np.float32)
    c = change_ref.change(a, b)
    assert c["differing"] == 2 and c["nonfinite"] == 3
    assert change_ref.same(c, change_ref.literal(a, b))
    # one f64 subtraction: 2^100 - 1 rounds to 2^100, and its square does not overflow; nor does (2 FLT_MAX)^2
    c = change_ref.change(f32(2.0 ** 100, 3.4028235e38), f32(1.0, -3.4028235e38))
    assert c["sum_abs"] == 2.0 ** 100 + 2 * float(np.float32(3.4028235e38)) and math.isfinite(c["sum_sq"])


@pytest.mark.parametrize("shape", [(37, 1029), (3, 600), (1, 300)])
def test_the_test_planes_are_order_sensitive(shape):
    """What makes a GPU kernel with the wrong fold order fail: on these planes plain ascending column order gives other
    bits in both sums."""
    a, b = change_ref.order_sensitive(shape, 4)
    right, wrong = change_ref.change(a, b), change_ref.ascending(a, b)
    assert change_ref.bits(right["sum_abs"]) != change_ref.bits(wrong["sum_abs"])
    assert change_ref.bits(right["sum_sq"]) != change_ref.bits(wrong["sum_sq"])
    assert right["max_abs"] == wrong["max_abs"] and right["differing"] == wrong["differing"] == a.size


def test_change_layouts():
    from grayscott_amd import capi
    from grayscott_amd.simulation import CHANGE_DTYPE

    C = capi.GsChange
    assert ctypes.sizeof(C) == 40
    assert [(n, getattr(C, n).offset) for n in change_ref.FIELDS] == \
        [("sum_abs", 0), ("sum_sq", 8), ("max_abs", 16), ("differing", 24), ("nonfinite", 32)]
    assert CHANGE_DTYPE.itemsize == 40
    assert [CHANGE_DTYPE.fields[n][1] for n in change_ref.FIELDS] == [0, 8, 16, 24, 32]
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    body = header[header.index("typedef struct gs_change {"):header.index("} gs_change;")]
    assert [" ".join(l.split(";")[0].split()) for l in body.splitlines()[1:] if ";" in l] == \
        ["double sum_abs", "double sum_sq", "double max_abs", "uint64_t differing", "uint64_t nonfinite"]
    ffi = open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    rust = ffi[ffi.index("pub struct gs_change {"):]
    rust = rust[:rust.index("}")]
    assert [x.strip() for x in rust.splitlines()[1:] if x.strip()] == \
        ["pub sum_abs: f64,", "pub sum_sq: f64,", "pub max_abs: f64,", "pub differing: u64,", "pub nonfinite: u64,"]
    for name in ("gs_fields_compare", "gs_members_compare", "gs_fields_copy", "gs_members_copy"):
        assert f"pub fn {name}(" in ffi, name
    hpp = open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    for name in ("Snapshot snapshot()", "change_since(", "void restore(", "Ensemble snapshot()", "changes_since("):
        assert name in hpp, name


def test_change_entry_points_are_exported_and_reject_null_handles(built):
    from grayscott_amd import capi

    lib = capi.load()
    for name in ("gs_fields_compare", "gs_members_compare", "gs_fields_copy", "gs_members_copy"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    out = (capi.GsChange * 4)()
    fields = (ctypes.c_void_p * 1)(None)
    INV = capi.GS_ERR_INVALID
    assert lib.gs_fields_compare(None, fields, fields, 1, out) == INV
    assert lib.gs_fields_compare(None, None, None, 0, out) == INV
    assert lib.gs_members_compare(None, None, None, 0, 1, out) == INV
    assert lib.gs_fields_copy(None, fields, fields, 1) == INV
    assert lib.gs_fields_copy(None, None, None, 1) == INV
    assert lib.gs_members_copy(None, None, None, 0, 1) == INV
    assert b"null" in lib.gs_last_error()


def test_change_object_statistics():
    from grayscott_amd import Change

    c = Change(sum_abs=6.0, sum_sq=18.0, max_abs=4.0, differing=2, nonfinite=1, cells=3)
    assert c.comparable == 2 and not c.equal and c.mean_abs == 3.0 and c.rms == 3.0
    none = Change(sum_abs=0.0, sum_sq=0.0, max_abs=0.0, differing=0, nonfinite=2, cells=2)
    assert none.comparable == 0 and none.equal and math.isnan(none.mean_abs) and math.isnan(none.rms)


BASE = ["--feed", "0.01:0.02:2", "--kill", "0.05:0.05:1"]


def test_sweep_steady_flags():
    from grayscott_amd import sweep

    a = sweep.parse(BASE + ["-s", "10", "-o", "out/run.h5"])
    assert a.steady_every == 0 and a.steady_tol == 0.0 and not a.steady_stop
    b = sweep.parse(BASE + ["--steady-every", "4", "--steady-tol", "1e-3", "--steady-stop", "-o", "out/run.h5"])
    assert b.steady_every == 4 and b.steady_tol == 1e-3 and b.steady_stop
    assert sweep.parse(BASE + ["--steady-every", "4", "--steady-tol", "inf"]).steady_tol == math.inf
    assert sweep.steady_path("out/run.h5") == os.path.join("out", "run.steady.npz")
    for bad in (["--steady-every", "-1"], ["--steady-every", "4", "--steady-tol", "-1e-9"],
                ["--steady-every", "4", "--steady-tol", "nan"], ["--steady-stop"],
                ["--steady-stop", "--steady-tol", "1"]):
        with pytest.raises(SystemExit):
            sweep.parse(BASE + bad)


def test_sweep_settled_steps():
    from grayscott_amd import sweep

    max_abs = np.array([[[0.0, 0.0], [0.0, 0.0], [9.0, 9.0]],      # settled at the first sample (and stays recorded so)
                        [[1.0, 0.0], [0.5, 0.5], [0.0, 0.0]],      # U and V must both be within the tolerance
                        [[1.0, 1.0], [1.0, 0.0], [0.6, 0.0]]])     # never
    assert list(sweep.settled_steps([5, 10, 12], max_abs, 0.5)) == [5, 10, -1]
    assert list(sweep.settled_steps([5, 10, 12], max_abs, math.inf)) == [5, 5, 5]
    assert list(sweep.settled_steps([5, 10, 12], max_abs, 0.0)) == [5, 12, -1]
    assert sweep.settled_steps([5, 10, 12], max_abs, 0.0).dtype == np.int64


def test_cpp_change_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("change_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_change.py)
        r = run_program([str(exe), "3", "8", "16", "5", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
