"""Summaries (gs_fields_summarize / gs_members_summarize) without a GPU: the numpy restatement of the fold order
(tests/summary_ref.py) against the literal per-cell definition, the gs_summary layout in every binding, the exports, null
handles, the sweep's flags, and the C++ mirror's build."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import summary_ref
from tests.children import ROOT, build_program, run_program

SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -3e-39, 3.4028235e38,
                     -3.4028235e38], np.float32)


def planted(shape, seed):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(shape) * 3).astype(np.float32)
    n = a.size
    if n:
        idx = rng.choice(n, size=min(n, 2 * len(SPECIALS)), replace=False)
        a.flat[idx] = np.resize(SPECIALS, len(idx))
    return a


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (7, 13), (3, 256), (2, 257), (5, 600), (2, 1030)])
@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_matches_the_literal_definition(shape, seed):
    a = planted(shape, seed)
    got, want = summary_ref.summary(a), summary_ref.literal(a)
    assert summary_ref.same(got, want), (got, want)
    # blocks of rows change nothing: the row fold is sequential
    assert summary_ref.same(summary_ref.summary(a, block_rows=2), want)


def test_restatement_special_cases():
    empty = summary_ref.summary(np.zeros((0, 5), np.float32))
    assert empty == {"sum": 0.0, "sum_sq": 0.0, "min": math.inf, "max": -math.inf, "nonfinite": 0}
    bad = summary_ref.summary(np.array([[np.nan, np.inf, -np.inf]], np.float32))
    assert bad["nonfinite"] == 3 and bad["min"] == math.inf and bad["max"] == -math.inf
    assert summary_ref.bits(bad["sum"]) == 0 and summary_ref.bits(bad["sum_sq"]) == 0
    sub = summary_ref.summary(np.array([[1e-45, -0.0, 2e-45]], np.float32))
    assert sub["sum"] == float(np.float32(1e-45)) + float(np.float32(2e-45)) and sub["min"] == 0.0
    # the fold order is not numpy's pairwise sum: a grid where the two differ
    a = np.full((1, 1024), 1.0, np.float32)
    a[0, 0] = 1e8
    assert summary_ref.summary(a)["sum"] == summary_ref.literal(a)["sum"]


def test_summary_layouts():
    from grayscott_amd import capi
    from grayscott_amd.simulation import SUMMARY_DTYPE

    S = capi.GsSummary
    assert ctypes.sizeof(S) == 32
    assert [(n, getattr(S, n).offset) for n in ("sum", "sum_sq", "min", "max", "nonfinite")] == \
        [("sum", 0), ("sum_sq", 8), ("min", 16), ("max", 20), ("nonfinite", 24)]
    assert SUMMARY_DTYPE.itemsize == 32
    assert [SUMMARY_DTYPE.fields[n][1] for n in summary_ref.FIELDS] == [0, 8, 16, 20, 24]
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    body = header[header.index("typedef struct gs_summary {"):header.index("} gs_summary;")]
    assert [l.split(";")[0].strip() for l in body.splitlines()[1:] if ";" in l] == \
        ["double sum", "double sum_sq", "float min, max", "uint64_t nonfinite"]
    ffi = open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    rust = ffi[ffi.index("pub struct gs_summary {"):]
    rust = rust[:rust.index("}")]
    assert [x.strip() for x in rust.splitlines()[1:] if x.strip()] == \
        ["pub sum: f64,", "pub sum_sq: f64,", "pub min: f32,", "pub max: f32,", "pub nonfinite: u64,"]


def test_summary_entry_points_are_exported_and_reject_null_handles(built):
    from grayscott_amd import capi

    lib = capi.load()
    for name in ("gs_fields_summarize", "gs_members_summarize"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    out = (capi.GsSummary * 4)()
    fields = (ctypes.c_void_p * 1)(None)
    assert lib.gs_fields_summarize(None, fields, 1, out) == capi.GS_ERR_INVALID
    assert lib.gs_fields_summarize(None, None, 0, out) == capi.GS_ERR_INVALID
    assert lib.gs_members_summarize(None, None, 0, 1, out) == capi.GS_ERR_INVALID
    assert b"null" in lib.gs_last_error()


def test_sweep_summary_flags():
    from grayscott_amd import sweep

    a = sweep.parse(["--feed", "0.01:0.02:2", "--kill", "0.05:0.05:1", "-s", "10", "-o", "out/run.h5"])
    assert a.summary_every == 0 and not a.no_fields
    b = sweep.parse(["--feed", "0.01:0.02:2", "--kill", "0.05:0.05:1", "--summary-every", "4", "--no-fields",
                     "-o", "out/run.h5"])
    assert b.summary_every == 4 and b.no_fields
    assert sweep.summary_path("out/run.h5") == os.path.join("out", "run.summary.npz")
    assert sweep.sample_steps(10, 4) == [4, 8, 10]
    assert sweep.sample_steps(8, 4) == [4, 8]
    assert sweep.sample_steps(0, 4) == [0]
    assert sweep.sample_steps(3, 5) == [3]
    with pytest.raises(SystemExit):
        sweep.parse(["--feed", "0.01:0.02:2", "--kill", "0.05:0.05:1", "--summary-every", "-1"])


def test_summary_object_statistics():
    from grayscott_amd import Summary

    s = Summary(sum=6.0, sum_sq=14.0, min=1.0, max=3.0, nonfinite=1, size=4)
    assert s.cells == 3 and s.mean == 2.0 and abs(s.std - math.sqrt(14 / 3 - 4)) < 1e-15
    none = Summary(sum=0.0, sum_sq=0.0, min=math.inf, max=-math.inf, nonfinite=2, size=2)
    assert none.cells == 0 and math.isnan(none.mean) and math.isnan(none.std)


def test_cpp_summary_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("summary_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_summary.py)
        r = run_program([str(exe), "3", "8", "16", "5", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
