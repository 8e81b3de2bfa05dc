"""Histograms (gs_fields_histogram / gs_members_histogram) without a GPU: the numpy restatement of the binning rule
(tests/hist_ref.py) against the literal per-cell definition, the exports, null handles and every refusal that needs no
device, the sweep's flags, the Histogram object's statistics, the Rust declarations and the C++ mirror's build."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import hist_ref
from tests.children import ROOT, build_program, run_program

ONE = np.float32(1.0)
# (lo, hi, bins): the defaults of U and V, one bin, an odd count on a range that is no power of two, the most bins, and a
# range eight ulps of 1.0 wide
SETTINGS = [(0.0, 1.0, 256), (0.0, 0.5, 256), (0.0, 1.0, 1), (-2.5, 3.75, 7), (0.0, 0.5, 4096), (0.1, 0.9, 4096),
            (1.0, float(ONE + np.float32(8 * 2.0 ** -23)), 4)]


@pytest.mark.parametrize("shape", [(1, 1), (7, 13), (2, 257), (2, 1030)])
@pytest.mark.parametrize("lo,hi,bins", SETTINGS)
def test_restatement_matches_the_literal_definition(shape, lo, hi, bins):
    for seed in (0, 1):
        a = hist_ref.planted(shape, lo, hi, bins, seed)
        got, want = hist_ref.histogram(a, lo, hi, bins), hist_ref.literal(a, lo, hi, bins)
        assert got.dtype == np.uint64 and got.shape == (bins + 3,)
        assert np.array_equal(got, want), (got, want)
        assert int(got.sum()) == a.size


@pytest.mark.parametrize("lo,hi,bins", SETTINGS)
def test_rule_consequences(lo, hi, bins):
    lo32, hi32, inf = np.float32(lo), np.float32(hi), np.float32(np.inf)
    at = lambda x: int(hist_ref.slots(np.array([x], np.float32), lo, hi, bins)[0])  # noqa: E731
    assert at(hi32) == bins - 1                                   # the last bin is closed
    assert at(lo32) == 0
    assert at(np.nextafter(lo32, -inf)) == bins and at(-inf) == bins
    assert at(np.nextafter(hi32, inf)) == bins + 1 and at(inf) == bins + 1
    assert at(np.nan) == bins + 2
    if lo32 == 0:
        assert at(np.float32(-0.0)) == 0 and at(np.float32(1e-45)) == 0
    # t is monotone in x: every bin is an interval
    x = np.sort(hist_ref.planted((40, 50), lo, hi, bins, 3).ravel())
    x = x[(x >= lo32) & (x <= hi32)]
    t = hist_ref.t_of(x, lo, hi, bins)
    assert np.all(np.diff(t) >= 0)
    assert np.all(np.diff(hist_ref.slots(x, lo, hi, bins)) >= 0)


def test_numpy_histogram_is_another_rule():
    # values next to the nominal edges of 1000 bins of [0, 1]: the f32 product x * 1000 rounds across the edge where
    # numpy's f64 arithmetic does not
    lo, hi, bins = 0.0, 1.0, 1000
    e = (np.arange(1, bins, dtype=np.float64) / bins).astype(np.float32)
    a = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))])
    ours = hist_ref.histogram(a, lo, hi, bins)
    theirs, _ = np.histogram(a, bins=bins, range=(lo, hi))
    assert np.array_equal(ours, hist_ref.literal(a, lo, hi, bins))
    assert int(ours[:bins].sum()) == int(theirs.sum()) == a.size
    assert np.count_nonzero(ours[:bins] != theirs.astype(np.uint64)) > 0


def test_histogram_entry_points_are_exported(built):
    from grayscott_amd import capi

    lib = capi.load()
    for name in ("gs_fields_histogram", "gs_members_histogram"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    assert "int32_t gs_fields_histogram(" in header and "int32_t gs_members_histogram(" in header
    assert lib.gs_abi_version() == 4


def _f32(*values):
    return (ctypes.c_float * len(values))(*values)


def test_histogram_refusals_need_no_device(built):
    """Argument checks come before any device work: with a context pointer that is never looked at and null plane /
    ensemble handles, every refusal of the header returns GS_ERR_INVALID with its own message."""
    from grayscott_amd import capi

    lib = capi.load()
    INV = capi.GS_ERR_INVALID
    out = (ctypes.c_uint64 * (4 * (4096 + 3)))()
    fields = (ctypes.c_void_p * 4)(None, None, None, None)
    dummy = ctypes.create_string_buffer(4096)                      # stands for a context; no check reads it
    ctx = ctypes.cast(dummy, ctypes.c_void_p)
    lo, hi = _f32(0, 0, 0, 0), _f32(1, 1, 1, 1)
    err = lambda: lib.gs_last_error().decode()  # noqa: E731

    # null handles and pointers
    assert lib.gs_fields_histogram(None, fields, 1, lo, hi, 16, out) == INV and "null" in err()
    assert lib.gs_fields_histogram(ctx, None, 1, lo, hi, 16, out) == INV and "null" in err()
    assert lib.gs_fields_histogram(ctx, fields, 1, None, hi, 16, out) == INV and "null" in err()
    assert lib.gs_fields_histogram(ctx, fields, 1, lo, None, 16, out) == INV and "null" in err()
    assert lib.gs_fields_histogram(ctx, fields, 1, lo, hi, 16, None) == INV and "null" in err()
    assert lib.gs_fields_histogram(ctx, fields, 1, lo, hi, 16, out) == INV and "field 0" in err()
    assert lib.gs_members_histogram(None, None, 0, 1, lo, hi, 16, out) == INV and "null" in err()
    assert lib.gs_members_histogram(ctx, None, 0, 1, lo, hi, 16, out) == INV and "null" in err()
    assert lib.gs_members_histogram(ctx, None, 0, 1, None, hi, 16, out) == INV and "null" in err()
    # n outside 1..4
    for n in (0, -1, 5):
        assert lib.gs_fields_histogram(ctx, fields, n, lo, hi, 16, out) == INV and "fields (1..4)" in err(), n
    # bins outside 1..4096
    for bins in (0, -3, 4097, 1 << 20):
        assert lib.gs_fields_histogram(ctx, fields, 1, lo, hi, bins, out) == INV and "bins" in err(), bins
        assert lib.gs_members_histogram(ctx, None, 0, 1, lo, hi, bins, out) == INV and "bins" in err(), bins
    for bins in (1, 4096):
        assert lib.gs_fields_histogram(ctx, fields, 1, lo, hi, bins, out) == INV and "field 0" in err(), bins
    # ranges: not finite, lo >= hi, a width or a scale that is no normal positive f32
    big, tiny = 3.4028235e38, 1e-45
    bad = [(math.nan, 1.0, 16), (0.0, math.nan, 16), (-math.inf, 1.0, 16), (0.0, math.inf, 16), (1.0, 1.0, 16),
           (2.0, 1.0, 16), (-big, big, 16),          # hi - lo overflows
           (0.0, tiny, 16), (0.0, 1e-39, 1),         # a sub-normal width
           (0.0, 2e-38, 4096),                       # bins / width overflows
           (0.0, big, 1)]                            # 1 / width is sub-normal
    for a, b, bins in bad:
        assert lib.gs_fields_histogram(ctx, fields, 1, _f32(a), _f32(b), bins, out) == INV and "range 0" in err(), (a, b, bins)
        assert lib.gs_members_histogram(ctx, None, 0, 1, _f32(a, 0), _f32(b, 1), bins, out) == INV and "range 0" in err()
        assert lib.gs_members_histogram(ctx, None, 0, 1, _f32(0, a), _f32(1, b), bins, out) == INV and "range 1" in err()
    # the range of a later field is checked too
    assert lib.gs_fields_histogram(ctx, fields, 3, _f32(0, 0, 5), _f32(1, 1, 5), 16, out) == INV and "range 2" in err()
    # a range that is fine: the refusal is the handle's
    assert lib.gs_fields_histogram(ctx, fields, 2, _f32(0, -1), _f32(1e-30, 1e30), 4096, out) == INV and "field 0" in err()


def test_sweep_histogram_flags():
    from grayscott_amd import sweep

    base = ["--feed", "0.01:0.02:2", "--kill", "0.05:0.05:1", "-s", "10", "-o", "out/run.h5"]
    a = sweep.parse(base)
    assert a.histogram_every == 0 and a.hist_bins == 256
    assert a.hist_range_u == (0.0, 1.0) and a.hist_range_v == (0.0, 0.5)
    b = sweep.parse(base + ["--histogram-every", "4", "--hist-bins", "64", "--hist-range-u", "0.2:1.5",
                            "--hist-range-v=-0.1:0.4", "--summary-every", "5", "--no-fields"])
    assert b.histogram_every == 4 and b.hist_bins == 64 and b.summary_every == 5 and b.no_fields
    assert b.hist_range_u == (0.2, 1.5) and b.hist_range_v == (-0.1, 0.4)
    assert sweep.hist_path("out/run.h5") == os.path.join("out", "run.hist.npz")
    for wrong in (["--histogram-every", "-1"], ["--hist-bins", "0"], ["--hist-bins", "4097"], ["--hist-range-u", "1:0"],
                  ["--hist-range-v", "0.5"]):
        with pytest.raises(SystemExit):
            sweep.parse(base + wrong)


def test_histogram_object_statistics():
    from grayscott_amd import Histogram

    h = Histogram.from_counters(np.array([1, 0, 3, 4, 5, 6, 7], np.uint64), 0.0, 2.0, 100)
    assert list(h.counts) == [1, 0, 3, 4] and (h.below, h.above, h.nan) == (5, 6, 7)
    assert h.bins == 4 and h.in_range == 8 and h.size == 100 and (h.lo, h.hi) == (0.0, 2.0)
    assert list(h.edges()) == [0.0, 0.5, 1.0, 1.5, 2.0] and h.edges().dtype == np.float64
    # bins whose lower edge is at least x, over the 8 in-range cells
    assert h.fraction_above(-1.0) == 1.0 and h.fraction_above(0.0) == 1.0
    assert h.fraction_above(0.5) == 7 / 8 and h.fraction_above(0.25) == 7 / 8
    assert h.fraction_above(1.0) == 7 / 8 and h.fraction_above(1.01) == 4 / 8 and h.fraction_above(1.5) == 4 / 8
    assert h.fraction_above(1.75) == 0.0 and h.fraction_above(2.0) == 0.0 and h.fraction_above(3.0) == 0.0
    # the upper edge of the bin at which the cumulative count reaches ceil(q * 8), at least 1
    assert h.quantile(0.0) == 0.5 and h.quantile(1 / 8) == 0.5
    assert h.quantile(0.2) == 1.5 and h.quantile(0.5) == 1.5 and h.quantile(0.51) == 2.0 and h.quantile(1.0) == 2.0
    with pytest.raises(ValueError):
        h.quantile(1.5)
    none = Histogram.from_counters(np.array([0, 0, 2, 0, 1], np.uint64), 0.0, 1.0, 3)
    assert none.in_range == 0 and math.isnan(none.fraction_above(0.5)) and math.isnan(none.quantile(0.5))


def test_rust_ffi_declares_the_histogram_calls():
    ffi = open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    for name in ("gs_fields_histogram", "gs_members_histogram"):
        at = ffi.index(f"pub fn {name}(")
        decl = ffi[at:ffi.index(";", at)]
        assert "lo: *const f32" in decl and "hi: *const f32" in decl and "bins: i32" in decl and "out: *mut u64" in decl
        assert decl.rstrip().endswith("-> i32")


def test_cpp_histogram_mirror_builds_and_fails_loudly_without_gpu(built, tmp_path):
    exe = build_program("histogram_mirror", tmp_path)
    if not os.path.exists("/dev/kfd"):  # (with a GPU it runs in tests/test_gpu_histogram.py)
        r = run_program([str(exe), "3", "8", "16", "5", "32", str(tmp_path / "o.bin")])
        assert r.returncode == 14 and "HipError" in r.stderr
