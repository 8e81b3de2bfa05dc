"""Reduced result images (gs_field_download_reduced and kin) without a GPU: the numpy restatement of the fold order
(tests/reduce_ref.py) against the literal per-pixel definition, the exports and prototypes in every binding, the slab rule's
mirror, null handles and bad factors, and the driver's ``--hip-image-reduce`` option."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import reduce_ref
from tests.children import ROOT

SYMBOLS = ("gs_field_reduced_shape", "gs_field_download_reduced", "gs_field_download_reduced_async",
           "gs_field_colormap_reduced")
FACTORS = (1, 2, 3, 4, 7, 64)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("shape", [(37, 53), (36, 56), (5, 3), (1, 1), (64, 128)])
def test_restatement_matches_the_literal_definition(shape, f):
    a = reduce_ref.special_plane(shape, seed=shape[0] * 100 + f)
    got, want = reduce_ref.reduce(a, f), reduce_ref.literal(a, f)
    assert got.shape == want.shape == reduce_ref.shape(shape[0], shape[1], f)
    assert got.dtype == np.float32
    if f == 1:
        # the plain call, not the fold (which would turn a cell of -0.0 into +0.0 + -0.0 = +0.0): the input's bits
        assert np.array_equal(bits(got), bits(a))
        want = np.where(a == 0, np.float32(0.0), a)
        assert reduce_ref.same_bits(reduce_ref.literal(a, 1), want)
        return
    assert reduce_ref.same_bits(got, want), (shape, f)
    if shape[0] * shape[1] >= 64:
        assert np.isnan(a).any() and np.isinf(a).any()            # the special values are really there ...
        if f > 1:
            assert np.isnan(got).any()                            # ... and propagate


def test_special_values_by_hand():
    sub, tiny = np.float32(3.0e-41), np.float32(1.0e-45)
    a = np.array([[-0.0, -0.0, sub, sub, np.nan, 1.0],
                  [-0.0, -0.0, sub, sub, 2.0, 3.0],
                  [tiny, 0.0, np.inf, 1.0, np.inf, 5.0],
                  [0.0, 0.0, 2.0, 3.0, -np.inf, 7.0]], np.float32)
    got = reduce_ref.reduce(a, 2)
    assert got.shape == (2, 3)
    assert bits(got)[0, 0] == 0                                   # a block of -0.0: +0.0 + -0.0 = +0.0
    assert bits(got)[0, 1] == bits(np.array([sub]))[0]            # the mean of four equal sub-normals is that sub-normal
    assert np.isnan(got[0, 2])                                    # NaN propagates
    assert got[1, 0] == 0.0 and bits(got)[1, 0] == 0              # 1.4e-45 / 4 = 3.5e-46, below half the smallest sub-normal: +0.0
    assert got[1, 1] == np.inf
    assert np.isnan(got[1, 2])                                    # +inf + -inf
    # edge blocks hold the cells that exist: 5 columns at f = 4 -> a last pixel of one column
    b = np.arange(15, dtype=np.float32).reshape(3, 5)
    r = reduce_ref.reduce(b, 4)
    assert r.shape == (1, 2) and r[0, 1] == np.float32((4 + 9 + 14) / 3) and r[0, 0] == np.float32(np.mean(b[:, :4], dtype=np.float64))
    # a plane smaller than one block
    assert reduce_ref.reduce(b, 64).shape == (1, 1)
    assert reduce_ref.same_bits(reduce_ref.reduce(b, 64), reduce_ref.literal(b, 64))


def test_the_fold_order_is_observable():
    """Cells of widely differing magnitude: folding a row's cells in descending column order changes a bit, and the
    restatement (held to the literal loop above) takes the ascending one."""
    a = np.array([[1.0, 2.0 ** -53, 2.0 ** -53, 0.0]], np.float32)
    up = reduce_ref.reduce(a, 4)                                  # (1 + 2^-53) + 2^-53: both ties round to even, 1.0
    assert up[0, 0] == np.float32(0.25) and reduce_ref.same_bits(up, reduce_ref.literal(a, 4))
    # (descending, (2^-53 + 2^-53) + 1 = 1 + 2^-52 in f64, is the same f32.)  A case whose difference survives the rounding
    # to f32: ascending, row 1 is (2^80 - 2^80) + 1 = 1; descending, (1 - 2^80) + 2^80 = 0
    c = np.array([[2.0 ** 29, 1.0, 1.0, -(2.0 ** 29)], [2.0 ** 80, -(2.0 ** 80), 1.0, 0.0],
                  [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]], np.float32)
    up, down = reduce_ref.reduce(c, 4), reduce_ref.reduce(c, 4, reverse_columns=True)
    assert reduce_ref.same_bits(up, reduce_ref.literal(c, 4))
    assert up[0, 0] == np.float32(3.0 / 16.0) and down[0, 0] == np.float32(2.0 / 16.0)
    assert bits(up)[0, 0] != bits(down)[0, 0], (up, down)
    # ... and on the planes the tests use (pairs of +-2^80 among cells of order 1) many pixels differ
    d = reduce_ref.special_plane((64, 128), 5)
    d[~np.isfinite(d)] = 1.0
    up, down = reduce_ref.reduce(d, 7), reduce_ref.reduce(d, 7, reverse_columns=True)
    assert np.count_nonzero(bits(up) != bits(down)) > 10


@pytest.mark.parametrize("shape", [(37, 53), (1, 9)])
def test_factor_one_returns_the_input_bits(shape):
    a = reduce_ref.special_plane(shape, 3)
    got = reduce_ref.reduce(a, 1)
    assert got is not a and np.array_equal(bits(got), bits(a))
    assert np.signbit(got[a == 0]).any()                          # cells of -0.0 included


def test_symbols_in_every_binding(built):
    from grayscott_amd import capi

    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = capi.load()
    ffi = open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    for name in SYMBOLS:
        assert name in capi.EXPORTS, name
        assert re.search(r"\bint32_t %s\(" % name, code), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype is ctypes.c_int32 and getattr(lib, name).argtypes, name
        assert "pub fn %s(" % name in ffi, name
        assert "%s(" % name in hpp, name
    assert lib.gs_abi_version() == 4
    assert "#define GS_ABI_VERSION 4" in header
    # the definition is in the header, word for word checkable
    for phrase in ("ascending column order", "ascending row order", "(float)(block sum / (double)count)",
                   "anchored at GLOBAL row 0 and column 0"):
        assert phrase in header, phrase
    assert len(lib.gs_field_download_reduced.argtypes) == 4 and len(lib.gs_field_colormap_reduced.argtypes) == 7
    assert len(lib.gs_field_reduced_shape.argtypes) == 6


def test_null_handles_are_refused_without_a_device(built):
    """The calls need a field, and a field needs a device: here only the refusals can be reached.  The arithmetic of
    gs_field_reduced_shape and its UNSUPPORTED verdict are held to reduce_ref.slab_rule / local_rows by the GPU tests."""
    from grayscott_amd import capi

    lib = capi.load()
    r = ctypes.c_uint64(7)
    assert lib.gs_field_reduced_shape(None, 2, ctypes.byref(r), None, None, None) == capi.GS_ERR_INVALID
    assert r.value == 7
    assert lib.gs_field_download_reduced(None, None, 2, None) == capi.GS_ERR_INVALID
    assert lib.gs_field_download_reduced_async(None, None, 2, None) == capi.GS_ERR_INVALID
    assert lib.gs_field_colormap_reduced(None, None, 2, 2.0, None, 256, None) == capi.GS_ERR_INVALID


def test_slab_rule_mirror():
    # the split is k * rows / S: 1080 rows over 2 slabs begin at 0 and 540
    assert reduce_ref.slab_starts(1080, 2) == [0, 540] and reduce_ref.slab_starts(301, 3) == [0, 100, 200]
    assert reduce_ref.slab_rule(1080, 2, 4) and reduce_ref.slab_rule(1080, 2, 5) and not reduce_ref.slab_rule(1080, 2, 8)
    assert reduce_ref.slab_rule(1080, 3, 8) and not reduce_ref.slab_rule(1080, 3, 16)        # 0, 360, 720
    assert reduce_ref.slab_rule(301, 3, 4) and reduce_ref.slab_rule(301, 3, 5) and not reduce_ref.slab_rule(301, 3, 3)
    assert all(reduce_ref.slab_rule(r, 1, f) for r in (1, 16, 301) for f in (1, 2, 64))     # one slab: always
    assert all(reduce_ref.slab_rule(r, s, 1) for r in (16, 301, 1080) for s in (1, 2, 3))   # factor 1: always
    # a process's output rows: [row0 / f, ceil(row1 / f)); together they tile the image
    for rows, slabs, f in ((1080, 2, 4), (301, 3, 4), (2048, 2, 64), (16, 2, 8), (1080, 3, 8)):
        assert reduce_ref.slab_rule(rows, slabs, f)
        edges = [reduce_ref.local_rows(rows, slabs, k, 1, f) for k in range(slabs)]
        assert edges[0][0] == 0 and edges[-1][1] == reduce_ref.shape(rows, 1, f)[0]
        assert all(edges[k][1] == edges[k + 1][0] for k in range(slabs - 1)), edges
    assert reduce_ref.local_rows(301, 3, 1, 2, 4) == (25, 76)


def test_driver_option():
    from grayscott_amd import simulate

    args = simulate.parse([])
    assert args.hip_image_reduce == 1 and simulate.image_shape(args) == (1080, 1920)
    args = simulate.parse(["-r", "2048", "-c", "4096", "-n", "4", "--hip-image-reduce", "8"])
    assert args.hip_image_reduce == 8 and simulate.image_shape(args) == (256, 512)
    args = simulate.parse(["-r", "301", "-c", "517", "--hip-image-reduce", "64"])
    assert simulate.image_shape(args) == (5, 9)
    for bad in ("0", "65", "-2", "two"):
        with pytest.raises(SystemExit):
            simulate.parse(["--hip-image-reduce", bad])
    # the option does not reach the context's options
    assert not hasattr(simulate.backend_args(args), "image_reduce")
