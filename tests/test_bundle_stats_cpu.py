"""Bundle statistics (gs_members_bundle_stats) without a GPU: the numpy restatement (tests/bundle_stats_ref.py) against the
literal per-cell, per-member loop, the mean against numpy's within a derived bound, the declaration in every binding, the
refusals that need no device, the sweep's flags and its .npz writer."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import bundle_stats_ref as ref
from tests import time_stats_ref as tref
from tests.children import ROOT

NAME = "gs_members_bundle_stats"


def tiny_members(shape, span, seed, threshold):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((span,) + shape) * 0.3 + threshold).astype(np.float32)
    flat = x.reshape(span, -1)
    # every special value somewhere, in the first, a middle and the last member; a -0 / +0 cell in both orders
    for k, value in enumerate(ref.SPECIALS):
        flat[(0, span // 2, span - 1)[k % 3], (k * 5 + seed) % flat.shape[1]] = value
    flat[:, -1] = np.float32(0.0)
    flat[0 if seed % 2 else span - 1, -1] = np.float32(-0.0)
    flat[span // 2, 0] = np.float32(threshold)
    return x


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (5, 7), (6, 9)])
@pytest.mark.parametrize("span", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("above", [True, False])
def test_restatement_matches_the_literal_loop(shape, span, above):
    members = tiny_members(shape, span, span + shape[1], 0.25)
    got, want = ref.bundle(members, 0.25, above), ref.literal(members, 0.25, above)
    assert sorted(got) == sorted(want) == sorted(ref.RESULTS)
    for name in ref.RESULTS:
        assert ref.same_bits(got[name], want[name]), (name, ref.describe(got[name], want[name]))
    # without a threshold there is no occupancy, and the others do not change
    bare = ref.bundle(members)
    assert sorted(bare) == ["max", "mean", "min", "variance"]
    assert all(ref.same_bits(bare[name], got[name]) for name in bare)


def test_the_planted_values_are_there():
    every = np.stack([tiny_members((6, 9), 5, seed, 0.25) for seed in range(4)])
    assert np.isnan(every).any() and np.isposinf(every).any() and np.isneginf(every).any()
    assert ((every == 0) & np.signbit(every)).any() and ((every == 0) & ~np.signbit(every)).any()
    tiny = np.abs(every[np.isfinite(every) & (every != 0)])
    assert (tiny < np.float32(1.1754944e-38)).any()                 # sub-normal values
    planes = ref.plant(np.zeros((6, 5, 7), np.float32) + np.float32(0.1), 3, 1, 0.25)
    for b in range(2):
        for m in (3 * b, 3 * b + 1, 3 * b + 2):                      # the first, the middle and the last member carry the extremes
            assert (planes[m] == np.float32(7.0 + b)).any() and (planes[m] == np.float32(-7.0 - b)).any()


def test_special_cases():
    f = lambda *rows: np.array(rows, np.float32).reshape(len(rows), 1, -1)
    nan, inf = np.nan, np.inf
    r = ref.bundle(f((nan, 0.0, 1e-45, 0.5), (1.0, -0.0, -1e-45, 0.75)), 0.5, True)
    # a NaN never replaces an extreme and is never set, but it stays in the sums
    assert r["min"][0, 0] == 1.0 and r["max"][0, 0] == 1.0 and np.isnan(r["mean"][0, 0]) and np.isnan(r["variance"][0, 0])
    assert r["occupancy"][0, 0] == 0.5
    # a zero never replaces a zero of the other sign: the first one met stays
    assert not np.signbit(r["min"][0, 1]) and not np.signbit(r["max"][0, 1])
    back = ref.bundle(f((-0.0,), (0.0,)))
    assert np.signbit(back["min"][0, 0]) and np.signbit(back["max"][0, 0])
    # sub-normal values count as the values they are
    assert r["min"][0, 2] == np.float32(-1e-45) and r["max"][0, 2] == np.float32(1e-45) and r["mean"][0, 2] == 0.0
    # a value equal to the threshold is not set
    assert r["occupancy"][0, 3] == 0.5
    # +inf and -inf: mean and variance turn NaN, the extremes take them
    blown = ref.bundle(f((inf,), (-inf,)))
    assert np.isnan(blown["mean"][0, 0]) and np.isnan(blown["variance"][0, 0])
    assert blown["min"][0, 0] == -inf and blown["max"][0, 0] == inf
    # a variance that rounds below zero is +0.0
    flat = ref.bundle(f((0.1,), (0.1,), (0.1,)))
    assert flat["variance"][0, 0] >= 0 and not np.signbit(flat["variance"][0, 0])
    # span 1: the mean is the member, the variance is +0.0
    one = ref.bundle(f((0.3, -2.5)))
    assert one["mean"].tobytes() == f((0.3, -2.5))[0].tobytes() and not one["variance"].any()


def test_the_restatement_is_the_time_statistics_over_members():
    """Member j in the place of sample j: the restated time statistics give the same bits."""
    members = tiny_members((5, 7), 5, 2, 0.25)
    acc = tref.Accumulators((5, 7), tref.ALL, 0.25, False)
    for j, x in enumerate(members):
        acc.accumulate(x, j)
    got = ref.bundle(members, 0.25, False)
    for name in ref.RESULTS:
        assert ref.same_bits(got[name], acc.result(name)), name


@pytest.mark.parametrize("span", [1, 2, 3, 7, 33])
def test_mean_against_numpy_within_a_derived_bound(span):
    """Bound: with u = 2^-53, a sequential f64 sum of n terms is within (n - 1) u S of the exact one, S the sum of the
    magnitudes (first order; doubled to be safe); numpy's own f64 mean of the same terms is within the same bound, whatever its
    order.  The f32 values are exact in f64.  Then one division (u |m|) and one rounding to f32 (2^-24 |m|, or half the
    smallest sub-normal), of each side."""
    rng = np.random.default_rng(span)
    x = (rng.standard_normal((span, 6, 9)) * np.float32(10.0) ** rng.integers(-3, 4, (span, 6, 9))).astype(np.float32)
    got = ref.bundle(x)["mean"].astype(np.float64)
    want = x.astype(np.float64).mean(axis=0)
    S = np.abs(x.astype(np.float64)).sum(axis=0) / span
    u = 2.0 ** -53
    bound = 2 * (2 * (span - 1) * u * S) + 2 * u * np.abs(want) + 2.0 ** -24 * np.abs(want) + 2.0 ** -150
    assert np.all(np.abs(got - want) <= bound), float(np.max(np.abs(got - want) - bound))


CTYPES_OF = {"gs_ctx *": ctypes.c_void_p, "gs_ensemble *": ctypes.c_void_p, "uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32,
             "const int32_t *": ctypes.POINTER(ctypes.c_int32), "const float *": ctypes.POINTER(ctypes.c_float),
             "gs_ensemble *const *": ctypes.POINTER(ctypes.c_void_p)}
RUST_OF = {"gs_ctx *": "*mut gs_ctx", "gs_ensemble *": "*mut gs_ensemble", "uint64_t": "u64", "int32_t": "i32",
           "const int32_t *": "*const i32", "const float *": "*const f32", "gs_ensemble *const *": "*const *mut gs_ensemble"}


def header_parameters():
    """[(C type, name)] of the declaration in include/gs_hip.h, arrays as the pointers they are."""
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    m = re.search(r"^int32_t %s\(([^;]*)\);" % NAME, header, re.M)
    assert m, "not declared"
    out = []
    for p in re.sub(r"\s+", " ", m.group(1)).split(","):
        ctype, name = re.match(r"\s*(.*?)\s*(\w+)(\[2\])?$", p).group(1, 2)
        if p.strip().endswith("[2]"):
            ctype += " *"
        out.append((ctype, name))
    return out


def test_header_exports_ctypes_and_ffi_agree(built):
    from grayscott_amd import Ensemble, capi

    params = header_parameters()
    assert [name for _, name in params] == ["ctx", "e", "first", "count", "span", "which", "n", "thresholds", "above", "out",
                                            "out_first"]
    assert NAME in capi.EXPORTS
    lib = capi.load()
    assert lib.gs_abi_version() == 4
    fn = getattr(lib, NAME)
    assert fn.restype is ctypes.c_int32
    assert list(fn.argtypes) == [CTYPES_OF[t] for t, _ in params], [t for t, _ in params]
    ffi = open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    m = re.search(r"pub fn %s\(([^;]*)\) -> i32;" % NAME, ffi)
    assert m, "not declared in ffi.rs"
    rust = [tuple(x.strip() for x in p.split(":")) for p in m.group(1).split(",") if p.strip()]
    assert rust == [(name, RUST_OF[t]) for t, name in params]
    hpp = open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    assert NAME + "(" in hpp and "std::vector<Ensemble> bundle_stats(std::size_t span" in hpp
    # the header's text: the contract's words
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    text = header[header.index("/* Bundle statistics"):header.index("int32_t " + NAME)]
    for word in ("ascending", "never split", "sub-normal", "GS_TSTAT_ARRIVAL", "gs_members_copy", "newest slot", "count == 0",
                 "GS_ERR_UNSUPPORTED", "Not done", "bit for bit", "lone Species"):
        assert word in text, word
    assert Ensemble.BUNDLE_RESULTS == {name: getattr(capi, "GS_TSTAT_" + name.upper()) for name in ref.RESULTS} == ref.CODES


def test_refusals_that_need_no_device(built):
    from grayscott_amd import capi

    lib = capi.load()
    which = (ctypes.c_int32 * 2)(0, 1)
    out = (ctypes.c_void_p * 2)(None, None)
    t, a = (ctypes.c_float * 2)(0.5, 0.25), (ctypes.c_int32 * 2)(0, 1)
    assert lib.gs_members_bundle_stats(None, None, 0, 4, 2, which, 2, t, a, out, 0) == capi.GS_ERR_INVALID
    assert b"null" in lib.gs_last_error()
    assert lib.gs_members_bundle_stats(None, None, 0, 0, 0, None, 0, None, None, None, 0) == capi.GS_ERR_INVALID


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_without_a_device_bundle_stats_fail_loudly(built):
    from grayscott_amd import GsError, Parameters, Simulation, capi

    with pytest.raises(GsError) as e:
        Simulation.new(Parameters()).make_ensemble((8, 16), [Parameters()] * 4).bundle_stats(2)
    assert e.value.code == capi.GS_ERR_NO_DEVICE


BASE = ["--feed", "0.01:0.02:2", "--kill", "0.05:0.06:2"]


def test_sweep_bundle_flags():
    from grayscott_amd import sweep

    a = sweep.parse(BASE + ["-s", "10", "-o", "out/run.h5"])
    assert a.bundle_stats is False and a.bundle_threshold_v is None
    b = sweep.parse(BASE + ["--noise", "0.01", "--realisations", "4", "--bundle-stats", "-o", "out/run.h5"])
    assert b.bundle_stats is True and b.bundle_threshold_v is None and b.realisations == 4
    c = sweep.parse(BASE + ["--noise", "0.01:0.02", "--realisations", "4", "--bundle-stats", "--bundle-threshold-v", "0.25",
                            "--no-fields"])
    assert c.bundle_threshold_v == 0.25 and c.no_fields
    assert sweep.parse(BASE + ["--bundle-stats"]).realisations == 1           # a span of one member is allowed
    for bad in (["--bundle-threshold-v", "0.25"], ["--bundle-stats", "--bundle-threshold-v", "nan"],
                ["--bundle-stats", "--bundle-threshold-v", "x"], ["--bundle-stats", "--realisations", "4"]):
        with pytest.raises(SystemExit):
            sweep.parse(BASE + bad)
    assert sweep.bundles_path("out/run.h5") == os.path.join("out", "run.bundles.npz")
    assert sweep.bundle_results(None) == ("mean", "variance", "min", "max")
    assert sweep.bundle_results(0.25) == ("mean", "variance", "min", "max", "occupancy")
    # the points of the bundles are every --realisations-th member, in members() order
    points = sweep.members(b)[::4]
    assert [(f, k) for _, f, k in points] == [(0.01, 0.05), (0.02, 0.05), (0.01, 0.06), (0.02, 0.06)]
    assert [i for i, _, _ in points] == [0, 4, 8, 12]


def test_npz_writer(tmp_path):
    from grayscott_amd import sweep

    order = ("mean", "variance", "min", "max", "occupancy")
    results = {name: name for name in order}
    view = lambda name, species: np.full((4, 3, 5), order.index(name) + (10 if species == "u" else 0), np.float32)
    for threshold in (None, 0.25):
        path = str(tmp_path / f"a{threshold}.bundles.npz")
        sweep.write_bundles(path, results, threshold, [0.01, 0.02, 0.01, 0.02], [0.05, 0.05, 0.06, 0.06], 4, view)
        with np.load(path) as z:
            want = ["mean_u", "mean_v", "variance_u", "variance_v", "min_v", "max_v", "feed", "kill", "span"]
            assert sorted(z.files) == sorted(want + (["occupancy_v"] if threshold is not None else []))
            assert z["mean_u"].shape == (4, 3, 5) and z["mean_u"].dtype == np.float32 and z["mean_u"][0, 0, 0] == 10
            assert z["variance_v"][0, 0, 0] == 1 and z["max_v"][0, 0, 0] == 3 and int(z["span"]) == 4
            assert list(z["feed"]) == [0.01, 0.02, 0.01, 0.02] and list(z["kill"]) == [0.05, 0.05, 0.06, 0.06]
            if threshold is not None:
                assert z["occupancy_v"][0, 0, 0] == 4
