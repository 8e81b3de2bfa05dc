"""Time statistics (gs_time_stats_*, gs_members_time_stats_*) without a GPU: the numpy restatement of the rule
(tests/time_stats_ref.py) against the literal per-cell loop, the rule's special cases, the declarations in every binding,
the exports, null handles and bad arguments, the drivers' flags and the .npz writers."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import time_stats_ref as ref
from tests.children import ROOT

SYMBOLS = ("gs_time_stats_create", "gs_time_stats_destroy", "gs_time_stats_reset", "gs_time_stats_accumulate",
           "gs_time_stats_samples", "gs_time_stats_result", "gs_time_stats_download", "gs_members_time_stats_create",
           "gs_members_time_stats_accumulate", "gs_members_time_stats_result")


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (5, 17), (2, 40)])
@pytest.mark.parametrize("above", [True, False])
@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_matches_the_literal_loop(shape, above, seed):
    threshold = 0.25
    samples = ref.sample_planes(shape, seed, threshold)
    acc = ref.Accumulators(shape, ref.ALL, threshold, above)
    for x, stamp in zip(samples, ref.STAMPS):
        acc.accumulate(x, stamp)
    want = ref.literal(samples, ref.STAMPS, threshold, above)
    assert acc.samples == 6
    for name in ref.RAW_GROUP:
        assert ref.same_bits(acc.raw(name), want[name]), (name, ref.describe(acc.raw(name), want[name]))
    for name in ref.RESULT_GROUPS:
        assert ref.same_bits(acc.result(name), want["result:" + name]), (name, ref.describe(acc.result(name), want["result:" + name]))


def test_the_sample_planes_hold_what_they_promise():
    samples = ref.sample_planes((37, 301), 3, 0.25)
    every = np.stack(samples)
    assert np.isnan(every).any() and np.isposinf(every).any() and np.isneginf(every).any()
    assert (every == np.float32(0.25)).any()
    assert ((every == 0) & np.signbit(every)).any() and ((every == 0) & ~np.signbit(every)).any()
    tiny = np.abs(every[np.isfinite(every) & (every != 0)])
    assert (tiny < np.float32(1.1754944e-38)).any()                 # sub-normal samples


def f32(*values):
    return np.array([values], np.float32)


def test_restatement_special_cases():
    nan, inf = np.nan, np.inf
    acc = ref.Accumulators((1, 4), ref.ALL, 0.5, True)
    acc.accumulate(f32(nan, 0.0, 1e-45, 0.5), 7)
    acc.accumulate(f32(1.0, -0.0, -1e-45, 0.75), 9)
    # a NaN sample never replaces an extreme and is never set, but it stays in the sums
    assert acc.min[0, 0] == 1.0 and acc.max[0, 0] == 1.0 and np.isnan(acc.sum[0, 0]) and np.isnan(acc.squares[0, 0])
    assert acc.set_count[0, 0] == 1 and acc.first_stamp[0, 0] == 9
    # a zero never replaces an extreme zero of the other sign
    assert not np.signbit(acc.min[0, 1]) and not np.signbit(acc.max[0, 1])
    # sub-normal samples count as the values they are; their squares are exact in f64
    assert acc.min[0, 2] == np.float32(-1e-45) and acc.max[0, 2] == np.float32(1e-45) and acc.squares[0, 2] == 2.0 ** -297
    # a sample equal to the threshold is not set
    assert acc.set_count[0, 3] == 1 and acc.first_stamp[0, 3] == 9
    assert acc.result("arrival")[0, 3] == 9.0 and acc.result("occupancy")[0, 3] == 0.5
    # never set: arrival -1; the largest stamp rounds to f32 like any u32
    never = ref.Accumulators((1, 2), ref.ALL, 0.5, False)
    never.accumulate(f32(0.75, 0.25), 4000000000)
    assert never.result("arrival")[0, 0] == -1.0 and never.first_stamp[0, 0] == ref.NEVER
    assert never.result("arrival")[0, 1] == np.float32(4000000000) and never.first_stamp[0, 1] == 4000000000
    # inf and -inf: the sum turns NaN, the variance stays NaN, the extremes take them
    blown = ref.Accumulators((1, 1))
    for x in (inf, -inf):
        blown.accumulate(f32(x), 1)
    assert np.isnan(blown.result("mean")[0, 0]) and np.isnan(blown.result("variance")[0, 0])
    assert blown.min[0, 0] == -inf and blown.max[0, 0] == inf
    # a variance that rounds below zero is +0.0
    flat = ref.Accumulators((1, 1))
    for _ in range(3):
        flat.accumulate(f32(0.1), 1)
    assert flat.result("variance")[0, 0] >= 0 and not np.signbit(flat.result("variance")[0, 0])
    assert ref.same_bits(np.array([np.nan], np.float32), -np.array([np.nan], np.float32))
    assert not ref.same_bits(np.array([0.0], np.float32), np.array([-0.0], np.float32))


def test_every_symbol_is_declared_in_every_binding():
    from grayscott_amd import capi

    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r"^int32_t %s\(" % name, header, re.M), name
        assert name in capi.EXPORTS, name
        assert f"pub fn {name}(" in ffi, name
        assert name + "(" in hpp, name
    assert "typedef struct gs_time_stats gs_time_stats;" in header and "pub struct gs_time_stats {" in ffi
    for name, value in (("GS_TSTAT_SUM", 1), ("GS_TSTAT_SQUARES", 2), ("GS_TSTAT_EXTREMES", 4), ("GS_TSTAT_CROSSINGS", 8)):
        assert f"#define {name} {value}u" in header and f"pub const {name}: u32 = {value};" in ffi
        assert getattr(capi, name) == value == getattr(ref, name[len("GS_TSTAT_"):])
    enums = header[header.index("enum { GS_TSTAT_MEAN"):header.index("typedef struct gs_time_stats")]
    for name, value in re.findall(r"(GS_TSTAT_\w+) = (\d+)", enums):
        assert getattr(capi, name) == int(value) and f"pub const {name}: i32 = {value};" in ffi, name
    assert "class TimeStats {" in hpp


def test_symbols_are_exported_bound_and_refuse_null_handles(built):
    from grayscott_amd import capi

    lib = capi.load()
    assert lib.gs_abi_version() == 4
    for name in SYMBOLS:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int32
    INV = capi.GS_ERR_INVALID
    h = ctypes.c_void_p()
    fields = (ctypes.c_void_p * 2)(None, None)
    t, a = (ctypes.c_float * 2)(0.25, 0.25), (ctypes.c_int32 * 2)(1, 1)
    n = ctypes.c_uint64(77)
    buf = (ctypes.c_float * 4)()
    assert lib.gs_time_stats_create(None, ctypes.byref(h), 8, 8, 2, 15, t, a) == INV and not h.value
    assert b"null" in lib.gs_last_error()
    assert lib.gs_time_stats_create(None, None, 8, 8, 2, 15, t, a) == INV
    assert lib.gs_members_time_stats_create(None, ctypes.byref(h), None, 0, 1, 15, t, a) == INV and not h.value
    assert lib.gs_time_stats_destroy(None, None) == capi.GS_OK            # (as gs_field_destroy: nothing to free)
    assert lib.gs_time_stats_reset(None, None) == INV
    assert lib.gs_time_stats_accumulate(None, None, fields, 2, 1) == INV
    assert lib.gs_time_stats_accumulate(None, None, None, 2, 1) == INV
    assert lib.gs_members_time_stats_accumulate(None, None, None, 1) == INV
    assert lib.gs_time_stats_samples(None, ctypes.byref(n)) == INV and n.value == 77
    assert lib.gs_time_stats_samples(None, None) == INV
    assert lib.gs_time_stats_result(None, None, 0, 0, None) == INV
    assert lib.gs_members_time_stats_result(None, None, 0, 0, buf) == INV
    assert lib.gs_members_time_stats_result(None, None, 0, 0, None) == INV
    assert lib.gs_time_stats_download(None, None, 0, 0, buf) == INV


def test_group_names():
    from grayscott_amd import TimeStats

    assert TimeStats.group_bits(("sum", "squares")) == 3 and TimeStats.group_bits("extremes") == 4
    assert TimeStats.group_bits(["crossings", "sum"]) == 9 and TimeStats.group_bits(15) == 15
    with pytest.raises(ValueError):
        TimeStats.group_bits(("sum", "cubes"))
    assert sorted(TimeStats.RAW) == sorted(ref.RAW_GROUP)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_without_a_device_time_stats_fail_loudly(built):
    from grayscott_amd import GsError, Parameters, Simulation, capi

    with pytest.raises(GsError) as e:
        Simulation.new(Parameters()).make_species((8, 16)).time_stats()
    assert e.value.code == capi.GS_ERR_NO_DEVICE


BASE = ["--feed", "0.01:0.02:2", "--kill", "0.05:0.05:1"]


def test_sweep_time_stats_flags():
    from grayscott_amd import sweep

    a = sweep.parse(BASE + ["-s", "10", "-o", "out/run.h5"])
    assert a.time_stats_every == 0 and a.time_stats_from is None and a.time_stats_threshold_v is None
    b = sweep.parse(BASE + ["--time-stats-every", "4", "-o", "out/run.h5"])
    assert b.time_stats_every == 4 and b.time_stats_from == 4
    c = sweep.parse(BASE + ["--time-stats-every", "4", "--time-stats-from", "0", "--time-stats-threshold-v", "0.25"])
    assert c.time_stats_from == 0 and c.time_stats_threshold_v == 0.25
    assert sweep.time_stats_path("out/run.h5") == os.path.join("out", "run.timestats.npz")
    for bad in (["--time-stats-from", "8"], ["--time-stats-every", "0", "--time-stats-from", "8"], ["--time-stats-every", "-1"],
                ["--time-stats-threshold-v", "0.25"], ["--time-stats-every", "4", "--time-stats-from", "-2"],
                ["--time-stats-every", "4", "--time-stats-threshold-v", "nan"]):
        with pytest.raises(SystemExit):
            sweep.parse(BASE + bad)


def test_simulate_time_stats_flags():
    from grayscott_amd import simulate

    a = simulate.parse(["-n", "2"])
    assert a.hip_time_stats_every == 0 and a.hip_time_stats_from is None and a.hip_time_stats_threshold_v is None
    b = simulate.parse(["--hip-time-stats-every", "8", "--hip-time-stats-from", "40", "--hip-time-stats-threshold-v", "0.25"])
    assert (b.hip_time_stats_every, b.hip_time_stats_from, b.hip_time_stats_threshold_v) == (8, 40, 0.25)
    assert simulate.parse(["--hip-time-stats-every", "8"]).hip_time_stats_from == 8
    for bad in (["--hip-time-stats-from", "8"], ["--hip-time-stats-every", "-3"], ["--hip-time-stats-every", "x"],
                ["--hip-time-stats-threshold-v", "0.25"], ["--hip-time-stats-every", "8", "--hip-time-stats-from", "-1"],
                ["--hip-time-stats-every", "8", "--hip-time-stats-threshold-v", "nan"]):
        with pytest.raises(SystemExit):
            simulate.parse(bad)
    assert simulate.time_stats_steps(200, 8, 40) == list(range(40, 201, 8))
    assert simulate.time_stats_steps(10, 4, 0) == [0, 4, 8] and simulate.time_stats_steps(10, 0, 0) == []
    assert simulate.time_stats_steps(3, 4, 4) == []
    assert simulate.time_stats_path("out/run.h5") == os.path.join("out", "run.timestats.npz")
    assert simulate.time_stats_path("out/run.h5", 1, 2) == os.path.join("out", "run.timestats.rank1.npz")
    assert simulate.time_stats_groups(None) == ("sum", "squares", "extremes")
    assert simulate.time_stats_groups(0.25) == ("sum", "squares", "extremes", "crossings")


class FakeStats:
    """What the writers read of a ``TimeStats``: every result method returns a plane filled with its own number."""

    ORDER = ("mean", "variance", "min", "max", "occupancy", "arrival")

    def __init__(self, shape):
        self.shape, self.asked = shape, []

    def __getattr__(self, method):
        if method not in self.ORDER:
            raise AttributeError(method)

        def plane(species):
            self.asked.append((method, species))
            return np.full(self.shape, self.ORDER.index(method) + (10 if species == "u" else 0), np.float32)
        return plane


def test_npz_writers(tmp_path):
    from grayscott_amd import simulate, sweep

    fake = FakeStats((3, 4, 5))
    planes = simulate.time_stats_planes(fake, 0.25, lambda a: a)
    assert sorted(planes) == sorted(["mean_v", "var_v", "min_v", "max_v", "mean_u", "var_u", "min_u", "max_u", "occupancy_v",
                                     "arrival_v"])
    assert planes["var_u"][0, 0, 0] == 11 and planes["arrival_v"][0, 0, 0] == 5
    assert sorted(simulate.time_stats_planes(FakeStats((2, 2)), None, lambda a: a)) == \
        sorted(["mean_v", "var_v", "min_v", "max_v", "mean_u", "var_u", "min_u", "max_u"])
    path = str(tmp_path / "a.timestats.npz")
    simulate.write_time_stats(path, 6, [3, 10], {k: v[0] for k, v in planes.items()}, {"rows": np.array([0, 4])})
    with np.load(path) as z:
        assert int(z["samples"]) == 6 and list(z["steps"]) == [3, 10] and z["mean_v"].shape == (4, 5) and list(z["rows"]) == [0, 4]
        assert z["var_v"].dtype == np.float32
    planes["var_v"][1, 2, 3] = 9.0
    for with_planes in (True, False):
        path = str(tmp_path / f"b{with_planes}.timestats.npz")
        sweep.write_time_stats(path, 6, [4, 8], planes, with_planes)
        with np.load(path) as z:
            assert z["var_v_mean"].shape == (3,) and z["var_v_mean"].dtype == np.float64
            assert list(z["var_v_max"]) == [1.0, 9.0, 1.0] and list(z["mean_v_mean"]) == [0.0, 0.0, 0.0]
            assert z["var_v_mean"][1] == (19 * 1.0 + 9.0) / 20
            assert ("max_u" in z.files) == with_planes and ("arrival_v" in z.files) == with_planes
    path = str(tmp_path / "c.timestats.npz")
    sweep.write_time_stats(path, 0, [], {}, True)                       # a run too short for a sample
    with np.load(path) as z:
        assert int(z["samples"]) == 0 and "var_v_mean" not in z.files
