"""Histograms on the device (gs_fields_histogram, gs_members_histogram) against the numpy restatement of their binning rule
(tests/hist_ref.py) on the downloaded plane: every counter equal."""
import ctypes

import numpy as np
import pytest

from grayscott_amd import HipArgs, HipConcentration, Histogram, Parameters, Simulation, capi
from grayscott_amd.simulation import histogram_fields
from tests import hist_ref
from tests.children import build_program, run_program
from tests.helpers import species_from_arrays, stress_fields

pytestmark = pytest.mark.gpu

RULES = {"clipped": capi.GS_BOUNDARY_CLIPPED, "zero_halo": capi.GS_BOUNDARY_ZERO_HALO,
         "periodic": capi.GS_BOUNDARY_PERIODIC, "neumann": capi.GS_BOUNDARY_NEUMANN}
U_RANGE, V_RANGE = (0.0, 1.0), (0.0, 0.5)


def counters(h: Histogram) -> np.ndarray:
    return np.concatenate([h.counts, np.array([h.below, h.above, h.nan], np.uint64)])


def assert_same(h: Histogram, plane: np.ndarray, rng, bins: int, what: str):
    want = hist_ref.histogram(plane, rng[0], rng[1], bins)
    got = counters(h)
    print(f"{what}: {plane.shape} bins {bins} range {rng}: in range {h.in_range}, below {h.below}, above {h.above}, "
          f"nan {h.nan}, largest bin {int(h.counts.max())}")
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert int(got.sum()) == plane.size == h.size, f"{what}: the counters sum to {int(got.sum())}, not {plane.size}"
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: counters {bad[:8]} are {got[bad[:8]]}, not {want[bad[:8]]}"


def check_species(species, bins=256, u_range=U_RANGE, v_range=V_RANGE, what=""):
    in_u, in_v, _, _ = species.in_out()
    ctx = species.context()
    hu, hv = species.histogram(bins, u_range, v_range)
    assert_same(hu, in_u.make_scalar_view(ctx), u_range, bins, what + " U")
    assert_same(hv, in_v.make_scalar_view(ctx), v_range, bins, what + " V")
    return hu, hv


# ---- planted planes ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", [1, 2, 255, 256, 1000, 4096])
@pytest.mark.parametrize("shape", [(5, 253), (3, 254), (9, 255), (4, 256), (3, 257), (2, 1023), (6, 1024), (3, 1025), (2, 1026),
                                   (2, 2049), (1, 1), (300, 1), (37, 4100)])
def test_planted_planes(built, shape, bins):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    settings = [(0.0, 1.0), (0.0, 0.5), (-2.5, 3.75), (0.1, 0.9)]
    planes = [hist_ref.planted(shape, lo, hi, bins, 10 + i) for i, (lo, hi) in enumerate(settings)]
    fields = []
    for p in planes:
        f = HipConcentration(sim.context, shape)
        f.upload(sim.context, p)
        fields.append(f)
    for n in (1, 2, 3, 4):                        # 1 to 4 fields in a call, each with its own range
        got = histogram_fields(sim.context, fields[:n], bins, settings[:n])
        assert len(got) == n
        for i in range(n):
            assert_same(got[i], planes[i], settings[i], bins, f"field {i} of {n}")
    # a plane alone through the plane's own method, with a range one more time different
    narrow = (1.0, float(np.float32(1.0) + np.float32(8 * 2.0 ** -23)))
    p = hist_ref.planted(shape, narrow[0], narrow[1], bins, 5)
    fields[0].upload(sim.context, p)
    assert_same(fields[0].histogram(sim.context, bins, narrow), p, narrow, bins, "narrow range")
    sim.context.close()


def test_refusals_that_need_handles_and_the_empty_plane(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    a, b = HipConcentration(sim.context, (8, 16)), HipConcentration(sim.context, (8, 17))
    foreign = HipConcentration(other.context, (8, 16))
    for fields in ([a, b], [a, foreign], [a] * 5):
        with pytest.raises(capi.GsError) as e:
            histogram_fields(sim.context, fields, 16, [U_RANGE] * len(fields))
        assert e.value.code == capi.GS_ERR_INVALID, fields
    for bins, rng in ((0, U_RANGE), (4097, U_RANGE), (16, (1.0, 1.0)), (16, (0.0, float("inf"))), (16, (0.0, 1e-45))):
        with pytest.raises(capi.GsError) as e:
            a.histogram(sim.context, bins, rng)
        assert e.value.code == capi.GS_ERR_INVALID, (bins, rng)
    ens = sim.make_ensemble((8, 16), Parameters(), members=3)
    for first, count in ((3, 1), (2, 2), (0, 0), (0, 4)):
        with pytest.raises(capi.GsError) as e:
            ens.histograms(first, count)
        assert e.value.code == capi.GS_ERR_INVALID, (first, count)
    theirs = other.make_ensemble((8, 16), Parameters(), members=3)
    out = np.zeros((3, 2, 19), np.uint64)
    lo, hi = (ctypes.c_float * 2)(0, 0), (ctypes.c_float * 2)(1, 1)
    assert capi.load().gs_members_histogram(sim.context.handle, theirs.handle, 0, 3, lo, hi, 16,
                                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))) == capi.GS_ERR_INVALID
    empty = HipConcentration(sim.context, (0, 16))
    h = empty.histogram(sim.context, 16, U_RANGE)
    assert h.size == 0 and int(counters(h).sum()) == 0
    for s in (sim, other):
        s.context.close()


# ---- the three distributions the kernel must survive -----------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(4096, 4096), (1080, 1920)])
@pytest.mark.parametrize("kind", ["new", "developed", "random"])
def test_distributions(built, shape, kind):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], place_candidates=0))
    if kind == "new":
        species = sim.make_species(shape)                           # one-valued: U = 1 and V = 0 outside a square
    elif kind == "developed":
        u0, v0 = stress_fields(shape, 21)
        species = species_from_arrays(sim, u0, v0)
        sim.perform_steps(species, 48)
    else:
        rng = np.random.default_rng(8)                              # spread over every bin, and a little outside
        species = species_from_arrays(sim, (rng.random(shape, dtype=np.float32) * np.float32(1.1) - np.float32(0.05)),
                                      (rng.random(shape, dtype=np.float32) * np.float32(0.55) - np.float32(0.025)))
    for bins in (256, 4096):
        hu, hv = check_species(species, bins, what=f"{kind} {shape}")
    if kind == "new":
        assert hu.counts[-1] + hu.counts[0] == hu.size and hv.counts[0] + hv.above == hv.size   # V = 1 is above [0, 0.5]
    if kind == "random":
        assert np.all(hu.counts > 0) and hu.below > 0 and hu.above > 0
    sim.context.close()


def test_species_new_16384_squared(built):
    """2^28 cells of which nearly all are one value: no 32-bit counter on the way may wrap, and the counters sum to 2^28."""
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], place_candidates=0))
    species = sim.make_species([16384, 16384])
    hu, hv = species.histogram()
    assert int(counters(hu).sum()) == 1 << 28 and int(counters(hv).sum()) == 1 << 28
    in_u, in_v, _, _ = species.in_out()
    assert_same(hu, in_u.make_scalar_view(sim.context), U_RANGE, 256, "U")
    assert_same(hv, in_v.make_scalar_view(sim.context), V_RANGE, 256, "V")
    assert int(hu.counts[255]) > 1 << 27
    sim.context.close()


# ---- any producer, any slab layout -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", sorted(RULES))
def test_the_producer_does_not_matter(built, rule):
    shape, steps = (1080, 1920), 40
    u0, v0 = stress_fields(shape, 9)
    ran = []
    for name, kernel in (("marching", capi.GS_KERNEL_TB), ("tile", capi.GS_KERNEL_TILE), ("window", capi.GS_KERNEL_WINDOW),
                         ("auto", capi.GS_KERNEL_AUTO)):
        try:
            sim = Simulation.new(Parameters(), HipArgs(devices=[0], kernel=kernel, boundary=RULES[rule]))
        except capi.GsError as e:                      # a kernel without a form for this rule
            assert e.code == capi.GS_ERR_UNSUPPORTED, e
            continue
        species = species_from_arrays(sim, u0, v0)
        try:
            sim.perform_steps(species, steps)
        except capi.GsError as e:
            assert e.code == capi.GS_ERR_UNSUPPORTED, e
            sim.context.close()
            continue
        ran.append(name)
        check_species(species, what=f"{name} ({sim.context.info()[0]}), {rule}")
        sim.context.close()
    assert {"marching", "auto"} <= set(ran), ran
    if rule in ("clipped", "zero_halo"):
        assert "window" in ran and "tile" in ran, ran


@pytest.mark.parametrize("rule", sorted(RULES))
def test_after_the_resident_kernel(built, rule):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], boundary=RULES[rule]))
    u0, v0 = stress_fields((32, 64), 2)
    species = species_from_arrays(sim, u0, v0)
    sim.perform_steps(species, 50)
    check_species(species, what=f"{sim.context.info()[0]}, {rule}")
    sim.context.close()


def test_right_after_an_unsynchronised_window_call(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = sim.make_species([1080, 1920])
    sim.perform_steps(species, 64)           # tuned and settled
    sim.prepare_steps(species, 64)           # enqueued only
    hu, hv = species.histogram()
    name, _ = sim.context.info()
    assert "window" in name, name
    in_u, in_v, _, _ = species.in_out()
    assert_same(hu, in_u.make_scalar_view(sim.context), U_RANGE, 256, "U")
    assert_same(hv, in_v.make_scalar_view(sim.context), V_RANGE, 256, "V")
    sim.context.close()


def test_histogram_does_not_depend_on_the_slab_layout(built):
    shape = (1000, 777)
    u0, v0 = stress_fields(shape, 11)
    got = {}
    for name, args in [("1", HipArgs(devices=[0])), ("2", HipArgs(devices=[0] * 2)), ("3", HipArgs(devices=[0] * 3)),
                       ("split2", HipArgs(devices=[0], split=2))]:
        sim = Simulation.new(Parameters(), args)
        species = species_from_arrays(sim, u0, v0)
        sim.perform_steps(species, 13)
        if name == "1":
            got[name] = check_species(species, 1000, what="one slab")
        else:
            got[name] = species.histogram(1000)
        sim.context.close()
    for name, (u, v) in got.items():
        assert counters(u).tobytes() == counters(got["1"][0]).tobytes(), f"U, {name} slabs"
        assert counters(v).tobytes() == counters(got["1"][1]).tobytes(), f"V, {name} slabs"


@pytest.mark.parametrize("shape", [(1080, 1920), (200, 333)])
def test_histograms_have_no_side_effects(built, shape):
    u0, v0 = stress_fields(shape, 5)
    planes, infos = [], []
    for look in (False, True):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
        species = species_from_arrays(sim, u0, v0)
        for _ in range(3):
            sim.prepare_steps(species, 40)
            if look:
                species.histogram()
                sim.context.sync()
                before = (sim.context.stats(), sim.context.info())
                species.histogram(64)
                species.u.in_out()[0].histogram(sim.context)
                assert (sim.context.stats(), sim.context.info()) == before
        sim.context.sync()
        infos.append((sim.context.stats(), sim.context.info()))
        in_u, in_v, _, _ = species.in_out()
        planes.append((in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)))
        sim.context.close()
    assert infos[0][1] == infos[1][1], infos                     # launches and the kernel's name
    for key in ("passes", "steps", "launches", "ghost_refreshes", "window_fallbacks"):
        assert infos[0][0][key] == infos[1][0][key], (key, infos)
    assert planes[0][0].tobytes() == planes[1][0].tobytes()
    assert planes[0][1].tobytes() == planes[1][1].tobytes()


# ---- ensembles -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("members,shape,check", [(512, (64, 128), [0, 1, 255, 511]), (7, (100, 130), list(range(7))),
                                                 (5, (45, 61), list(range(5)))])
def test_ensemble_members_equal_lone_species(built, members, shape, check):
    params = [Parameters(feed_rate=0.01 + 0.05 * i / members, kill_rate=0.05 + 0.015 * (members - 1 - i) / members)
              for i in range(members)]
    sim = Simulation.new(params[0], HipArgs(devices=[0]))
    ens = sim.make_ensemble(shape, params)
    rng = np.random.default_rng(1)
    ens.upload(rng.random((members,) + shape, dtype=np.float32),
               (rng.random((members,) + shape, dtype=np.float32) * np.float32(0.5)).astype(np.float32))
    ens.perform_steps(23)
    bins = 100
    allh = ens.histograms(bins=bins)
    assert allh.shape == (members, 2, bins + 3) and allh.dtype == np.uint64
    assert np.all(allh.sum(axis=2) == shape[0] * shape[1])
    part = ens.histograms(2, 3, bins=bins)
    assert part.tobytes() == allh[2:5].tobytes()
    other = ens.histograms(1, 2, bins=17, u_range=(0.2, 0.7), v_range=(-0.1, 0.3))
    u, v = ens.u_views(), ens.result_views()
    for i in (1, 2):
        assert np.array_equal(other[i - 1, 0], hist_ref.histogram(u[i], 0.2, 0.7, 17))
        assert np.array_equal(other[i - 1, 1], hist_ref.histogram(v[i], -0.1, 0.3, 17))
    for i in check:
        assert np.array_equal(allh[i, 0], hist_ref.histogram(u[i], *U_RANGE, bins)), f"member {i} U"
        assert np.array_equal(allh[i, 1], hist_ref.histogram(v[i], *V_RANGE, bins)), f"member {i} V"
        lone = Simulation.new(params[i], HipArgs(devices=[0]))
        species = species_from_arrays(lone, u[i], v[i])
        hu, hv = species.histogram(bins)
        assert np.array_equal(counters(hu), allh[i, 0]) and np.array_equal(counters(hv), allh[i, 1]), f"member {i} alone"
        lone.context.close()
    ens.destroy()
    sim.context.close()


# ---- the sweep driver and the C++ mirror -----------------------------------------------------------------------------------

def test_sweep_records_histograms_without_changing_the_fields(built, tmp_path):
    from grayscott_amd import hdf5_min, sweep

    base = ["--feed", "0.02:0.05:3", "--kill", "0.05:0.062:2", "-r", "48", "-c", "72", "-s", "30"]
    sweep.main(base + ["-o", str(tmp_path / "plain.h5")])
    sweep.main(base + ["--histogram-every", "4", "--summary-every", "4", "--hist-bins", "64", "-o", str(tmp_path / "hist.h5")])
    sweep.main(base + ["--histogram-every", "30", "--hist-bins", "64", "--no-fields", "-o", str(tmp_path / "nof.h5")])
    assert (tmp_path / "plain.h5").read_bytes() == (tmp_path / "hist.h5").read_bytes()
    assert not (tmp_path / "plain.hist.npz").exists() and not (tmp_path / "nof.h5").exists()
    assert (tmp_path / "hist.summary.npz").exists() and not (tmp_path / "nof.summary.npz").exists()
    z = np.load(tmp_path / "hist.hist.npz")
    steps = [4, 8, 12, 16, 20, 24, 28, 30]
    assert list(z["steps"]) == steps and list(np.load(tmp_path / "hist.summary.npz")["steps"]) == steps
    assert z["counts"].shape == (6, 8, 2, 64) and z["outside"].shape == (6, 8, 2, 3)
    assert z["counts"].dtype == np.uint64 and z["outside"].dtype == np.uint64
    assert list(z["lo"]) == [0.0, 0.0] and list(z["hi"]) == [1.0, 0.5]
    assert np.all(z["counts"].sum(axis=3) + z["outside"].sum(axis=3) == 48 * 72)
    v = hdf5_min.read(str(tmp_path / "hist.h5"))
    for i in range(6):
        want = hist_ref.histogram(v[i], 0.0, 0.5, 64)
        assert np.array_equal(z["counts"][i, -1, 1], want[:64]) and np.array_equal(z["outside"][i, -1, 1], want[64:]), i
    z2 = np.load(tmp_path / "nof.hist.npz")
    assert list(z2["steps"]) == [30]
    assert z2["counts"][:, -1].tobytes() == z["counts"][:, -1].tobytes()
    assert z2["outside"][:, -1].tobytes() == z["outside"][:, -1].tobytes()


def test_cpp_mirror_histograms(built, tmp_path):
    exe = build_program("histogram_mirror", tmp_path)
    members, rows, cols, bins = 4, 72, 200, 50
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(members), str(rows), str(cols), "31", str(bins), str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    n = (2 + 2 * members) * (bins + 3)
    c = np.frombuffer(raw[:8 * n], np.uint64).reshape(1 + members, 2, bins + 3)
    planes = np.frombuffer(raw[8 * n:], np.float32).reshape(2, rows, cols)
    assert np.array_equal(c[0, 0], hist_ref.histogram(planes[0], *U_RANGE, bins))
    assert np.array_equal(c[0, 1], hist_ref.histogram(planes[1], *V_RANGE, bins))
    for i in range(members):
        assert c[1 + i].tobytes() == c[0].tobytes(), i
