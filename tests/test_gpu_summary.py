"""Summaries on the device (gs_fields_summarize, gs_members_summarize) against the numpy restatement of their fold order
(tests/summary_ref.py), bit for bit: sums as f64 bit patterns, min and max as values, equal counts."""
import numpy as np
import pytest

from grayscott_amd import HipArgs, Parameters, Simulation, capi
from tests import summary_ref
from tests.children import build_program, run_program
from tests.helpers import species_from_arrays, stress_fields

pytestmark = pytest.mark.gpu

RULES = {"clipped": capi.GS_BOUNDARY_CLIPPED, "zero_halo": capi.GS_BOUNDARY_ZERO_HALO,
         "periodic": capi.GS_BOUNDARY_PERIODIC, "neumann": capi.GS_BOUNDARY_NEUMANN}


def restated(species):
    in_u, in_v, _, _ = species.in_out()
    ctx = species.context()
    return summary_ref.summary(in_u.make_scalar_view(ctx)), summary_ref.summary(in_v.make_scalar_view(ctx))


def assert_same(got, want, what):
    assert summary_ref.same(got, want), f"{what}: {summary_ref.as_dict(got)} != {want}"


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (7, 13), (64, 128), (1080, 1920), (4096, 4096)])
def test_species_summary_matches_the_restatement(built, rule, shape):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], boundary=RULES[rule], place_candidates=0))
    u0, v0 = stress_fields(shape, 7)
    species = species_from_arrays(sim, u0, v0)
    sim.perform_steps(species, 9)
    u, v = species.summary()
    want_u, want_v = restated(species)
    assert_same(u, want_u, "U")
    assert_same(v, want_v, "V")
    assert u.size == shape[0] * shape[1] and u.nonfinite == 0 and u.cells == u.size
    sim.context.close()


def test_species_summary_16384_squared(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], place_candidates=0))
    species = sim.make_species([16384, 16384])
    sim.perform_steps(species, 8)
    u, v = species.summary()
    want_u, want_v = restated(species)
    assert_same(u, want_u, "U")
    assert_same(v, want_v, "V")
    sim.context.close()


def test_planted_values_are_counted_and_skipped(built):
    rows, cols = 37, 1029
    rng = np.random.default_rng(3)
    u = rng.standard_normal((rows, cols)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-45, -2e-45, 1e-40, -1.1754942e-38], np.float32)
    pos = rng.choice(rows * cols, size=64, replace=False)
    u.flat[pos] = np.resize(special, 64)
    v = np.full((rows, cols), np.nan, np.float32)
    v[5, 7] = 1e-45                                     # the only finite cell: a sub-normal
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = species_from_arrays(sim, u, v)
    su, sv = species.summary()
    assert_same(su, summary_ref.summary(u), "U")
    assert su.nonfinite == int(np.count_nonzero(~np.isfinite(u))) == 24
    assert np.isfinite(su.sum) and np.isfinite(su.sum_sq)
    assert_same(sv, summary_ref.summary(v), "V")
    assert sv.nonfinite == rows * cols - 1 and sv.cells == 1
    assert sv.min == sv.max == float(np.float32(1e-45)) and sv.sum == float(np.float32(1e-45)) > 0.0
    # a plane without a finite cell
    bad = species_from_arrays(sim, np.full((rows, cols), -np.inf, np.float32), v)
    bu, _ = bad.summary()
    assert bu.nonfinite == rows * cols and bu.min == np.inf and bu.max == -np.inf
    assert summary_ref.bits(bu.sum) == 0 and summary_ref.bits(bu.sum_sq) == 0
    sim.context.close()


def test_summary_does_not_depend_on_the_slab_layout(built):
    shape = (1000, 777)
    u0, v0 = stress_fields(shape, 11)
    got = {}
    for name, args in [("1", HipArgs(devices=[0])), ("2", HipArgs(devices=[0] * 2)), ("3", HipArgs(devices=[0] * 3)),
                       ("5", HipArgs(devices=[0] * 5)), ("split2", HipArgs(devices=[0], split=2))]:
        sim = Simulation.new(Parameters(), args)
        species = species_from_arrays(sim, u0, v0)
        sim.perform_steps(species, 13)
        got[name] = species.summary()
        if name == "1":
            want = restated(species)
        sim.context.close()
    for name, (u, v) in got.items():
        assert_same(u, want[0], f"U, {name} slabs")
        assert_same(v, want[1], f"V, {name} slabs")


def test_summary_right_after_an_unsynchronised_window_call(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = sim.make_species([1080, 1920])
    sim.perform_steps(species, 64)           # tuned and settled
    sim.prepare_steps(species, 64)           # enqueued only
    u, v = species.summary()
    name, _ = sim.context.info()
    assert "window" in name, name
    want_u, want_v = restated(species)
    assert_same(u, want_u, "U")
    assert_same(v, want_v, "V")
    sim.context.close()


@pytest.mark.parametrize("shape", [(1080, 1920), (200, 333)])
def test_summaries_have_no_side_effects(built, shape):
    u0, v0 = stress_fields(shape, 5)
    planes = []
    for summarize in (False, True):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
        species = species_from_arrays(sim, u0, v0)
        for _ in range(3):
            sim.prepare_steps(species, 40)
            if summarize:
                species.summary()
                sim.context.sync()
                before = (sim.context.stats(), sim.context.info())
                species.summary()
                species.u.in_out()[0].summary(sim.context)
                assert (sim.context.stats(), sim.context.info()) == before
        sim.context.sync()
        in_u, in_v, _, _ = species.in_out()
        planes.append((in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)))
        sim.context.close()
    assert planes[0][0].tobytes() == planes[1][0].tobytes()
    assert planes[0][1].tobytes() == planes[1][1].tobytes()


@pytest.mark.parametrize("rule", ["clipped", "periodic", "neumann"])
@pytest.mark.parametrize("shape", [(32, 64), (45, 61), (100, 130)])  # resident form, then tile forms (61, 130: cols % 4 != 0)
def test_ensemble_members_equal_lone_species(built, rule, shape):
    members = 7
    params = [Parameters(feed_rate=0.01 + 0.006 * i, kill_rate=0.05 + 0.002 * (members - 1 - i)) for i in range(members)]
    sim = Simulation.new(params[0], HipArgs(devices=[0], boundary=RULES[rule]))
    ens = sim.make_ensemble(shape, params)
    rng = np.random.default_rng(1)
    ens.upload(rng.random((members,) + shape, dtype=np.float32),
               (rng.random((members,) + shape, dtype=np.float32) * np.float32(0.5)).astype(np.float32))
    ens.perform_steps(23)
    allsum = ens.summaries()
    assert allsum.shape == (members, 2)
    part = ens.summaries(2, 3)
    assert part.tobytes() == allsum[2:5].tobytes()
    u, v = ens.u_views(), ens.result_views()
    for i in range(members):
        lone = Simulation.new(params[i], HipArgs(devices=[0], boundary=RULES[rule]))
        species = species_from_arrays(lone, u[i], v[i])
        su, sv = species.summary()
        assert_same(allsum[i, 0], summary_ref.as_dict(su), f"member {i} U")
        assert_same(allsum[i, 1], summary_ref.as_dict(sv), f"member {i} V")
        assert_same(su, summary_ref.summary(u[i]), f"member {i} U restated")
        lone.context.close()
    with pytest.raises(capi.GsError) as e:
        ens.summaries(members - 1, 2)
    assert e.value.code == capi.GS_ERR_INVALID
    ens.destroy()
    sim.context.close()


def test_sweep_records_summaries_without_changing_the_fields(built, tmp_path):
    from grayscott_amd import hdf5_min, sweep

    base = ["--feed", "0.02:0.05:3", "--kill", "0.05:0.062:2", "-r", "48", "-c", "72", "-s", "30"]
    sweep.main(base + ["-o", str(tmp_path / "plain.h5")])
    sweep.main(base + ["--summary-every", "7", "-o", str(tmp_path / "summ.h5")])
    sweep.main(base + ["--summary-every", "30", "--no-fields", "-o", str(tmp_path / "nof.h5")])
    assert (tmp_path / "plain.h5").read_bytes() == (tmp_path / "summ.h5").read_bytes()
    assert not (tmp_path / "plain.summary.npz").exists() and not (tmp_path / "nof.h5").exists()
    assert (tmp_path / "nof.json").exists()
    z = np.load(tmp_path / "summ.summary.npz")
    assert list(z["steps"]) == [7, 14, 21, 28, 30]
    for name in summary_ref.FIELDS:
        assert z[name].shape == (6, 5, 2), name
    v = hdf5_min.read(str(tmp_path / "summ.h5"))
    for i in range(6):
        want = summary_ref.summary(v[i])
        got = {name: z[name][i, -1, 1] for name in summary_ref.FIELDS}
        got = {k: (int(x) if k == "nonfinite" else float(x)) for k, x in got.items()}
        assert summary_ref.same(got, want), i
    z2 = np.load(tmp_path / "nof.summary.npz")
    assert list(z2["steps"]) == [30]
    for name in summary_ref.FIELDS:
        assert z2[name][:, -1].tobytes() == z[name][:, -1].tobytes(), name


def test_cpp_mirror_summaries(built, tmp_path):
    exe = build_program("summary_mirror", tmp_path)
    members, rows, cols = 4, 72, 200
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(members), str(rows), str(cols), "31", str(out)])
    assert r.returncode == 0, r.stderr
    from grayscott_amd.simulation import SUMMARY_DTYPE

    raw = out.read_bytes()
    rec = np.frombuffer(raw[:32 * (2 + 2 * members)], SUMMARY_DTYPE)
    v = np.frombuffer(raw[32 * (2 + 2 * members):], np.float32).reshape(rows, cols)
    assert summary_ref.same(rec[1], summary_ref.summary(v))
    for i in range(members):
        assert rec[2 + 2 * i].tobytes() == rec[0].tobytes() and rec[3 + 2 * i].tobytes() == rec[1].tobytes(), i
