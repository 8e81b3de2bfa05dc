"""Noise of ensembles on the MI355X (gs_members_set_noise): member i of a noisy ensemble is bit for bit the restatement of
tests/noise_ref.py with member i's parameters, initial state, seed, sigmas and step counter -- under all four boundary
rules, in both math flavours, in the resident forms with 1, 2, 4 and 8 cells per thread and in the windowed form, over two
calls, with and without an active set; zero sigmas against the plain ensemble, the bare noise field, replay from a snapshot
plus the structs, the context's noise staying out of it, the refusals, and the sweep's --noise end to end."""
from __future__ import annotations

import ctypes
import functools
import json
import sys

import numpy as np
import pytest

import oracle
from grayscott_amd import GsError, HipArgs, Parameters, Simulation, capi, hdf5_min

from . import noise_ref as N
from .helpers import assert_bits_equal, oracle_params, species_from_arrays, stress_fields
from tests.children import ROOT, run_program, run_rate_tool

pytestmark = pytest.mark.gpu
RULES = [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_PERIODIC, capi.GS_BOUNDARY_NEUMANN]
RULE_SUFFIX = {0: "", 1: "", 2: "/periodic", 3: "/neumann"}
STRICT, FUSED = capi.GS_MATH_STRICT, capi.GS_MATH_FUSED

# Five members with distinct parameters, seeds, sigmas and starting steps.  Member 1 starts at 2^32 - 3: the high word of
# its step changes inside the first call; member 3's u64 counter wraps inside the second.  PARAMS[3] is the one member that
# is not .op-eligible (dt != 1); OP_PARAMS replaces it with one that is.
PARAMS = [Parameters(),
          Parameters(feed_rate=0.030, kill_rate=0.060),
          Parameters(feed_rate=0.022, kill_rate=0.051, diffusion_rate_u=0.12, diffusion_rate_v=0.06),
          Parameters(feed_rate=0.010, kill_rate=0.045, time_step=0.5),
          Parameters(feed_rate=0.046, kill_rate=0.063, diffusion_rate_u=0.2, diffusion_rate_v=0.1)]
OP_PARAMS = PARAMS[:3] + [Parameters(feed_rate=0.010, kill_rate=0.045)] + PARAMS[4:]
NOISES = [dict(sigma_u=0.02, sigma_v=0.01, seed=0x1234567890ABCDEF, step=0),
          dict(sigma_u=0.004, sigma_v=0.015, seed=7, step=2 ** 32 - 3),
          dict(sigma_u=0.01, sigma_v=0.0, seed=2 ** 64 - 1, step=5),
          dict(sigma_u=0.005, sigma_v=0.0025, seed=1 << 40, step=2 ** 64 - 14),
          dict(sigma_u=0.03, sigma_v=0.02, seed=99, step=123456789012)]
CALLS = (11, 8)  # a short windowed launch first (11 = 3 + 8), then a full one; the counters carried across the calls

# shape -> members of the ensemble.  A member of more than 1536 cells stays resident only when the members fill the chip:
# those shapes run 260 members, member i with the parameters, state and noise of member i % 5.
SHAPES = {(8, 16): 5,      # resident, 2 waves
          (37, 53): 260,   # resident, 2 cells per thread, odd sizes
          (64, 64): 260,   # resident, 4 cells per thread
          (64, 128): 260,  # resident, 8 cells per thread; windowed under the clipped rule (no 8-cell form there)
          (100, 300): 5}   # windowed, several windows both ways, periodic copies


def expect_resident(shape, rule):
    return shape != (100, 300) and not (shape == (64, 128) and rule == capi.GS_BOUNDARY_CLIPPED)


@functools.lru_cache(maxsize=None)
def fields(shape, i):
    u, v = stress_fields(shape, 4000 + i)
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


@functools.lru_cache(maxsize=None)
def reference(shape, i, op, rule, ftz, steps):
    """Member i of the five after ``steps`` steps from its initial state and starting step: computed once, shared, read-only."""
    p = (OP_PARAMS if op else PARAMS)[i]
    u0, v0 = fields(shape, i)
    u, v = N.run(u0, v0, steps, NOISES[i], params=oracle_params(p), rule=rule, ftz=ftz)
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


def make(shape, rule, math, op=False, members=None, noise=True, ctx_noise=None):
    n = members or SHAPES[shape]
    params = [(OP_PARAMS if op else PARAMS)[i % 5] for i in range(n)]
    sim = Simulation.new(params[0], HipArgs(devices=[0], boundary=rule, math=math))
    if ctx_noise:
        sim.set_noise(**ctx_noise)
    ens = sim.make_ensemble(shape, params, seed=False)
    ens.upload(np.stack([fields(shape, i % 5)[0] for i in range(n)]), np.stack([fields(shape, i % 5)[1] for i in range(n)]))
    if noise:
        ens.set_noise(*(np.array([NOISES[i % 5][k] for i in range(n)], dtype=object if k in ("seed", "step") else np.float32)
                        for k in ("sigma_u", "sigma_v", "seed", "step")))
    return sim, ens


def close(sim, *ensembles):
    for e in ensembles:
        e.destroy()
    sim.context.close()


def check_members(ens, which, op, rule, math, counts, what):
    u, v = ens.u_views(), ens.result_views()
    for m in which:
        ru, rv = reference(tuple(u.shape[1:]), m % 5, op, rule, math == STRICT, int(counts[m]))
        assert_bits_equal(u[m], ru, f"U of member {m} after {counts[m]} steps ({what})")
        assert_bits_equal(v[m], rv, f"V of member {m} after {counts[m]} steps ({what})")


# ---- 1. every form, rule and flavour against the restatement --------------------------------------------------------------
# strict: the .op kernels (every member eligible) and the general ones (one member is not); fused has no .op variant
VARIANTS = [(STRICT, True), (STRICT, False), (FUSED, False)]


@pytest.mark.parametrize("math,op", VARIANTS, ids=["strict.op", "strict", "fused"])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_members_are_the_reference(shape, rule, math, op):
    sim, ens = make(shape, rule, math, op)
    n, done = SHAPES[shape], 0
    which = list(range(5)) + ([n - 1] if n > 5 else [])  # (the last member of a full launch too)
    for steps in CALLS:
        ens.perform_steps(steps)
        done += steps
        name = sim.context.info()[0]
        form = "ensemble-resident/" if expect_resident(shape, rule) else "ensemble-tile"
        flavour = ("fused" if math == FUSED else "strict") + (".op" if op else "")
        assert name.startswith(form) and name.endswith("/" + flavour + RULE_SUFFIX[rule] + "/noise"), name
        got = ens.noise()
        assert got["step"].tolist() == [(NOISES[i % 5]["step"] + done) % 2 ** 64 for i in range(n)]
        assert got["seed"].tolist() == [NOISES[i % 5]["seed"] for i in range(n)]
        assert got["sigma_u"].tolist() == [np.float32(NOISES[i % 5]["sigma_u"]) for i in range(n)]
        check_members(ens, which, op, rule, math, [done] * n, name)
    close(sim, ens)


@pytest.mark.parametrize("math", [STRICT, FUSED])
@pytest.mark.parametrize("shape,rule", [((8, 16), capi.GS_BOUNDARY_PERIODIC), ((64, 128), capi.GS_BOUNDARY_ZERO_HALO),
                                        ((100, 300), capi.GS_BOUNDARY_CLIPPED), ((100, 300), capi.GS_BOUNDARY_PERIODIC)])
def test_members_are_lone_species_with_their_noise(shape, rule, math):
    """The contract as worded: a lone Species on a context with the member's parameters and the member's gs_noise attached."""
    sim, ens = make(shape, rule, math)
    for steps in CALLS:
        ens.perform_steps(steps)
    name = sim.context.info()[0]
    u, v = ens.u_views(), ens.result_views()
    close(sim, ens)
    for i in range(5):
        lone = Simulation.new(PARAMS[i], HipArgs(devices=[0], boundary=rule, math=math))
        species = species_from_arrays(lone, *fields(shape, i))
        lone.set_noise(**NOISES[i])
        for steps in CALLS:
            lone.perform_steps(species, steps)
        iu, iv, _, _ = species.in_out()
        lu, lv, solo = iu.make_scalar_view(lone.context), iv.make_scalar_view(lone.context), lone.context.info()[0]
        assert lone.noise()["step"] == (NOISES[i]["step"] + sum(CALLS)) % 2 ** 64
        lone.context.close()
        assert_bits_equal(u[i], lu, f"U of member {i} ({name} against {solo})")
        assert_bits_equal(v[i], lv, f"V of member {i} ({name} against {solo})")


# ---- 2. the bare field, zero sigmas ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", [STRICT, FUSED])
@pytest.mark.parametrize("shape", [(8, 16), (37, 53)], ids=["resident", "windowed"])
@pytest.mark.parametrize("sigmas", [(0.5, 0.25), (1e-38, 3e-39)], ids=["normal", "subnormal"])
def test_the_bare_noise_field(sigmas, shape, math):
    """du = dv = F = k = 0 on zero planes: the steps leave sums of sigma * xi.  With sigmas of (1e-38, 3e-39) every product
    is sub-normal: flushed in the strict flavour -- the planes stay zeros --, kept in the fused one."""
    p = Parameters(diffusion_rate_u=0.0, diffusion_rate_v=0.0, feed_rate=0.0, kill_rate=0.0)
    noise = dict(sigma_u=sigmas[0], sigma_v=sigmas[1], seed=77, step=2 ** 32 + 5)
    zero = np.zeros((1,) + shape, np.float32)
    sim = Simulation.new(p, HipArgs(devices=[0], math=math))
    ens = sim.make_ensemble(shape, [p], seed=False)
    ens.upload(zero, zero)
    ens.set_noise(**noise)
    ens.perform_steps(2)
    name = sim.context.info()[0]
    assert name.startswith("ensemble-resident" if shape == (8, 16) else "ensemble-tile") and name.endswith("/noise"), name
    ru, rv = N.run(zero[0], zero[0], 2, noise, params=oracle_params(p), ftz=math == STRICT)
    if math == STRICT and sigmas[0] < 1e-30:
        assert not ru.any() and not rv.any()  # (|xi| < 1: every product is below the smallest normal number)
    else:
        assert np.count_nonzero(ru) > ru.size // 2 and np.count_nonzero(rv) > rv.size // 2  # (the field is there)
    assert_bits_equal(ens.u_views()[0], ru, f"U ({name})")
    assert_bits_equal(ens.result_views()[0], rv, f"V ({name})")
    close(sim, ens)


MINUS_ZERO_CELLS = [(0, 0), (3, 5), (-1, -1)]


def signed_zero_fields(shape, n):
    """Stress fields with +0 and -0 planted in about a sixth of the cells, and U = V = -0 in MINUS_ZERO_CELLS."""
    out = []
    for i in range(n):
        u, v = (x.copy() for x in stress_fields(shape, 900 + i))
        rng = np.random.default_rng(950 + i)
        for x in (u, v):
            where = rng.random(shape) < 0.17
            x[where] = np.array([0.0, -0.0], np.float32)[rng.integers(0, 2, shape)[where]]
            for cell in MINUS_ZERO_CELLS:
                x[cell] = -0.0
        out.append((u, v))
    return np.stack([p[0] for p in out]), np.stack([p[1] for p in out])


@pytest.mark.parametrize("math", [STRICT, FUSED])
@pytest.mark.parametrize("shape", [(8, 16), (100, 300)], ids=["resident", "windowed"])
def test_zero_sigmas_and_clear_noise(shape, math):
    """One step: a species whose sigma is zero has the plain ensemble's bits (the other has not).  Both zero: the plain
    ensemble's bits after any steps, under a name that still says /noise; after clear_noise the plain kernel runs."""
    u0, v0 = signed_zero_fields(shape, 3)
    # Member 0 has rates of -0: where U = V = -0 its plain step leaves V = -0 (every term of dv is -0 there), the one way a
    # step's output is -0 -- the bits that an untouched species must keep and an added +0 would lose.
    params = [Parameters(diffusion_rate_u=-0.0, diffusion_rate_v=-0.0, feed_rate=-0.0, kill_rate=-0.0), PARAMS[1], PARAMS[2]]

    def run(noise, steps, clear=False):
        sim = Simulation.new(params[0], HipArgs(devices=[0], math=math))
        ens = sim.make_ensemble(shape, params, seed=False)
        ens.upload(u0, v0)
        if noise is not None:
            ens.set_noise(*noise)
        if clear:
            ens.clear_noise()
            assert ens.noise() is None
        ens.perform_steps(steps)
        out = ens.u_views(), ens.result_views(), sim.context.info()[0]
        close(sim, ens)
        return out

    pu, pv, plain = run(None, 1)
    assert "/noise" not in plain
    u, v, name = run((0.0, [0.01, 0.02, 0.03], 5, 9), 1)
    assert name == plain + "/noise", (name, plain)
    assert u.tobytes() == pu.tobytes() and all(v[i].tobytes() != pv[i].tobytes() for i in range(3))
    u, v, _ = run(([0.01, 0.02, 0.03], 0.0, 5, 9), 1)
    assert v.tobytes() == pv.tobytes() and all(u[i].tobytes() != pu[i].tobytes() for i in range(3))
    for cell in MINUS_ZERO_CELLS:  # (the -0 outputs the comparison is about are there)
        assert pv[0][cell] == 0 and np.signbit(pv[0][cell]), cell
    pu, pv, _ = run(None, 13)
    u, v, name = run((0.0, 0.0, [1, 2, 3], 2 ** 32 - 1), 13)
    assert name == plain + "/noise" and u.tobytes() == pu.tobytes() and v.tobytes() == pv.tobytes()
    u, v, name = run((0.5, 0.5, 1, 0), 13, clear=True)
    assert name == plain and u.tobytes() == pu.tobytes() and v.tobytes() == pv.tobytes()


# ---- 3. active sets, replay, the context's noise -----------------------------------------------------------------------------
@pytest.mark.parametrize("math", [STRICT, FUSED])
@pytest.mark.parametrize("shape,rule", [((8, 16), capi.GS_BOUNDARY_CLIPPED), ((8, 16), capi.GS_BOUNDARY_PERIODIC),
                                        ((100, 300), capi.GS_BOUNDARY_ZERO_HALO), ((100, 300), capi.GS_BOUNDARY_PERIODIC),
                                        ((100, 300), capi.GS_BOUNDARY_NEUMANN)])
def test_active_sets_keep_every_members_own_counter(shape, rule, math):
    """run 11; retire {1, 3}; run 8; reactivate {3}; run 11: every member equals the reference after its own step count,
    a retired member's counter stands still and goes on from where it stopped."""
    sim, ens = make(shape, rule, math)
    start = [n["step"] for n in NOISES]
    ens.perform_steps(11)
    assert sim.context.info()[0].endswith("/noise")
    ens.retire([1, 3])
    ens.perform_steps(8)
    name = sim.context.info()[0]
    assert name.endswith("/noise/listed"), name
    counts = [19, 11, 19, 11, 19]
    assert ens.steps_taken().tolist() == counts
    assert ens.noise()["step"].tolist() == [(s + c) % 2 ** 64 for s, c in zip(start, counts)]
    check_members(ens, range(5), False, rule, math, counts, name)
    ens.reactivate([3])
    assert ens.noise()["step"].tolist() == [(s + c) % 2 ** 64 for s, c in zip(start, counts)]  # (nothing moved)
    ens.perform_steps(11)
    name = sim.context.info()[0]
    assert name.endswith("/noise/listed"), name
    counts = [30, 11, 30, 22, 30]
    assert ens.steps_taken().tolist() == counts
    assert ens.noise()["step"].tolist() == [(s + c) % 2 ** 64 for s, c in zip(start, counts)]
    check_members(ens, range(5), False, rule, math, counts, name)
    # noise set on a retired member: its counter is the one given, and stands still
    ens.set_noise(0.5, 0.5, seed=3, step=1000, first=1, count=1)
    ens.perform_steps(2)
    assert ens.noise(1, 1)["step"].tolist() == [1000] and ens.noise(0, 1)["step"].tolist() == [(start[0] + 32) % 2 ** 64]
    ens.reactivate([1])
    ens.perform_steps(1)
    assert not sim.context.info()[0].endswith("/listed")
    assert ens.noise(1, 1)["step"].tolist() == [1001]
    close(sim, ens)


@pytest.mark.parametrize("shape", [(8, 16), (100, 300)], ids=["resident", "windowed"])
def test_replay_from_a_snapshot_and_the_structs(shape):
    rule, math = capi.GS_BOUNDARY_PERIODIC, STRICT
    sim, ens = make(shape, rule, math)
    ens.perform_steps(5)
    snap, saved = ens.snapshot(), ens.noise()
    assert snap.noise() is None  # gs_members_copy copies no noise
    ens.perform_steps(9)
    u, v = ens.u_views(), ens.result_views()
    fresh = sim.make_ensemble(shape, PARAMS, seed=False)
    fresh.copy_from(snap)
    fresh.set_noise(saved["sigma_u"], saved["sigma_v"], saved["seed"], saved["step"])
    fresh.perform_steps(9)
    assert fresh.u_views().tobytes() == u.tobytes() and fresh.result_views().tobytes() == v.tobytes()
    assert fresh.noise().tobytes() == ens.noise().tobytes()
    check_members(fresh, range(5), False, rule, math, [14] * 5, "replayed")
    close(sim, ens, snap, fresh)


def test_the_contexts_noise_stays_out_of_ensembles():
    shape, rule = (8, 16), capi.GS_BOUNDARY_CLIPPED
    out = []
    for ctx_noise in (None, dict(sigma_u=0.3, sigma_v=0.2, seed=5, step=40)):
        sim, ens = make(shape, rule, STRICT, ctx_noise=ctx_noise)
        ens.perform_steps(7)
        out.append((ens.u_views(), ens.result_views()))
        if ctx_noise:
            assert sim.noise()["step"] == 40  # an ensemble's steps are not the context's
        close(sim, ens)
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()


def test_refusals():
    sim, ens = make((8, 16), capi.GS_BOUNDARY_CLIPPED, STRICT, noise=False)
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    lib, ctx, e = sim.context._lib, sim.context.handle, ens.handle
    n = (capi.GsNoise * 5)(*[capi.GsNoise(0.1, 0.1, 1, 0)] * 5)
    attached = ctypes.c_int32(-1)
    cases = {"range": (ctx, e, 3, 3, n, 3), "empty range": (ctx, e, 0, 0, n, 1), "null noise": (ctx, e, 0, 5, None, 5),
             "entries": (ctx, e, 0, 5, n, 2), "foreign context": (other.context.handle, e, 0, 5, n, 5)}
    for what, args in cases.items():
        assert lib.gs_members_set_noise(*args) == capi.GS_ERR_INVALID, what
    for bad in (-0.5, float("nan"), float("inf")):
        for field in ("sigma_u", "sigma_v"):
            m = (capi.GsNoise * 5)(*[capi.GsNoise(0.1, 0.1, 1, 0) for _ in range(5)])
            setattr(m[4], field, bad)
            assert lib.gs_members_set_noise(ctx, e, 0, 5, m, 5) == capi.GS_ERR_INVALID, (field, bad)
            assert b"sigma" in lib.gs_last_error()
    assert lib.gs_members_get_noise(ctx, e, 0, 5, None, None) == capi.GS_ERR_INVALID
    assert lib.gs_members_get_noise(ctx, e, 4, 2, n, ctypes.byref(attached)) == capi.GS_ERR_INVALID
    # nothing was attached by any of them, and `out` is untouched while nothing is
    assert lib.gs_members_get_noise(ctx, e, 0, 5, n, ctypes.byref(attached)) == capi.GS_OK and attached.value == 0
    assert n[0].seed == 1 and ens.noise() is None
    with pytest.raises(GsError):
        ens.set_noise(-1.0)
    # the first call names one member: the others hold sigmas 0, seed 0, step 0 -- from now on
    ens.perform_steps(3)
    ens.set_noise(0.25, 0.5, seed=9, step=100, first=2, count=1)
    got = ens.noise()
    assert got["step"].tolist() == [0, 0, 100, 0, 0] and got["seed"].tolist() == [0, 0, 9, 0, 0]
    assert got["sigma_v"].tolist() == [0, 0, 0.5, 0, 0]
    ens.perform_steps(4)
    assert ens.noise()["step"].tolist() == [4, 4, 104, 4, 4]
    ens.clear_noise()
    ens.clear_noise()  # (detaching twice is fine)
    other.context.close()
    close(sim, ens)


# ---- 4. the sweep driver end to end -------------------------------------------------------------------------------------------
def test_sweep_with_realisations(tmp_path):
    args = ["--feed", "0.02:0.04:2", "--kill", "0.055:0.062:2", "-r", "16", "-c", "32", "-s", "12", "--realisations", "3",
            "--noise", "0.01:0.005", "--noise-seed", "7"]
    for d in ("a", "b"):
        (tmp_path / d).mkdir()
        r = run_program([sys.executable, "-m", "grayscott_amd.sweep"] + args + ["-o", str(tmp_path / d / "run.h5")], cwd=ROOT, limit=300)
        assert r.returncode == 0, r.stderr
    for name in ("run.h5", "run.json"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read(), name
    side = json.load(open(tmp_path / "a" / "run.json"))
    images = hdf5_min.read(str(tmp_path / "a" / "run.h5"))
    assert images.shape == (12, 16, 32) and len(side["members"]) == 12 and side["steps"] == 12
    assert side["noise"] == {"sigma_u": 0.01, "sigma_v": 0.005, "seed": 7, "realisations": 3}
    u0, v0 = oracle.init_species(16, 32)
    points = [(f, k) for k in (0.055, 0.062) for f in (0.02, 0.04)]
    for point, (feed, kill) in enumerate(points):
        for r in range(3):
            m = side["members"][point * 3 + r]
            assert m == {"index": point * 3 + r, "feed": feed, "kill": kill, "realisation": r, "noise_seed": 7 + r}, m
            noise = dict(sigma_u=0.01, sigma_v=0.005, seed=7 + r, step=0)
            _, rv = N.run(u0, v0, 12, noise, params=oracle_params(Parameters(feed_rate=feed, kill_rate=kill)))
            assert_bits_equal(images[point * 3 + r], rv, f"image of point {point}, realisation {r}")
    # the realisations of a point differ, the same realisation at two points differs by the parameters only
    assert images[0].tobytes() != images[1].tobytes() and images[0].tobytes() != images[3].tobytes()


# ---- 5. the rate tool, once at small arguments ---------------------------------------------------------------------------------
def test_rate_tool_runs_and_proves_a_member(tmp_path):
    r, md, rows = run_rate_tool("ensemble_noise", ["--rows", "6x8x16:2,4x40x72", "--steps", "16", "--calls", "2", "--sample", "2"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert md[0].startswith("| members x grid | run | kernel |") and len(rows) == 2
    for row, form in zip(rows, ("ensemble-resident", "ensemble-tile")):
        assert row["bitcheck"] is True and row["bitcheck_steps"] == 48
        assert row["plain"]["kernel"].startswith(form) and "/noise" not in row["plain"]["kernel"]
        assert row["zero"]["kernel"] == row["noisy"]["kernel"] == row["plain"]["kernel"] + "/noise"
        assert row["sequential"]["kernel"].split("@")[0].endswith("/noise") and row["sequential"]["sampled"] == 2
        assert all(row[k]["ms"] > 0 for k in ("plain", "zero", "noisy", "sequential"))
