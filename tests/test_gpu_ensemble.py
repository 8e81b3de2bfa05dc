"""Ensembles on the MI355X: every member bit for bit what a lone Species with its parameters and initial state becomes --
against the CPU oracle (strict math) and against gs_run (both flavours) -- under both boundary rules, in both kernel
forms (resident, windowed), with members that differ in feed, kill, diffusion rates, dt and stencil."""
from __future__ import annotations

import ctypes
import json
import sys

import numpy as np
import pytest

import oracle
from grayscott_amd import HipArgs, Parameters, Simulation, capi, hdf5_min
from grayscott_amd.simulation import STENCILS

from .helpers import assert_bits_equal, gpu_run, oracle_params, stress_fields
from tests.children import ROOT, run_program

pytestmark = pytest.mark.gpu

# six members with distinct (feed, kill, du, dv, dt), the defaults first
PARAMS = [Parameters(),
          Parameters(feed_rate=0.030, kill_rate=0.060),
          Parameters(feed_rate=0.022, kill_rate=0.051, diffusion_rate_u=0.12, diffusion_rate_v=0.06),
          Parameters(feed_rate=0.010, kill_rate=0.045, time_step=0.5),
          Parameters(feed_rate=0.046, kill_rate=0.063, diffusion_rate_u=0.2, diffusion_rate_v=0.1, time_step=0.25),
          Parameters(feed_rate=0.018, kill_rate=0.049, diffusion_rate_v=0.03, time_step=2.0)]


def member_fields(n, shape, seed=0):
    pairs = [stress_fields(shape, seed * 1000 + i) for i in range(n)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def run_ensemble(params, u0, v0, steps, boundary=capi.GS_BOUNDARY_CLIPPED, math=capi.GS_MATH_STRICT, calls=None):
    sim = Simulation.new(params[0], HipArgs(devices=[0], boundary=boundary, math=math))
    ens = sim.make_ensemble(u0.shape[1:], params, seed=False)
    ens.upload(u0, v0)
    for n in (calls or [steps]):
        ens.prepare_steps(n)
    u, v = ens.u_views(), ens.result_views()
    name = sim.context.info()[0]
    ens.destroy()
    sim.context.close()
    return u, v, name


def assert_member_is_oracle(i, p, u0, v0, steps, boundary, u, v, name):
    ref_u, ref_v = oracle.run(u0, v0, steps, params=oracle_params(p), ftz=True, boundary=boundary)
    assert_bits_equal(u, ref_u, f"U of member {i} ({name})")
    assert_bits_equal(v, ref_v, f"V of member {i} ({name})")


CASES = [(s, n) for s in [(8, 16), (16, 32), (37, 53)] for n in (1, 7, 64, 1000)] + [((64, 128), 7), ((64, 128), 64),
                                                                                      ((100, 300), 7), ((100, 300), 64)]


@pytest.mark.parametrize("boundary", [oracle.CLIPPED, oracle.ZERO_HALO])
@pytest.mark.parametrize("shape,steps", CASES)
def test_members_match_the_oracle(shape, steps, boundary):
    u0, v0 = member_fields(len(PARAMS), shape, seed=steps)
    u, v, name = run_ensemble(PARAMS, u0, v0, steps, boundary=boundary)
    assert name.startswith("ensemble-") and ".op" not in name, name
    for i, p in enumerate(PARAMS):
        assert_member_is_oracle(i, p, u0[i], v0[i], steps, boundary, u[i], v[i], name)


@pytest.mark.parametrize("boundary", [oracle.CLIPPED, oracle.ZERO_HALO])
@pytest.mark.parametrize("shape", [(64, 64), (37, 100), (64, 128)])
def test_resident_form_for_members_that_fill_the_chip(shape, boundary):
    """With at least one member per CU, members of up to 4096 cells (8192 under the zero-halo rule) stay on one CU."""
    n = 300
    rng = np.random.default_rng(7)
    params = [Parameters(feed_rate=float(f), kill_rate=float(k)) for f, k in zip(rng.uniform(0.01, 0.05, n), rng.uniform(0.045, 0.065, n))]
    u0, v0 = member_fields(n, shape, seed=3)
    u, v, name = run_ensemble(params, u0, v0, 33, boundary=boundary)
    cells = shape[0] * shape[1]
    resident = cells <= 4096 or (cells <= 8192 and boundary == oracle.ZERO_HALO)
    assert name.startswith("ensemble-resident/" if resident else "ensemble-tile"), name
    for i in (0, 1, n // 2, n - 1):
        assert_member_is_oracle(i, params[i], u0[i], v0[i], 33, boundary, u[i], v[i], name)


@pytest.mark.parametrize("math", [capi.GS_MATH_STRICT, capi.GS_MATH_FUSED])
@pytest.mark.parametrize("shape,members,steps", [((256, 512), 6, 40), ((1024, 2048), 3, 40)])
def test_members_equal_lone_species(shape, members, steps, math):
    params = PARAMS[:members]
    u0, v0 = member_fields(members, shape, seed=11)
    u, v, name = run_ensemble(params, u0, v0, steps, math=math)
    assert name.startswith("ensemble-tile") and name.split("/")[1].startswith("fused" if math else "strict"), name
    for i, p in enumerate(params):
        ru, rv, (solo, _) = gpu_run(u0[i], v0[i], steps, p, HipArgs(devices=[0], math=math))
        assert_bits_equal(u[i], ru, f"U of member {i} ({name} against {solo})")
        assert_bits_equal(v[i], rv, f"V of member {i} ({name} against {solo})")


@pytest.mark.parametrize("shape", [(16, 32), (37, 53)])
def test_members_with_different_stencils(shape):
    params = [Parameters.with_stencil(n, feed_rate=0.02 + 0.005 * i) for i, n in enumerate(sorted(STENCILS))]
    u0, v0 = member_fields(len(params), shape, seed=5)
    u, v, name = run_ensemble(params, u0, v0, 64)
    assert ".op" not in name, name  # 5points / pretty / patrakarttunen: side weights are not 0.5
    for i, p in enumerate(params):
        assert_member_is_oracle(i, p, u0[i], v0[i], 64, oracle.CLIPPED, u[i], v[i], name)


@pytest.mark.parametrize("shape", [(8, 16), (37, 53)])
def test_specialised_kernel_only_when_every_member_qualifies(shape):
    ops = [Parameters(feed_rate=0.01 * (i + 1)) for i in range(4)]  # side weights 0.5, dt == 1
    u0, v0 = member_fields(4, shape, seed=9)
    for params, op in ((ops, True), (ops[:3] + [Parameters(feed_rate=0.04, time_step=0.5)], False),
                       (ops[:3] + [Parameters.with_stencil("5points")], False)):
        u, v, name = run_ensemble(params, u0, v0, 20)
        assert name.endswith(".op") == op, name
        for i, p in enumerate(params):
            assert_member_is_oracle(i, p, u0[i], v0[i], 20, oracle.CLIPPED, u[i], v[i], name)


@pytest.mark.parametrize("shape", [(8, 16), (37, 53), (256, 512)])
@pytest.mark.parametrize("fill", [3.0e38, np.nan, np.inf])
def test_a_wild_member_leaves_its_neighbours_alone(shape, fill):
    params = PARAMS[:3]
    u0, v0 = member_fields(3, shape, seed=2)
    u0[1].fill(fill)
    v0[1].fill(fill)
    u, v, name = run_ensemble(params, u0, v0, 24)
    for i in (0, 2):
        ru, rv, _ = gpu_run(u0[i], v0[i], 24, params[i])
        assert_bits_equal(u[i], ru, f"U of member {i} next to a member of {fill} ({name})")
        assert_bits_equal(v[i], rv, f"V of member {i} next to a member of {fill} ({name})")


@pytest.mark.parametrize("shape", [(8, 16), (37, 53)])
def test_calls_compose_and_subsets_download(shape):
    u0, v0 = member_fields(len(PARAMS), shape, seed=4)
    u11, v11, _ = run_ensemble(PARAMS, u0, v0, 11)
    u56, v56, _ = run_ensemble(PARAMS, u0, v0, 11, calls=[5, 0, 6])
    assert_bits_equal(u56, u11, "U after run(5); run(0); run(6)")
    assert_bits_equal(v56, v11, "V after run(5); run(0); run(6)")
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ens = sim.make_ensemble(shape, PARAMS, seed=False)
    ens.upload(u0, v0)
    ens.perform_steps(0)
    assert_bits_equal(ens.u_views(), u0, "U after run(0)")
    ens.perform_steps(11)
    assert_bits_equal(ens.result_views(2, 3), v11[2:5], "V of members 2-4")
    assert_bits_equal(ens.u_views(5, 1), u11[5:6], "U of member 5")
    ens.upload(None, v0[1:3], first=4)  # V of members 4 and 5 only
    assert_bits_equal(ens.result_views(4), v0[1:3], "V uploaded into members 4, 5")
    assert_bits_equal(ens.u_views(4), u11[4:6], "U of members 4, 5 untouched")
    with pytest.raises(capi.GsError) as e:
        ens.result_views(5, 2)
    assert e.value.code == capi.GS_ERR_INVALID
    ens.destroy()
    sim.context.close()


@pytest.mark.parametrize("shape", [(8, 16), (37, 53), (100, 300)])
def test_seed_is_species_new(shape):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ens = sim.make_ensemble(shape, PARAMS)
    su, sv = oracle.init_species(*shape)
    u, v = ens.u_views(), ens.result_views()
    for i in range(len(PARAMS)):
        assert_bits_equal(u[i], su, f"U of seeded member {i}")
        assert_bits_equal(v[i], sv, f"V of seeded member {i}")
    ens.destroy()
    sim.context.close()


def test_refusals():
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], math=capi.GS_MATH_FUSED))
    lib, handle = sim.context._lib, ctypes.c_void_p()
    for members, rows, cols in ((0, 8, 16), (2, 0, 16), (2, 8, 0)):
        assert lib.gs_ensemble_create(sim.context.handle, ctypes.byref(handle), members, rows, cols) == capi.GS_ERR_INVALID
        assert not handle.value
    with pytest.raises(capi.GsError) as e:  # fused math: weights 0 or powers of two only, as gs_ctx_create
        sim.make_ensemble((8, 16), [Parameters(), Parameters.with_stencil("patrakarttunen")])
    assert e.value.code == capi.GS_ERR_UNSUPPORTED
    ens = sim.make_ensemble((8, 16), Parameters(), members=3)
    with pytest.raises(capi.GsError) as e:
        ens.set_params([Parameters()] * 2)
    assert e.value.code == capi.GS_ERR_INVALID
    ens.destroy()
    sim.context.close()
    chain = Simulation.new(Parameters(), HipArgs(devices=[0, 0]))
    with pytest.raises(capi.GsError) as e:
        chain.make_ensemble((8, 16), Parameters(), members=2)
    assert e.value.code == capi.GS_ERR_UNSUPPORTED
    chain.context.close()


def test_member_offsets_are_64_bit():
    """1100 members of 1024 x 2048: each plane holds 2.3 G floats (9.2 GB; 37 GB for the four).  The last member, given
    its own state and parameters, equals its lone run; the first is the seed pattern advanced."""
    members, shape, steps = 1100, (1024, 2048), 8
    assert members * shape[0] * shape[1] > 2 ** 31
    p_last = Parameters(feed_rate=0.037, kill_rate=0.061, diffusion_rate_u=0.15)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ens = sim.make_ensemble(shape, [Parameters()] * (members - 1) + [p_last])
    u0, v0 = stress_fields(shape, 42)
    ens.upload(u0[None], v0[None], first=members - 1)
    ens.perform_steps(steps)
    ru, rv, _ = gpu_run(u0, v0, steps, p_last)
    assert_bits_equal(ens.u_views(members - 1), ru[None], "U of the last member")
    assert_bits_equal(ens.result_views(members - 1), rv[None], "V of the last member")
    su, sv = oracle.init_species(*shape)
    fu, fv, _ = gpu_run(su, sv, steps, Parameters())
    assert_bits_equal(ens.result_views(0, 1), fv[None], "V of the first member")
    assert_bits_equal(ens.result_views(members // 2, 1), fv[None], "V of a middle member")
    ens.destroy()
    sim.context.close()


def test_sweep_end_to_end(tmp_path):
    out = tmp_path / "sweep.h5"
    rows, cols, steps = 40, 64, 50
    r = run_program([sys.executable, "-m", "grayscott_amd.sweep", "--feed", "0.01:0.04:4", "--kill", "0.045:0.06:4",
                     "-r", str(rows), "-c", str(cols), "-s", str(steps), "-o", str(out)],
                    cwd=ROOT, limit=300)
    assert r.returncode == 0, r.stderr
    images = hdf5_min.read(str(out))
    side = json.load(open(tmp_path / "sweep.json"))
    assert images.shape == (16, rows, cols) and len(side["members"]) == 16
    kills = sorted({m["kill"] for m in side["members"]})
    u0, v0 = oracle.init_species(rows, cols)
    for m in side["members"]:
        assert m["index"] == kills.index(m["kill"]) * 4 + [x["feed"] for x in side["members"][:4]].index(m["feed"])
        _, ref_v = oracle.run(u0, v0, steps, params=oracle_params(Parameters(feed_rate=m["feed"], kill_rate=m["kill"])), ftz=True)
        assert_bits_equal(images[m["index"]], ref_v, f"image {m['index']} (F = {m['feed']}, k = {m['kill']})")
