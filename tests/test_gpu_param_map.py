"""Parameter maps on the MI355X (gs_ctx_set_param_map): per-cell feed and kill rates, bit for bit against the mapped
reference of tests/param_map_ref.py under every boundary rule, in the strict flavour and in the fused one on states
without sub-normals; every form of the marching kernel (K = 1..4, 1, 2 and 4 columns per lane, general and .op), the
single-step kernels of gs_step, slab chains, row bands and two processes; a uniform map changes no bit; the map's
lifecycle (replace, detach, the caller's planes destroyed, graph replay, set_params switching between the .op and the
general form, the two kernel sets' tuned choices) never replays stale state; the refusals;
ensembles ignore the map; the simulate driver end to end."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import pytest

from grayscott_amd import GsError, HipArgs, Parameters, Simulation, capi, hdf5_min

from . import param_map_ref as R
from .helpers import assert_bits_equal, species_from_arrays, stress_fields
from tests.children import ROOT, run_program, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
RULES = [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_PERIODIC, capi.GS_BOUNDARY_NEUMANN]
RULE_SUFFIX = {0: "/map", 1: "/map", 2: "/periodic/map", 3: "/neumann/map"}


def random_map(shape, seed):
    """F in [0.01, 0.06], k in [0.04, 0.07]: the range where patterns form."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.01, 0.06, shape).astype(np.float32), rng.uniform(0.04, 0.07, shape).astype(np.float32))


def mapped_run(u0, v0, steps, feed, kill, args, stepwise=False, calls=None):
    """upload -> set_param_map -> gs_run (in `calls` pieces) or gs_step x steps -> download."""
    sim = Simulation.new(Parameters(), args)
    try:
        species = species_from_arrays(sim, u0, v0)
        sim.set_param_map(feed, kill, shape=u0.shape)
        if stepwise:
            for _ in range(steps):
                sim.perform_step(species)
        else:
            for n in (calls or [steps]):
                sim.perform_steps(species, n)
        iu, iv, _, _ = species.in_out()
        return iu.make_scalar_view(sim.context), iv.make_scalar_view(sim.context), sim.context.info()[0]
    finally:
        sim.context.close()


def check(got_u, got_v, name, ref, boundary, what):
    assert name.split("@")[0].endswith(RULE_SUFFIX[boundary]), (name, what)
    assert_bits_equal(got_u, ref[0], f"U {what} ({name})")
    assert_bits_equal(got_v, ref[1], f"V {what} ({name})")


# ---- 1. random maps against the reference: every marching form, rule and flavour --------------------------------------
# strict: the .op variant (default weights) and the general one; fused: the general one (it has no .op variant)
TB_FORMS = [dict(cols_per_lane=c, fuse_steps=k, general_kernels=g, math=m) for c in (1, 2, 4) for k in (1, 2, 3, 4)
            for g, m in ((0, capi.GS_MATH_STRICT), (1, capi.GS_MATH_STRICT), (0, capi.GS_MATH_FUSED))]


@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("cfg", TB_FORMS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_marching_kernel_forms(cfg, boundary):
    cfg = dict(cfg)
    math = cfg.pop("math")
    for shape, seed in (((61, 263), 1), ((9, 70), 2)):
        u0, v0 = stress_fields(shape, seed)
        feed, kill = random_map(shape, seed + 10)
        steps = 11  # remainder passes for K = 2, 3, 4
        ref = R.run(u0, v0, steps, feed, kill, boundary=boundary, ftz=math == capi.GS_MATH_STRICT)
        got_u, got_v, name = mapped_run(u0, v0, steps, feed, kill, HipArgs(
            devices=[0], boundary=boundary, math=math, kernel=capi.GS_KERNEL_TB, no_tune=1, **cfg))
        assert name.startswith("tb-k") and ("/fused" in name) == (math == capi.GS_MATH_FUSED), name
        assert (".op" in name) == (math == capi.GS_MATH_STRICT and not cfg["general_kernels"]), name
        check(got_u, got_v, name, ref, boundary, f"{shape} {cfg}")


@pytest.mark.parametrize("math", [capi.GS_MATH_STRICT, capi.GS_MATH_FUSED])
@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("kernel", [capi.GS_KERNEL_SIMPLE, capi.GS_KERNEL_STREAM])
def test_single_step_kernels(kernel, boundary, math):
    for shape in ((1, 1), (7, 5), (40, 300), (33, 257)):
        u0, v0 = stress_fields(shape, 4)
        feed, kill = random_map(shape, 14)
        ref = R.run(u0, v0, 5, feed, kill, boundary=boundary, ftz=math == capi.GS_MATH_STRICT)
        got_u, got_v, name = mapped_run(u0, v0, 5, feed, kill, HipArgs(devices=[0], boundary=boundary, math=math,
                                                                        kernel=kernel), stepwise=True)
        assert name.startswith("simple" if kernel == capi.GS_KERNEL_SIMPLE else "stream"), name
        check(got_u, got_v, name, ref, boundary, f"{shape}")


@pytest.mark.parametrize("math", [capi.GS_MATH_STRICT, capi.GS_MATH_FUSED])
@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("shape", [(1, 1), (40, 37), (256, 512), (1080, 1920)])
def test_auto_runs_the_marching_kernel_at_every_size(shape, boundary, math):
    """Sizes that run the resident, tile and window kernels without a map; calls of 1, 2, 26 and 67 steps."""
    u0, v0 = stress_fields(shape, 5)
    feed, kill = random_map(shape, 15)
    calls = [1, 2, 26, 67]
    ref = R.run(u0, v0, sum(calls), feed, kill, boundary=boundary, ftz=math == capi.GS_MATH_STRICT)
    got_u, got_v, name = mapped_run(u0, v0, 0, feed, kill, HipArgs(devices=[0], boundary=boundary, math=math), calls=calls)
    assert name.startswith("tb-k"), name
    check(got_u, got_v, name, ref, boundary, f"{shape}")


# ---- 2. a uniform map changes no bit ----------------------------------------------------------------------------------
UNIFORM = ([((300, 701), 37, b, m) for b in RULES for m in (capi.GS_MATH_STRICT, capi.GS_MATH_FUSED)]
           + [((16384, 16384), 300, b, m) for b, m in ((0, capi.GS_MATH_STRICT), (2, capi.GS_MATH_STRICT),
                                                         (3, capi.GS_MATH_FUSED))])


@pytest.mark.parametrize("shape,steps,boundary,math", UNIFORM)
def test_uniform_map_changes_nothing(shape, steps, boundary, math):
    import oracle

    p = Parameters()
    u0, v0 = oracle.init_species(*shape)
    out = []
    for mapped in (False, True):
        sim = Simulation.new(p, HipArgs(devices=[0], boundary=boundary, math=math))
        try:
            species = species_from_arrays(sim, u0, v0)
            if mapped:
                sim.set_param_map(p.feed_rate, p.kill_rate, shape=shape)
            sim.perform_steps(species, steps)
            iu, iv, _, _ = species.in_out()
            out.append((iu.make_scalar_view(sim.context), iv.make_scalar_view(sim.context), sim.context.info()[0]))
        finally:
            sim.context.close()
    assert out[1][2].split("@")[0].endswith(RULE_SUFFIX[boundary]) and not out[0][2].split("@")[0].endswith("/map"), out
    assert_bits_equal(out[1][0], out[0][0], f"U {shape} ({out[1][2]} vs {out[0][2]})")
    assert_bits_equal(out[1][1], out[0][1], f"V {shape} ({out[1][2]} vs {out[0][2]})")


# ---- 3. slab chains, row bands, processes -----------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_NEUMANN])
@pytest.mark.parametrize("devices,shape", [([0, 0], (300, 701)), ([0, 0, 0], (600, 1003)), ([0, 0, 0], (11, 40))])
@pytest.mark.parametrize("kernel", [capi.GS_KERNEL_AUTO, capi.GS_KERNEL_STREAM])
def test_slab_chains(devices, shape, kernel, boundary):
    u0, v0 = stress_fields(shape, 6)
    feed, kill = random_map(shape, 16)
    ref = R.run(u0, v0, 11, feed, kill, boundary=boundary)
    got_u, got_v, name = mapped_run(u0, v0, 11, feed, kill, HipArgs(devices=devices, boundary=boundary, kernel=kernel))
    check(got_u, got_v, name, ref, boundary, f"{shape} {devices}")


@pytest.mark.parametrize("boundary", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_NEUMANN])
def test_row_bands(boundary):
    shape = (1000, 1003)
    u0, v0 = stress_fields(shape, 7)
    feed, kill = random_map(shape, 17)
    ref = R.run(u0, v0, 13, feed, kill, boundary=boundary)
    got_u, got_v, name = mapped_run(u0, v0, 13, feed, kill, HipArgs(devices=[0], boundary=boundary, split=2))
    check(got_u, got_v, name, ref, boundary, "split 2")


def _worker(rank, world, port, rows, cols, steps, out_dir, transport_lib, boundary):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", GS_RCCL_LIBRARY=transport_lib)
    import torch.distributed as dist

    from grayscott_amd import HipArgs, Parameters, Simulation
    from grayscott_amd import dist as gsd
    from tests.helpers import species_from_arrays, stress_fields
    from tests.test_gpu_param_map import random_map

    info = gsd.bootstrap(backend="gloo", device="cpu")
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], rank=info.rank, world=info.world,
                                               unique_id=info.unique_id, boundary=boundary))
    r0, r1 = gsd.slab_range(rows, world, rank)
    u0, v0 = stress_fields((rows, cols), 22)
    feed, kill = random_map((rows, cols), 23)
    species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(rows, cols))
    sim.set_param_map(feed, kill)
    sim.perform_steps(species, steps)
    for _ in range(3):
        sim.perform_step(species)
    in_u, in_v, _, _ = species.in_out()
    u = gsd.gather_rows(in_u.make_scalar_view(sim.context), rank, world)
    v = gsd.gather_rows(in_v.make_scalar_view(sim.context), rank, world)
    if rank == 0:
        np.save(os.path.join(out_dir, "u.npy"), u)
        np.save(os.path.join(out_dir, "v.npy"), v)
        open(os.path.join(out_dir, "name"), "w").write(sim.context.info()[0])
    dist.barrier()
    sim.context.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("boundary", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_NEUMANN])
def test_two_processes_over_the_shm_transport(tmp_path, built, shm_transport, boundary):  # noqa: F811
    from tests.helpers import free_port

    rows, cols, steps = 300, 517, 14
    spawn_ranks(_worker, (2, free_port(), rows, cols, steps, str(tmp_path), shm_transport, boundary), 2)
    u0, v0 = stress_fields((rows, cols), 22)
    feed, kill = random_map((rows, cols), 23)
    ref = R.run(u0, v0, steps + 3, feed, kill, boundary=boundary)
    check(np.load(tmp_path / "u.npy"), np.load(tmp_path / "v.npy"), open(tmp_path / "name").read(), ref, boundary,
          "2 processes")


# ---- 4. lifecycle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("boundary", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_PERIODIC])
def test_attach_replace_detach(use_graph, boundary):
    """Each phase continues from the state the last one left; a stale graph or tuning would show in the bits."""
    shape = (300, 701)
    p = Parameters()
    u0, v0 = stress_fields(shape, 8)
    maps = [random_map(shape, 18), random_map(shape, 19)]
    sim = Simulation.new(p, HipArgs(devices=[0], boundary=boundary, use_graph=use_graph, fuse_steps=4))
    try:
        species = species_from_arrays(sim, u0, v0)
        ref = (u0, v0)
        for phase in ("map0", "map1", "none", "map0"):
            if phase == "none":
                sim.clear_param_map()
                feed, kill = p.feed_rate, p.kill_rate
            else:
                feed, kill = maps[int(phase[-1])]
                sim.set_param_map(feed, kill)
            sim.perform_steps(species, 70)  # 17 passes + 2: graph batches of 16 passes and a remainder
            ref = R.run(ref[0], ref[1], 70, feed, kill, boundary=boundary)
            iu, iv, _, _ = species.in_out()
            name = sim.context.info()[0]
            assert name.split("@")[0].endswith("/map") == (phase != "none"), (phase, name)
            assert_bits_equal(iu.make_scalar_view(sim.context), ref[0], f"U after {phase} ({name})")
            assert_bits_equal(iv.make_scalar_view(sim.context), ref[1], f"V after {phase} ({name})")
    finally:
        sim.context.close()


# dt = 0.5 and power-of-two weights that are not the default ones, a centre weight included: the general map form
SKEWED = Parameters(weights=((0.25, 0.5, 0.125), (1.0, 0.5, 0.25), (0.0, 0.125, 0.5)), time_step=0.5)


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("boundary", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_PERIODIC])
def test_map_across_set_params(use_graph, boundary):
    """set_params with a map attached switches the map form between .op and the general one (and back); detaching and
    re-attaching keeps the parameters in force.  Each phase continues from the state the last one left."""
    shape = (300, 701)
    default = Parameters()
    u0, v0 = stress_fields(shape, 10)
    feed, kill = random_map(shape, 21)
    sim = Simulation.new(default, HipArgs(devices=[0], boundary=boundary, use_graph=use_graph, fuse_steps=4))
    try:
        species = species_from_arrays(sim, u0, v0)
        sim.set_param_map(feed, kill)
        ref = (u0, v0)
        for phase, p in (("defaults", default), ("skewed", SKEWED), ("defaults again", default), ("detached", default),
                         ("re-attached", default)):
            mapped = phase != "detached"
            if phase == "detached":
                sim.clear_param_map()
            elif phase == "re-attached":
                sim.set_param_map(feed, kill)
            else:
                sim.context.set_params(p)
            sim.perform_steps(species, 70)  # 17 passes + 2: graph batches of 16 passes and a remainder
            ref = R.run(ref[0], ref[1], 70, feed if mapped else p.feed_rate, kill if mapped else p.kill_rate,
                        params=R.params_of(p), boundary=boundary)
            iu, iv, _, _ = species.in_out()
            name = sim.context.info()[0]
            assert name.split("@")[0].endswith("/map") == mapped, (phase, name)
            if mapped:
                assert name.split("@")[0].endswith(RULE_SUFFIX[boundary]), (phase, name)
                assert name.startswith("tb-k4") and (".op" in name) == (p is default), (phase, name)
            assert_bits_equal(iu.make_scalar_view(sim.context), ref[0], f"U after {phase} ({name})")
            assert_bits_equal(iv.make_scalar_view(sim.context), ref[1], f"V after {phase} ({name})")
    finally:
        sim.context.close()


def test_tuned_choices_of_each_kernel_set():
    """gs_ctx_set_tuned with a map attached pins the mapped run (K and CPL in its name); gs_ctx_get_tuned returns the
    uniform set's choice after a detach and the map set's after re-attaching."""
    shape = (200, 300)
    u0, v0 = stress_fields(shape, 11)
    feed, kill = random_map(shape, 24)
    p = Parameters()
    sim = Simulation.new(p, HipArgs(devices=[0], kernel=capi.GS_KERNEL_TB, no_tune=1))
    try:
        ctx = sim.context
        species = species_from_arrays(sim, u0, v0)
        ref = (u0, v0)

        def steps(mapped, prefix):
            nonlocal ref
            sim.perform_steps(species, 9)
            ref = R.run(ref[0], ref[1], 9, feed if mapped else p.feed_rate, kill if mapped else p.kill_rate)
            name = ctx.info()[0]
            assert name.startswith(prefix) and name.split("@")[0].endswith("/map") == mapped, (prefix, name)
            iu, iv, _, _ = species.in_out()
            assert_bits_equal(iu.make_scalar_view(ctx), ref[0], f"U ({name})")
            assert_bits_equal(iv.make_scalar_view(ctx), ref[1], f"V ({name})")

        ctx.set_tuned(shape[0], shape[1], 8, 3, 2)
        uniform = ctx.get_tuned(*shape)
        assert uniform[:3] == (8, 3, 2), uniform
        steps(False, "tb-k3c2/")
        sim.set_param_map(feed, kill)
        assert ctx.get_tuned(*shape) == (0, 0, 0, 0)   # nothing chosen for the map's kernels yet
        ctx.set_tuned(shape[0], shape[1], 16, 2, 1)
        mapped = ctx.get_tuned(*shape)
        assert mapped[:3] == (16, 2, 1), mapped
        steps(True, "tb-k2c1/")
        sim.clear_param_map()
        assert ctx.get_tuned(*shape) == uniform
        steps(False, "tb-k3c2/")
        sim.set_param_map(feed, kill)
        assert ctx.get_tuned(*shape) == mapped
        steps(True, "tb-k2c1/")
    finally:
        sim.context.close()


def test_caller_planes_may_change_and_go():
    """The library copies the map: the caller's planes are overwritten, then destroyed, before the steps run."""
    shape = (64, 300)
    u0, v0 = stress_fields(shape, 9)
    feed, kill = random_map(shape, 20)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    try:
        ctx = sim.context
        f = sim.Concentration(ctx, shape)
        k = sim.Concentration(ctx, shape)
        f.upload(ctx, feed)
        k.upload(ctx, kill)
        capi.check(ctx._lib.gs_ctx_set_param_map(ctx.handle, f.handle, k.handle))
        f.upload(ctx, np.zeros(shape, np.float32))
        k.upload(ctx, np.ones(shape, np.float32))
        f.destroy()
        k.destroy()
        species = species_from_arrays(sim, u0, v0)
        sim.perform_steps(species, 9)
        iu, iv, _, _ = species.in_out()
        ref = R.run(u0, v0, 9, feed, kill)
        check(iu.make_scalar_view(ctx), iv.make_scalar_view(ctx), ctx.info()[0], ref, 0, "after the caller's planes went")
    finally:
        sim.context.close()


def test_wrong_shape_and_refusals():
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    try:
        species = species_from_arrays(sim, *stress_fields((40, 300), 1))
        sim.set_param_map(*random_map((41, 300), 2))
        for call in (lambda: sim.perform_steps(species, 5), lambda: sim.perform_step(species)):
            with pytest.raises(GsError) as e:
                call()
            assert e.value.code == capi.GS_ERR_INVALID
        with pytest.raises(GsError) as e:
            capi.check(sim.context._lib.gs_ctx_set_param_map(sim.context.handle, species.in_out()[0].handle, None))
        assert e.value.code == capi.GS_ERR_INVALID
        sim.clear_param_map()
        sim.perform_steps(species, 5)
    finally:
        sim.context.close()
    for kernel in (capi.GS_KERNEL_WINDOW, capi.GS_KERNEL_LDS, capi.GS_KERNEL_TILE):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0], kernel=kernel))
        try:
            with pytest.raises(GsError) as e:
                sim.set_param_map(0.03, 0.06, shape=(40, 300))
            assert e.value.code == capi.GS_ERR_UNSUPPORTED, kernel
        finally:
            sim.context.close()


# ---- 5. ensembles ignore the map -------------------------------------------------------------------------------------
def test_ensembles_ignore_the_map():
    shape = (37, 53)
    params = [Parameters(feed_rate=0.03, kill_rate=0.06), Parameters(feed_rate=0.022, kill_rate=0.051)]
    out = []
    for mapped in (False, True):
        sim = Simulation.new(params[0], HipArgs(devices=[0]))
        try:
            if mapped:
                sim.set_param_map(*random_map(shape, 3))
            ens = sim.make_ensemble(shape, params)
            ens.perform_steps(25)
            out.append((ens.u_views(), ens.result_views()))
            ens.destroy()
        finally:
            sim.context.close()
    assert_bits_equal(out[1][0].reshape(-1, shape[1]), out[0][0].reshape(-1, shape[1]), "ensemble U")
    assert_bits_equal(out[1][1].reshape(-1, shape[1]), out[0][1].reshape(-1, shape[1]), "ensemble V")


# ---- 6. the simulate driver end to end -------------------------------------------------------------------------------
def test_simulate_end_to_end(tmp_path):
    import oracle

    out = tmp_path / "m.h5"
    r = run_program([sys.executable, "-m", "grayscott_amd.simulate", "--hip-feed-map", "0.01:0.05", "--hip-kill-map",
                     "0.045:0.065", "-r", "64", "-c", "128", "-n", "3", "-e", "16", "-o", str(out)],
                    cwd=ROOT, limit=300)
    assert r.returncode == 0, r.stdout + r.stderr
    data = hdf5_min.read(str(out))
    assert data.shape == (3, 64, 128)
    side = json.loads(open(tmp_path / "m.param_map.json").read())
    assert side["feed"] == {"along": "rows", "from": 0.01, "to": 0.05}, side
    feed = np.repeat(R.linear(0.01, 0.05, 64)[:, None], 128, axis=1)
    kill = np.repeat(R.linear(0.045, 0.065, 128)[None, :], 64, axis=0)
    u, v = oracle.init_species(64, 128)
    for i in range(3):
        u, v = R.run(u, v, 16, feed, kill)
        assert_bits_equal(np.asarray(data[i]), v, f"image {i} (after {16 * (i + 1)} steps)")
