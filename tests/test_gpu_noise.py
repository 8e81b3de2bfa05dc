"""The noise term on the MI355X (gs_ctx_set_noise): seeded stochastic steps, every word of U and V against the restatement
of tests/noise_ref.py under every boundary rule and in both flavours; every form of the marching kernel (K = 1..4, 1, 2 and
4 columns per lane, general and .op), the simple and streaming kernels, kernel = auto at every size, the bare noise field,
one and both sigmas zero against the uniform run, the step counter over calls, species and replays, slab chains and row
bands (global rows across seams), the refusals, ensembles, and the simulate driver end to end."""
from __future__ import annotations

import functools
import sys

import numpy as np
import pytest

from grayscott_amd import GsError, HipArgs, Parameters, Simulation, capi, hdf5_min

from . import noise_ref as N
from .helpers import assert_bits_equal, species_from_arrays, stress_fields
from tests.children import ROOT, run_program

pytestmark = pytest.mark.gpu
RULES = [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_PERIODIC, capi.GS_BOUNDARY_NEUMANN]
RULE_SUFFIX = {0: "/noise", 1: "/noise", 2: "/periodic/noise", 3: "/neumann/noise"}
STRICT, FUSED = capi.GS_MATH_STRICT, capi.GS_MATH_FUSED
NOISE = dict(sigma_u=0.02, sigma_v=0.01, seed=0x1234567890ABCDEF, step=0)


def planted_fields(shape, seed, subnormals):
    """Stress fields with signed zeros and -- for the strict flavour, whose contract covers them -- sub-normals planted in
    about a sixth of the cells."""
    u, v = stress_fields(shape, seed)
    rng = np.random.default_rng(seed + 1000)
    values = [0.0, -0.0] + ([1e-39, -1e-39, 1.1754942e-38, -3e-45] if subnormals else [])
    values = np.array(values, np.float32)
    for x in (u, v):
        where = rng.random(shape) < 0.17
        x[where] = values[rng.integers(0, len(values), shape)[where]]
    return u, v


def noisy_run(u0, v0, args, noise, calls=(), stepwise=0, params=None):
    """upload -> set_noise -> gs_run in `calls` pieces, then `stepwise` gs_steps -> download, the name, noise()."""
    sim = Simulation.new(params or Parameters(), args)
    try:
        species = species_from_arrays(sim, u0, v0)
        if noise is not None:
            sim.set_noise(**noise)
        for n in calls:
            sim.perform_steps(species, n)
        for _ in range(stepwise):
            sim.perform_step(species)
        iu, iv, _, _ = species.in_out()
        return iu.make_scalar_view(sim.context), iv.make_scalar_view(sim.context), sim.context.info()[0], sim.noise()
    finally:
        sim.context.close()


@functools.lru_cache(maxsize=None)
def reference(shape, seed, steps, rule, ftz):
    """The restatement's result for planted_fields(shape, seed, ftz) under NOISE, computed once and shared."""
    u0, v0 = planted_fields(shape, seed, ftz)
    u, v = N.run(u0, v0, steps, NOISE, rule=rule, ftz=ftz)
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


def check(got_u, got_v, name, ref, rule, what):
    assert name.split("@")[0].endswith(RULE_SUFFIX[rule]), (name, what)
    assert_bits_equal(got_u, ref[0], f"U {what} ({name})")
    assert_bits_equal(got_v, ref[1], f"V {what} ({name})")


# ---- 1. every marching form, rule and flavour -------------------------------------------------------------------------
# strict: the .op variant (default weights) and the general one; fused: the general one (it has no .op variant)
TB_FORMS = [dict(cols_per_lane=c, fuse_steps=k, general_kernels=g, math=m) for c in (1, 2, 4) for k in (1, 2, 3, 4)
            for g, m in ((0, STRICT), (1, STRICT), (0, FUSED))]


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("cfg", TB_FORMS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_marching_kernel_forms(cfg, rule):
    cfg = dict(cfg)
    math = cfg.pop("math")
    for shape, seed in (((61, 263), 1), ((9, 70), 2)):
        steps = 7  # a 4 + 3 pass split at K = 4
        u0, v0 = planted_fields(shape, seed, math == STRICT)
        got_u, got_v, name, after = noisy_run(u0, v0, HipArgs(devices=[0], boundary=rule, math=math, kernel=capi.GS_KERNEL_TB,
                                                               no_tune=1, **cfg), NOISE, calls=[steps])
        assert name.startswith(f"tb-k") and ("/fused" in name) == (math == FUSED), name
        assert (".op" in name) == (math == STRICT and not cfg["general_kernels"]), name
        assert after["step"] == steps
        check(got_u, got_v, name, reference(shape, seed, steps, rule, math == STRICT), rule, f"{shape} {cfg}")


@pytest.mark.parametrize("math", [STRICT, FUSED])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("kernel", [capi.GS_KERNEL_SIMPLE, capi.GS_KERNEL_STREAM])
def test_single_step_kernels(kernel, rule, math):
    for shape in ((1, 1), (7, 5), (40, 300), (33, 257)):
        u0, v0 = planted_fields(shape, 4, math == STRICT)
        got_u, got_v, name, _ = noisy_run(u0, v0, HipArgs(devices=[0], boundary=rule, math=math, kernel=kernel), NOISE, stepwise=5)
        assert name.startswith("simple" if kernel == capi.GS_KERNEL_SIMPLE else "stream"), name
        check(got_u, got_v, name, reference(shape, 4, 5, rule, math == STRICT), rule, f"{shape}")


@pytest.mark.parametrize("math", [STRICT, FUSED])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("shape", [(1, 1), (40, 37), (256, 512), (1080, 1920)])
def test_auto_runs_the_marching_kernel_at_every_size(shape, rule, math):
    """Sizes that run the resident, tile and window kernels without noise; 9 steps.  The largest is compared with a replay by
    the streaming kernel instead of numpy."""
    u0, v0 = planted_fields(shape, 5, math == STRICT)
    got_u, got_v, name, _ = noisy_run(u0, v0, HipArgs(devices=[0], boundary=rule, math=math), NOISE, calls=[9])
    assert name.startswith("tb-k"), name
    if shape == (1080, 1920):
        ru, rv, rname, _ = noisy_run(u0, v0, HipArgs(devices=[0], boundary=rule, math=math, kernel=capi.GS_KERNEL_STREAM), NOISE,
                                     stepwise=9)
        assert rname.startswith("stream"), rname
        ref = (ru, rv)
    else:
        ref = reference(shape, 5, 9, rule, math == STRICT)
    check(got_u, got_v, name, ref, rule, f"{shape}")


# ---- 2. the bare field, zero sigmas -----------------------------------------------------------------------------------
@pytest.mark.parametrize("math", [STRICT, FUSED])
@pytest.mark.parametrize("kernel", [capi.GS_KERNEL_AUTO, capi.GS_KERNEL_STREAM, capi.GS_KERNEL_SIMPLE])
@pytest.mark.parametrize("sigmas", [(0.5, 0.25), (1e-38, 3e-39)])
def test_the_bare_noise_field(kernel, math, sigmas):
    """du = dv = F = k = 0 and U = V = 0: one step leaves exactly sigma * xi -- flushed where the product is sub-normal in
    the strict flavour."""
    import oracle

    shape = (37, 300)
    p = Parameters(diffusion_rate_u=0.0, diffusion_rate_v=0.0, feed_rate=0.0, kill_rate=0.0)
    zero = np.zeros(shape, np.float32)
    noise = dict(sigma_u=sigmas[0], sigma_v=sigmas[1], seed=77, step=2 ** 32 + 5)
    calls, stepwise = ([1], 0) if kernel == capi.GS_KERNEL_AUTO else ([], 1)
    got_u, got_v, name, after = noisy_run(zero, zero, HipArgs(devices=[0], math=math, kernel=kernel), noise, calls=calls,
                                          stepwise=stepwise, params=p)
    x0, x1 = N.draws(shape, 77, 2 ** 32 + 5)
    prev = oracle.set_ftz(math == STRICT)
    try:
        want_u = np.float32(0) + np.float32(sigmas[0]) * N.xi(x0)
        want_v = np.float32(0) + np.float32(sigmas[1]) * N.xi(x1)
    finally:
        oracle.set_ftz(prev)
    assert after["step"] == 2 ** 32 + 6
    check(got_u, got_v, name, (want_u, want_v), 0, f"{sigmas}")


def special_fields(shape, seed):
    """Stress fields that hold -0 and NaNs."""
    u, v = planted_fields(shape, seed, True)
    u[3, 5], v[7, 11] = np.nan, np.nan
    u[0, 0], v[shape[0] - 1, shape[1] - 1] = -0.0, -0.0
    return u, v


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("which", ["u", "v"])
def test_one_sigma_zero_leaves_that_species_alone(which, rule):
    """The species whose sigma is 0 is the reference step's bit for bit -- on a plane with -0 and NaNs, over ONE step, where
    the other species' noise has not reached it yet: it equals the uniform run's."""
    shape = (40, 300)
    u0, v0 = special_fields(shape, 12)
    noise = dict(sigma_u=0.0 if which == "u" else 0.03, sigma_v=0.0 if which == "v" else 0.03, seed=5, step=0)
    for kernel, calls, stepwise in ((capi.GS_KERNEL_TB, [1], 0), (capi.GS_KERNEL_STREAM, [], 1)):
        args = dict(devices=[0], boundary=rule, kernel=kernel)
        nu, nv, name, _ = noisy_run(u0, v0, HipArgs(**args), noise, calls=calls, stepwise=stepwise)
        pu, pv, pname, _ = noisy_run(u0, v0, HipArgs(**args), None, calls=calls, stepwise=stepwise)
        assert name.split("@")[0].endswith(RULE_SUFFIX[rule]) and "/noise" not in pname, (name, pname)
        got, plain, other, other_plain = (nu, pu, nv, pv) if which == "u" else (nv, pv, nu, pu)
        assert_bits_equal(got, plain, f"{which} with sigma 0 ({name} vs {pname})")
        assert other.tobytes() != other_plain.tobytes()


@pytest.mark.parametrize("math", [STRICT, FUSED])
@pytest.mark.parametrize("rule", RULES)
def test_both_sigmas_zero_is_the_uniform_run(rule, math):
    import oracle

    shape = (300, 701)
    u0, v0 = oracle.init_species(*shape)
    noise = dict(sigma_u=0.0, sigma_v=0.0, seed=9, step=3)
    nu, nv, name, after = noisy_run(u0, v0, HipArgs(devices=[0], boundary=rule, math=math), noise, calls=[37])
    pu, pv, pname, none = noisy_run(u0, v0, HipArgs(devices=[0], boundary=rule, math=math), None, calls=[37])
    assert after == dict(sigma_u=0.0, sigma_v=0.0, seed=9, step=40) and none is None
    assert name.split("@")[0].endswith(RULE_SUFFIX[rule]) and "/noise" not in pname, (name, pname)
    assert_bits_equal(nu, pu, f"U ({name} vs {pname})")
    assert_bits_equal(nv, pv, f"V ({name} vs {pname})")


# ---- 3. the counter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_PERIODIC])
def test_the_counter_over_calls(rule):
    shape = (61, 263)
    u0, v0 = planted_fields(shape, 1, True)
    ref = reference(shape, 1, 7, rule, True)
    args = dict(devices=[0], boundary=rule)
    for what, calls, stepwise in (("7", [7], 0), ("3 + 4", [3, 4], 0), ("2 + 1 + 3, then a gs_step", [2, 1, 3], 1), ("gs_step x 7", [], 7)):
        got_u, got_v, name, after = noisy_run(u0, v0, HipArgs(**args), NOISE, calls=calls, stepwise=stepwise)
        assert after == dict(NOISE, sigma_u=float(np.float32(NOISE["sigma_u"])), sigma_v=float(np.float32(NOISE["sigma_v"])),
                             step=NOISE["step"] + 7), (what, after)
        check(got_u, got_v, name, ref, rule, what)
    # gs_step between two gs_run calls
    sim = Simulation.new(Parameters(), HipArgs(**args))
    try:
        species = species_from_arrays(sim, u0, v0)
        sim.set_noise(**NOISE)
        sim.perform_steps(species, 3)
        sim.perform_step(species)
        sim.perform_steps(species, 3)
        iu, iv, _, _ = species.in_out()
        assert sim.noise()["step"] == 7
        check(iu.make_scalar_view(sim.context), iv.make_scalar_view(sim.context), sim.context.info()[0], ref, rule, "3, step, 3")
    finally:
        sim.context.close()


def test_replay_from_a_snapshot():
    """Snapshot, run, restore, set_noise with the saved struct, run again: the same bits; and an earlier step replays."""
    shape = (100, 300)
    u0, v0 = planted_fields(shape, 3, True)
    noise = dict(sigma_u=0.02, sigma_v=0.01, seed=42, step=2 ** 40)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    try:
        ctx = sim.context
        species = species_from_arrays(sim, u0, v0)
        sim.set_noise(**noise)
        sim.perform_steps(species, 6)
        saved = sim.noise()
        assert saved["step"] == 2 ** 40 + 6
        iu, iv, _, _ = species.in_out()
        snap = iu.make_scalar_view(ctx), iv.make_scalar_view(ctx)
        sim.perform_steps(species, 9)
        iu, iv, _, _ = species.in_out()
        first = iu.make_scalar_view(ctx), iv.make_scalar_view(ctx)
        again = species_from_arrays(sim, *snap)
        sim.set_noise(**saved)
        sim.perform_steps(again, 9)
        iu, iv, _, _ = again.in_out()
        assert_bits_equal(iu.make_scalar_view(ctx), first[0], "U replayed")
        assert_bits_equal(iv.make_scalar_view(ctx), first[1], "V replayed")
        assert sim.noise()["step"] == 2 ** 40 + 15
        ref = N.run(u0, v0, 15, noise)
        assert_bits_equal(first[0], ref[0], "U against the restatement")
        assert_bits_equal(first[1], ref[1], "V against the restatement")
        sim.clear_noise()
        assert sim.noise() is None
    finally:
        sim.context.close()


def test_several_species_share_the_counter():
    """The counter is the context's: a second Species' steps advance it too."""
    shape = (40, 300)
    a0, b0 = planted_fields(shape, 6, True), planted_fields(shape, 7, True)
    noise = dict(NOISE, step=10)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    try:
        ctx = sim.context
        a, b = species_from_arrays(sim, *a0), species_from_arrays(sim, *b0)
        sim.set_noise(**noise)
        sim.perform_steps(a, 3)    # steps 10, 11, 12
        sim.perform_steps(b, 2)    # 13, 14
        sim.perform_step(a)        # 15
        sim.perform_steps(b, 4)    # 16 .. 19
        assert sim.noise()["step"] == 20
        ra = N.run(*N.run(*a0, 3, dict(noise, step=10)), 1, dict(noise, step=15))
        rb = N.run(*N.run(*b0, 2, dict(noise, step=13)), 4, dict(noise, step=16))
        for sp, ref, what in ((a, ra, "first species"), (b, rb, "second species")):
            iu, iv, _, _ = sp.in_out()
            assert_bits_equal(iu.make_scalar_view(ctx), ref[0], f"U of the {what}")
            assert_bits_equal(iv.make_scalar_view(ctx), ref[1], f"V of the {what}")
    finally:
        sim.context.close()


# ---- 4. slab chains and row bands: global rows across seams -----------------------------------------------------------
@pytest.mark.parametrize("rule", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_NEUMANN])
@pytest.mark.parametrize("devices,shape", [([0, 0], (300, 701)), ([0, 0, 0], (11, 40))])
@pytest.mark.parametrize("kernel", [capi.GS_KERNEL_AUTO, capi.GS_KERNEL_STREAM])
def test_slab_chains(devices, shape, kernel, rule):
    u0, v0 = planted_fields(shape, 6, True)
    got_u, got_v, name, after = noisy_run(u0, v0, HipArgs(devices=devices, boundary=rule, kernel=kernel), NOISE, calls=[11])
    assert after["step"] == 11
    check(got_u, got_v, name, reference(shape, 6, 11, rule, True), rule, f"{shape} {devices}")


@pytest.mark.parametrize("rule", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_NEUMANN])
def test_row_bands(rule):
    shape = (1000, 1003)
    u0, v0 = planted_fields(shape, 7, True)
    got_u, got_v, name, _ = noisy_run(u0, v0, HipArgs(devices=[0], boundary=rule, split=2), NOISE, calls=[13])
    check(got_u, got_v, name, reference(shape, 7, 13, rule, True), rule, "split 2")


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
def refused(call, code, *words):
    with pytest.raises(GsError) as e:
        call()
    assert e.value.code == code, (e.value.code, e.value.message)
    for w in words:
        assert w in e.value.message, (w, e.value.message)


def test_refusals():
    shape = (40, 300)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    try:
        for su, sv in ((float("nan"), 0.0), (0.0, float("inf")), (-0.01, 0.0), (0.0, -1.0), (float("-inf"), 0.0)):
            refused(lambda: sim.set_noise(su, sv), capi.GS_ERR_INVALID)
            assert sim.noise() is None
        sim.set_noise(0.0, 0.0)                                # legal, and it stays attached
        assert sim.noise() == dict(sigma_u=0.0, sigma_v=0.0, seed=0, step=0)
        refused(lambda: sim.set_param_map(0.03, 0.06, shape=shape), capi.GS_ERR_UNSUPPORTED, "parameter map", "noise term")
        refused(lambda: sim.set_mask(np.zeros(shape, np.float32)), capi.GS_ERR_UNSUPPORTED, "domain mask", "noise term")
        sim.clear_noise()
        sim.set_param_map(0.03, 0.06, shape=shape)
        refused(lambda: sim.set_noise(0.1), capi.GS_ERR_UNSUPPORTED, "noise term", "parameter map")
        sim.clear_param_map()
        sim.set_mask(np.zeros(shape, np.float32))
        refused(lambda: sim.set_noise(0.1), capi.GS_ERR_UNSUPPORTED, "noise term", "domain mask")
        sim.clear_mask()
        sim.set_noise(0.1, seed=3)                             # ... and with both gone it attaches
        assert sim.noise()["seed"] == 3
    finally:
        sim.context.close()
    for kernel in (capi.GS_KERNEL_WINDOW, capi.GS_KERNEL_LDS, capi.GS_KERNEL_TILE):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0], kernel=kernel))
        try:
            refused(lambda: sim.set_noise(0.1), capi.GS_ERR_UNSUPPORTED, "noise")
        finally:
            sim.context.close()
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], use_graph=1))
    try:
        refused(lambda: sim.set_noise(0.1), capi.GS_ERR_UNSUPPORTED, "use_graph")
        assert sim.noise() is None
    finally:
        sim.context.close()


def test_ensembles_ignore_the_noise():
    shape = (37, 53)
    params = [Parameters(feed_rate=0.03, kill_rate=0.06), Parameters(feed_rate=0.022, kill_rate=0.051)]
    out = []
    for noisy in (False, True):
        sim = Simulation.new(params[0], HipArgs(devices=[0]))
        try:
            if noisy:
                sim.set_noise(0.1, 0.1, seed=1)
            ens = sim.make_ensemble(shape, params)
            ens.perform_steps(25)
            out.append((ens.u_views(), ens.result_views()))
            ens.destroy()
            if noisy:
                assert sim.noise()["step"] == 0
        finally:
            sim.context.close()
    assert_bits_equal(out[1][0].reshape(-1, shape[1]), out[0][0].reshape(-1, shape[1]), "ensemble U")
    assert_bits_equal(out[1][1].reshape(-1, shape[1]), out[0][1].reshape(-1, shape[1]), "ensemble V")


# ---- 6. the simulate driver end to end --------------------------------------------------------------------------------
def test_simulate_end_to_end(tmp_path):
    import oracle

    files = []
    for name in ("a.h5", "b.h5"):
        out = tmp_path / name
        r = run_program([sys.executable, "-m", "grayscott_amd.simulate", "--hip-noise", "0.02:0.005", "--hip-noise-seed", "12345",
                         "--hip-noise-step", "7", "-r", "64", "-c", "128", "-n", "3", "-e", "16", "-o", str(out)], cwd=ROOT, limit=300)
        assert r.returncode == 0, r.stdout + r.stderr
        files.append(out)
    data = hdf5_min.read(str(files[0]))
    assert data.shape == (3, 64, 128)
    noise = dict(sigma_u=0.02, sigma_v=0.005, seed=12345, step=7)
    u, v = oracle.init_species(64, 128)
    for i in range(3):
        u, v = N.run(u, v, 16, dict(noise, step=7 + 16 * i))
        assert_bits_equal(np.asarray(data[i]), v, f"image {i} (after {16 * (i + 1)} steps)")
    assert open(files[0], "rb").read() == open(files[1], "rb").read()
    # ... and the flags are refused together with a map, with the library's message
    r = run_program([sys.executable, "-m", "grayscott_amd.simulate", "--hip-noise", "0.02", "--hip-feed-map", "0.01:0.05", "-r", "64",
                     "-c", "128", "-n", "1", "-e", "4", "-o", str(tmp_path / "c.h5")], cwd=ROOT, limit=300)
    assert r.returncode != 0 and "cannot be attached together" in r.stdout + r.stderr, r.stdout + r.stderr
