"""Domain masks on the MI355X (gs_ctx_set_mask): wall cells, bit for bit against the masked reference of
tests/mask_ref.py under every boundary rule, in the strict flavour and in the fused one on states without sub-normals;
every form of the marching kernel (K = 1..4, 1, 2 and 4 columns per lane, general and .op), the single-step kernels,
kernel auto at sizes that run the resident, tile and window kernels without a mask, slab chains, row bands and graph
replay; an all-fluid mask changes no bit, walls keep their bits; a sealed box stays sealed; the fluid's mass is conserved
under the zero-flux rule without reaction; the mask's lifecycle and refusals; ensembles ignore the mask; the simulate
driver end to end.  The masks go through Simulation.set_mask, which uploads 0 and 1: the values random_mask writes (1,
-3, NaN, -0) reach the device's own classification in test_caller_field_may_change_and_go only.  (Raw mask values, drawn
schedules and aimed wall layouts: tests/test_gpu_mask_property.py.  Two processes: tests/test_gpu_mask_multiprocess.py.)"""
from __future__ import annotations

import sys

import numpy as np
import pytest

from grayscott_amd import GsError, HipArgs, Parameters, Simulation, capi

from . import mask_ref as R
from .helpers import assert_bits_equal, oracle_params, rule_run, species_from_arrays, stress_fields
from tests.children import ROOT, run_program

pytestmark = pytest.mark.gpu
RULES = [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_PERIODIC, capi.GS_BOUNDARY_NEUMANN]
RULE_SUFFIX = {0: "/mask", 1: "/mask", 2: "/periodic/mask", 3: "/neumann/mask"}


def random_mask(shape, seed, share=0.25):
    """Walls (1, -3 or NaN) in about ``share`` of the cells, fluid +0 or -0.  The reference classifies these values;
    the device sees them only where a test hands the field to gs_ctx_set_mask itself (test_caller_field_may_change_and_go):
    Simulation.set_mask turns the plane into 0 and 1 on the host before it uploads it.  Raw mask values of every class on
    the device: tests/test_gpu_mask_property.py."""
    rng = np.random.default_rng(seed)
    m = np.where(rng.random(shape) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    walls = rng.random(shape) < share
    m[walls] = np.array([1.0, -3.0, np.nan], np.float32)[rng.integers(0, 3, int(walls.sum()))]
    return m


def masked_run(u0, v0, steps, mask, args, stepwise=False, calls=None, params=None):
    """upload -> set_mask -> gs_run (in `calls` pieces) or gs_step x steps -> download."""
    sim = Simulation.new(params or Parameters(), args)
    try:
        species = species_from_arrays(sim, u0, v0)
        if mask is not None:
            sim.set_mask(mask)
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
    assert ".ds" not in name and ".dx" not in name, name
    assert_bits_equal(got_u, ref[0], f"U {what} ({name})")
    assert_bits_equal(got_v, ref[1], f"V {what} ({name})")


# ---- 1. every kernel form, rule and flavour ----------------------------------------------------------------------------
TB_FORMS = [dict(cols_per_lane=c, fuse_steps=k, general_kernels=g, math=m) for c in (1, 2, 4) for k in (1, 2, 3, 4)
            for g, m in ((0, capi.GS_MATH_STRICT), (1, capi.GS_MATH_STRICT), (0, capi.GS_MATH_FUSED))]


@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("cfg", TB_FORMS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_marching_kernel_forms(cfg, boundary):
    cfg = dict(cfg)
    math = cfg.pop("math")
    for shape, seed in (((61, 263), 1), ((9, 70), 2)):
        u0, v0 = stress_fields(shape, seed)
        mask = random_mask(shape, seed + 10)
        steps = 11  # remainder passes for K = 2, 3, 4
        ref = R.run(u0, v0, steps, mask, boundary=boundary, ftz=math == capi.GS_MATH_STRICT)
        got_u, got_v, name = masked_run(u0, v0, steps, mask, HipArgs(
            devices=[0], boundary=boundary, math=math, kernel=capi.GS_KERNEL_TB, no_tune=1, **cfg))
        assert name.startswith("tb-k") and ("/fused" in name) == (math == capi.GS_MATH_FUSED), name
        if math == capi.GS_MATH_FUSED or cfg["general_kernels"]:
            assert ".op" not in name, name
        check(got_u, got_v, name, ref, boundary, f"{shape} {cfg}")


@pytest.mark.parametrize("math", [capi.GS_MATH_STRICT, capi.GS_MATH_FUSED])
@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("kernel", [capi.GS_KERNEL_SIMPLE, capi.GS_KERNEL_STREAM])
def test_single_step_kernels(kernel, boundary, math):
    for shape in ((1, 1), (1, 9), (9, 1), (7, 5), (40, 300), (33, 257)):
        u0, v0 = stress_fields(shape, 4)
        mask = random_mask(shape, 14)
        ref = R.run(u0, v0, 5, mask, boundary=boundary, ftz=math == capi.GS_MATH_STRICT)
        got_u, got_v, name = masked_run(u0, v0, 5, mask, HipArgs(devices=[0], boundary=boundary, math=math, kernel=kernel),
                                        stepwise=True)
        assert name.startswith("simple" if kernel == capi.GS_KERNEL_SIMPLE else "stream"), name
        check(got_u, got_v, name, ref, boundary, f"{shape}")


@pytest.mark.parametrize("math", [capi.GS_MATH_STRICT, capi.GS_MATH_FUSED])
@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("shape", [(1, 1), (40, 37), (256, 512), (1080, 1920)])
def test_auto_runs_the_marching_kernel_at_every_size(shape, boundary, math):
    """Sizes that run the resident, tile and window kernels without a mask; calls of 1, 2, 26 and 67 steps."""
    u0, v0 = stress_fields(shape, 5)
    mask = random_mask(shape, 15)
    calls = [1, 2, 26, 67]
    ref = R.run(u0, v0, sum(calls), mask, boundary=boundary, ftz=math == capi.GS_MATH_STRICT)
    got_u, got_v, name = masked_run(u0, v0, 0, mask, HipArgs(devices=[0], boundary=boundary, math=math), calls=calls)
    assert name.startswith("tb-k"), name
    check(got_u, got_v, name, ref, boundary, f"{shape}")


# ---- 2. an all-fluid mask changes no bit; walls keep theirs --------------------------------------------------------------
@pytest.mark.parametrize("math", [capi.GS_MATH_STRICT, capi.GS_MATH_FUSED])
@pytest.mark.parametrize("boundary", RULES)
def test_all_fluid_mask_changes_nothing(boundary, math):
    import oracle

    shape = (300, 701)
    u0, v0 = oracle.init_species(*shape)
    fluid = np.where(np.random.default_rng(3).random(shape) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    plain = masked_run(u0, v0, 37, None, HipArgs(devices=[0], boundary=boundary, math=math))
    masked = masked_run(u0, v0, 37, fluid, HipArgs(devices=[0], boundary=boundary, math=math))
    assert masked[2].split("@")[0].endswith(RULE_SUFFIX[boundary]) and "/mask" not in plain[2], (plain[2], masked[2])
    assert_bits_equal(masked[0], plain[0], f"U ({masked[2]} vs {plain[2]})")
    assert_bits_equal(masked[1], plain[1], f"V ({masked[2]} vs {plain[2]})")


@pytest.mark.parametrize("kernel", [capi.GS_KERNEL_AUTO, capi.GS_KERNEL_STREAM, capi.GS_KERNEL_SIMPLE])
def test_walls_keep_their_bits(kernel):
    """Wall cells holding NaNs with payloads, infinities and sub-normals come out as they went in; the fluid is the
    reference's (which never reads a wall's values)."""
    shape = (130, 300)
    u0, v0 = stress_fields(shape, 12)
    mask = R.maze(shape, np.random.default_rng(4))
    walls = mask != 0
    odd = np.array([0x7fc01234, 0xffc00077, 0x7f800000, 0x00000003, 0x80000005], np.uint32).view(np.float32)
    pick = np.random.default_rng(5).integers(0, odd.size, shape)
    u0 = np.where(walls, odd[pick], u0).astype(np.float32)
    v0 = np.where(walls, odd[::-1][pick], v0).astype(np.float32)
    ref = R.run(u0, v0, 9, mask)
    got_u, got_v, name = masked_run(u0, v0, 9, mask, HipArgs(devices=[0], kernel=kernel), stepwise=kernel != capi.GS_KERNEL_AUTO)
    assert got_u[walls].tobytes() == u0[walls].tobytes() and got_v[walls].tobytes() == v0[walls].tobytes(), name
    check(got_u, got_v, name, ref, 0, "walls")


# ---- 3. a sealed box; conservation --------------------------------------------------------------------------------------
def test_sealed_box_stays_sealed():
    """Fluid at U = 1, V = 0 inside a closed ring of walls keeps its bits for 2000 steps while a pattern grows outside."""
    import oracle

    shape = (256, 256)
    u0, v0 = oracle.init_species(*shape)      # the seed square sits near the centre
    ring = R.ring(shape, (60, 60), 30, 33)
    rr, cc = np.mgrid[0:shape[0], 0:shape[1]]
    inside = np.hypot(rr - 60, cc - 60) < 30
    u0[inside], v0[inside] = 1.0, 0.0
    got_u, got_v, name = masked_run(u0, v0, 2000, ring, HipArgs(devices=[0]))
    assert (got_u[inside] == 1.0).all() and (got_v[inside] == 0.0).all(), name
    outside = ~inside & (ring == 0)
    assert float(np.abs(got_v[outside] - v0[outside]).max()) > 0.1, name   # a pattern developed outside


@pytest.mark.parametrize("kernel", [capi.GS_KERNEL_AUTO, capi.GS_KERNEL_STREAM])
def test_fluid_mass_is_conserved_without_reaction(kernel):
    """Zero-flux rule, F = k = 0, the reaction term's uvv cancelling between U and V: the sum of U + V over the fluid
    cells (gs_fields_summarize, walls at 0) stays put up to rounding."""
    shape = (512, 700)
    p = Parameters(feed_rate=0.0, kill_rate=0.0)
    u0, v0 = stress_fields(shape, 13)
    mask = R.maze(shape, np.random.default_rng(6))
    u0[mask != 0], v0[mask != 0] = 0.0, 0.0
    sim = Simulation.new(p, HipArgs(devices=[0], boundary=capi.GS_BOUNDARY_NEUMANN, kernel=kernel))
    try:
        species = species_from_arrays(sim, u0, v0)
        sim.set_mask(mask)
        s0 = species.summary()
        total0 = float(s0[0].sum) + float(s0[1].sum)
        for _ in range(200 if kernel == capi.GS_KERNEL_STREAM else 4):
            if kernel == capi.GS_KERNEL_STREAM:
                sim.perform_step(species)
            else:
                sim.perform_steps(species, 50)
        s1 = species.summary()
        total1 = float(s1[0].sum) + float(s1[1].sum)
        iu, iv, _, _ = species.in_out()
        u1, v1 = iu.make_scalar_view(sim.context), iv.make_scalar_view(sim.context)
    finally:
        sim.context.close()
    assert (u1[mask != 0] == 0).all() and (v1[mask != 0] == 0).all()
    # 200 steps of f32 rounding over 358 400 cells of O(1): well below 1e-4 relative
    assert abs(total1 - total0) <= 1e-4 * abs(total0), (total0, total1)
    ref = R.run(u0, v0, 200, mask, params=oracle_params_dict(p), boundary=capi.GS_BOUNDARY_NEUMANN)
    assert_bits_equal(u1, ref[0], "U conserved run")


def oracle_params_dict(p):
    f = np.float32
    return dict(w=np.array(p.weights, np.float32), du=f(p.diffusion_rate_u), dv=f(p.diffusion_rate_v), feed=f(p.feed_rate),
                kill=f(p.kill_rate), dt=f(p.time_step))


# ---- 4. slab chains, row bands, graph replay ------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_NEUMANN])
@pytest.mark.parametrize("devices,shape", [([0, 0], (300, 701)), ([0, 0, 0], (600, 1003)), ([0, 0, 0], (11, 40))])
@pytest.mark.parametrize("kernel", [capi.GS_KERNEL_AUTO, capi.GS_KERNEL_STREAM])
def test_slab_chains(devices, shape, kernel, boundary):
    u0, v0 = stress_fields(shape, 6)
    mask = random_mask(shape, 16)
    ref = R.run(u0, v0, 11, mask, boundary=boundary)
    got_u, got_v, name = masked_run(u0, v0, 11, mask, HipArgs(devices=devices, boundary=boundary, kernel=kernel))
    check(got_u, got_v, name, ref, boundary, f"{shape} {devices}")


@pytest.mark.parametrize("boundary", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_NEUMANN])
def test_row_bands(boundary):
    shape = (1000, 1003)
    u0, v0 = stress_fields(shape, 7)
    mask = random_mask(shape, 17)
    ref = R.run(u0, v0, 13, mask, boundary=boundary)
    got_u, got_v, name = masked_run(u0, v0, 13, mask, HipArgs(devices=[0], boundary=boundary, split=2))
    check(got_u, got_v, name, ref, boundary, "split 2")


# ---- 5. lifecycle -------------------------------------------------------------------------------------------------------
SKEWED = Parameters(weights=((0.25, 0.5, 0.125), (1.0, 0.5, 0.25), (0.0, 0.125, 0.5)), time_step=0.5)


@pytest.mark.parametrize("use_graph", [0, 1])
@pytest.mark.parametrize("boundary", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_PERIODIC])
def test_attach_replace_detach_set_params(use_graph, boundary):
    """Each phase continues from the state the last one left; a stale graph, link plane or tuning would show in the bits.
    set_params with a mask attached switches between the .op and the general form."""
    shape = (300, 701)
    default = Parameters()
    u0, v0 = stress_fields(shape, 8)
    masks = [random_mask(shape, 18), random_mask(shape, 19, share=0.5)]
    sim = Simulation.new(default, HipArgs(devices=[0], boundary=boundary, use_graph=use_graph, fuse_steps=4))
    try:
        species = species_from_arrays(sim, u0, v0)
        ref = (u0, v0)
        for phase, mask, p in (("mask0", 0, default), ("mask1", 1, default), ("skewed", 1, SKEWED), ("none", None, SKEWED),
                               ("mask0 again", 0, default)):
            if phase == "none":
                sim.clear_mask()
            elif phase != "skewed":
                sim.set_mask(masks[mask])
            sim.context.set_params(p)
            sim.perform_steps(species, 70)  # 17 passes + 2: graph batches of 16 passes and a remainder
            if mask is None:
                ref = rule_run(ref[0], ref[1], 70, params=oracle_params(p), boundary=boundary)
            else:
                ref = R.run(ref[0], ref[1], 70, masks[mask], params=oracle_params_dict(p), boundary=boundary)
            iu, iv, _, _ = species.in_out()
            name = sim.context.info()[0]
            assert name.split("@")[0].endswith("/mask") == (mask is not None), (phase, name)
            if mask is not None:
                assert (".op" in name) == (p is default), (phase, name)
            assert_bits_equal(iu.make_scalar_view(sim.context), ref[0], f"U after {phase} ({name})")
            assert_bits_equal(iv.make_scalar_view(sim.context), ref[1], f"V after {phase} ({name})")
    finally:
        sim.context.close()


def test_caller_field_may_change_and_go():
    """The library copies the mask: the caller's field is overwritten, then destroyed, before the steps run."""
    from grayscott_amd import HipConcentration

    shape = (64, 300)
    u0, v0 = stress_fields(shape, 9)
    mask = random_mask(shape, 20)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    try:
        ctx = sim.context
        species = species_from_arrays(sim, u0, v0)
        c = HipConcentration(ctx, shape)
        c.upload(ctx, mask)
        capi.check(ctx._lib.gs_ctx_set_mask(ctx.handle, c.handle))
        c.upload(ctx, np.zeros(shape, np.float32))
        c.destroy()
        sim.perform_steps(species, 23)
        iu, iv, _, _ = species.in_out()
        ref = R.run(u0, v0, 23, mask)
        check(iu.make_scalar_view(ctx), iv.make_scalar_view(ctx), ctx.info()[0], ref, 0, "after the caller's field went")
    finally:
        sim.context.close()


def test_tuned_choices_of_the_mask_set():
    shape = (200, 300)
    u0, v0 = stress_fields(shape, 11)
    mask = random_mask(shape, 24)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], kernel=capi.GS_KERNEL_TB, no_tune=1))
    try:
        ctx = sim.context
        ctx.set_tuned(shape[0], shape[1], 8, 3, 2)
        uniform = ctx.get_tuned(*shape)
        sim.set_mask(mask)
        assert ctx.get_tuned(*shape) == (0, 0, 0, 0)   # nothing chosen for the mask's kernels yet
        ctx.set_tuned(shape[0], shape[1], 16, 2, 1)
        masked = ctx.get_tuned(*shape)
        species = species_from_arrays(sim, u0, v0)
        sim.perform_steps(species, 9)
        assert ctx.info()[0].startswith("tb-k2c1/"), ctx.info()
        iu, iv, _, _ = species.in_out()
        check(iu.make_scalar_view(ctx), iv.make_scalar_view(ctx), ctx.info()[0], R.run(u0, v0, 9, mask), 0, "tuned")
        sim.clear_mask()
        assert ctx.get_tuned(*shape) == uniform
        sim.set_mask(mask)
        assert ctx.get_tuned(*shape) == masked
        # ... and a parameter map's kernels keep a third choice on the same context: map attached -> detached -> mask
        # attached -> detached, each set answering with its own
        sim.clear_mask()
        rates = np.full(shape, 0.03, np.float32), np.full(shape, 0.06, np.float32)
        sim.set_param_map(*rates)
        assert ctx.get_tuned(*shape) == (0, 0, 0, 0)   # nothing chosen for the map's kernels yet
        ctx.set_tuned(shape[0], shape[1], 12, 4, 4)
        mapped = ctx.get_tuned(*shape)
        assert len({uniform, masked, mapped}) == 3
        sim.clear_param_map()
        assert ctx.get_tuned(*shape) == uniform
        sim.set_mask(mask)
        assert ctx.get_tuned(*shape) == masked
        sim.clear_mask()
        assert ctx.get_tuned(*shape) == uniform
        sim.set_param_map(*rates)
        assert ctx.get_tuned(*shape) == mapped
    finally:
        sim.context.close()


# ---- 6. refusals; ensembles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [capi.GS_KERNEL_WINDOW, capi.GS_KERNEL_LDS, capi.GS_KERNEL_TILE])
def test_pinned_kernels_without_a_mask_form_are_refused(kernel):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], kernel=kernel))
    try:
        with pytest.raises(GsError) as e:
            sim.set_mask(np.zeros((64, 300), np.float32))
        assert e.value.code == capi.GS_ERR_UNSUPPORTED
    finally:
        sim.context.close()


def test_shape_mismatch_and_map_together_are_refused():
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    try:
        u0, v0 = stress_fields((64, 300), 1)
        species = species_from_arrays(sim, u0, v0)
        sim.set_mask(np.zeros((32, 300), np.float32))
        with pytest.raises(GsError) as e:
            sim.perform_steps(species, 3)
        assert e.value.code == capi.GS_ERR_INVALID
        with pytest.raises(GsError) as e:
            sim.perform_step(species)
        assert e.value.code == capi.GS_ERR_INVALID
        sim.set_mask(np.zeros((64, 300), np.float32))
        with pytest.raises(GsError) as e:
            sim.set_param_map(0.03, 0.06, shape=(64, 300))
        assert e.value.code == capi.GS_ERR_UNSUPPORTED and "mask" in str(e.value) and "map" in str(e.value)
        sim.clear_mask()
        sim.set_param_map(0.03, 0.06, shape=(64, 300))
        with pytest.raises(GsError) as e:
            sim.set_mask(np.zeros((64, 300), np.float32))
        assert e.value.code == capi.GS_ERR_UNSUPPORTED and "mask" in str(e.value) and "map" in str(e.value)
        sim.clear_param_map()
        sim.set_mask(np.zeros((64, 300), np.float32))
        sim.perform_steps(species, 3)
    finally:
        sim.context.close()


def test_ensembles_ignore_the_mask():
    shape = (37, 53)
    params = [Parameters(feed_rate=0.03, kill_rate=0.06), Parameters(feed_rate=0.022, kill_rate=0.051)]
    out = []
    for masked in (False, True):
        sim = Simulation.new(params[0], HipArgs(devices=[0]))
        try:
            if masked:
                sim.set_mask(random_mask(shape, 3))
            ens = sim.make_ensemble(shape, params)
            ens.perform_steps(25)
            out.append((ens.u_views(), ens.result_views()))
            ens.destroy()
        finally:
            sim.context.close()
    assert_bits_equal(out[1][0].reshape(-1, shape[1]), out[0][0].reshape(-1, shape[1]), "ensemble U")
    assert_bits_equal(out[1][1].reshape(-1, shape[1]), out[0][1].reshape(-1, shape[1]), "ensemble V")


# ---- 7. the simulate driver ---------------------------------------------------------------------------------------------
def test_simulate_with_a_mask(tmp_path):
    import oracle

    rows, cols, images, extra = 120, 200, 3, 7
    mask = R.maze((rows, cols), np.random.default_rng(8))
    np.save(tmp_path / "m.npy", mask)
    out = tmp_path / "out.npy"
    r = run_program([sys.executable, "-m", "grayscott_amd.simulate", "-r", str(rows), "-c", str(cols), "-n", str(images),
                     "-e", str(extra), "-o", str(out), "--hip-devices", "0", "--hip-mask", str(tmp_path / "m.npy")],
                    cwd=ROOT, limit=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    u, v = oracle.init_species(rows, cols)
    for i in range(images):
        u, v = R.run(u, v, extra, mask)
        assert_bits_equal(got[i], v, f"image {i}")
