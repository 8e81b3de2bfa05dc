"""Reduced result images on the device (gs_field_download_reduced, _reduced_async, gs_field_colormap_reduced) against the
numpy restatement of their definition (tests/reduce_ref.py), bit for bit (NaN pixels by position): every factor and
shape, one slab and slab chains, every producer kernel and boundary rule, the overlapped form as a snapshot, behind
window launches and after a launch that gave up, colour mapping, and the driver's --hip-image-reduce."""
import numpy as np
import pytest

import oracle
from grayscott_amd import HipArgs, Parameters, Simulation, capi
from grayscott_amd import simulate as driver
from grayscott_amd.simulation import HipConcentration, pinned_empty
from oracle import colormap_ref
from tests import reduce_ref
from tests.helpers import species_from_arrays, stress_fields

pytestmark = pytest.mark.gpu

FACTORS = (2, 3, 4, 5, 8, 16, 64)
SHAPES = [(16, 32), (301, 517), (1080, 1920), (2048, 4096)]
RULES = {"clipped": capi.GS_BOUNDARY_CLIPPED, "zero_halo": capi.GS_BOUNDARY_ZERO_HALO,
         "periodic": capi.GS_BOUNDARY_PERIODIC, "neumann": capi.GS_BOUNDARY_NEUMANN}


def assert_image(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    if not reduce_ref.same_bits(got, want):
        gn, wn = np.isnan(got), np.isnan(want)
        bad = np.argwhere((gn != wn) | (~gn & ~wn & (got.view(np.uint32) != want.view(np.uint32))))
        r, c = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} pixels differ; first at ({r},{c}): got {got[r, c]!r}, want {want[r, c]!r}")


def check_plane(sim, field, plane, slabs, what):
    """Every factor on `field` (which holds `plane`): blocking and overlapped against the restatement where the slab rule
    admits the pair, GS_ERR_UNSUPPORTED (and a context that goes on working) where it does not."""
    ctx = sim.context
    rows, cols = plane.shape
    for f in FACTORS:
        if not reduce_ref.slab_rule(rows, slabs, f):
            bad = next(r0 for r0 in reduce_ref.slab_starts(rows, slabs) if r0 % f)
            for call in (lambda: field.reduced_shape(f), lambda: field.make_scalar_view(ctx, reduce=f),
                         lambda: field.write_scalar_view_after(ctx, pinned_empty((1, 1)), reduce=f),
                         lambda: field.colormap(ctx, np.zeros((4, 3), np.uint8), reduce=f)):
                with pytest.raises(capi.GsError) as e:
                    call()
                assert e.value.code == capi.GS_ERR_UNSUPPORTED, (what, f, e.value)
                assert str(bad) in e.value.message and str(f) in e.value.message, e.value.message
            continue
        want = reduce_ref.reduce(plane, f)
        assert field.reduced_shape(f) == want.shape == reduce_ref.shape(rows, cols, f)
        assert_image(field.make_scalar_view(ctx, reduce=f), want, f"{what}, blocking, f = {f}")
        image = pinned_empty(want.shape)
        image[...] = -7.0
        field.write_scalar_view_after(ctx, image, reduce=f)
        ctx.download_wait()
        assert_image(np.array(image), want, f"{what}, overlapped, f = {f}")
    # the context is as usable as before (refusals included): the plane itself comes back
    assert field.make_scalar_view(ctx).tobytes() == plane.tobytes(), what
    assert field.make_scalar_view(ctx, reduce=1).tobytes() == plane.tobytes(), what


@pytest.mark.parametrize("slabs", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_random_planes_with_special_values(built, shape, slabs):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * slabs, place_candidates=0))
    u0, v0 = reduce_ref.special_plane(shape, 1), reduce_ref.special_plane(shape, 2)
    species = species_from_arrays(sim, u0, v0)
    in_u, in_v, _, _ = species.in_out()
    check_plane(sim, in_u, u0, slabs, f"U {shape} on {slabs} slabs")
    check_plane(sim, in_v, v0, slabs, f"V {shape} on {slabs} slabs")
    sim.context.close()


@pytest.mark.parametrize("slabs", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_developed_pattern(built, shape, slabs):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * slabs, place_candidates=0))
    species = sim.make_species(shape)
    sim.perform_steps(species, 300)
    in_u, in_v, _, _ = species.in_out()
    v = in_v.make_scalar_view(sim.context)
    assert np.isfinite(v).all()
    check_plane(sim, in_v, v, slabs, f"V after 300 steps, {shape} on {slabs} slabs")
    f = next((f for f in FACTORS if reduce_ref.slab_rule(shape[0], slabs, f)), 1)   # (2048 rows on 3 slabs admit none)
    want = reduce_ref.reduce(v, f)
    assert_image(species.make_result_view(reduce=f), want, "Species.make_result_view")
    target = np.empty(want.shape, np.float32)
    species.write_result_view(target, reduce=f)
    assert_image(target, want, "Species.write_result_view")
    sim.context.close()


def test_bad_arguments(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    species = sim.make_species([40, 50])
    v = species.in_out()[1]
    for f in (0, -1, 65, 1000):
        for call in (lambda: v.reduced_shape(f), lambda: v.make_scalar_view(ctx, reduce=f)):
            with pytest.raises(capi.GsError) as e:
                call()
            assert e.value.code == capi.GS_ERR_INVALID
    lib = ctx._lib
    out = np.zeros((20, 25), np.float32)
    ptr = out.ctypes.data
    assert lib.gs_field_download_reduced(other.context.handle, v.handle, 2, ptr) == capi.GS_ERR_INVALID    # a foreign handle
    assert lib.gs_field_download_reduced_async(other.context.handle, v.handle, 2, ptr) == capi.GS_ERR_INVALID
    assert lib.gs_field_colormap_reduced(other.context.handle, v.handle, 2, 2.0, ptr, 1, ptr) == capi.GS_ERR_INVALID
    assert lib.gs_field_download_reduced(ctx.handle, v.handle, 2, None) == capi.GS_ERR_INVALID
    # a target of the wrong shape: ValueError, nothing enqueued
    for bad in (np.zeros((20, 26), np.float32), np.zeros((40, 50), np.float32), np.zeros((20, 25), np.float64)):
        with pytest.raises(ValueError):
            v.write_scalar_view(ctx, bad, reduce=2)
        with pytest.raises(ValueError):
            v.write_scalar_view_after(ctx, bad, reduce=2)
        with pytest.raises(ValueError):
            species.write_result_view_after(bad, reduce=2)
    # an empty field: GS_OK, nothing written
    empty = Simulation.new(Parameters(), HipArgs(devices=[0]))
    e = HipConcentration(empty.context, (0, 7))
    assert e.reduced_shape(4) == (0, 2)
    assert e.make_scalar_view(empty.context, reduce=4).shape == (0, 2)
    assert lib.gs_field_download_reduced_async(empty.context.handle, e.handle, 4, None) == capi.GS_OK
    for s in (sim, other, empty):
        s.context.close()


@pytest.mark.parametrize("rule", sorted(RULES))
def test_the_producer_does_not_matter(built, rule):
    """The same state reached with the marching, streaming, LDS-window (resident / tile) and persistent window kernels:
    the same planes, and every reduced image equals the restatement of the downloaded plane."""
    shape, steps = (1080, 1920), 40
    u0, v0 = stress_fields(shape, 9)
    planes, ran = {}, []
    for name, kernel in (("marching", capi.GS_KERNEL_TB), ("streaming", capi.GS_KERNEL_STREAM), ("tile", capi.GS_KERNEL_TILE),
                         ("window", capi.GS_KERNEL_WINDOW), ("auto", capi.GS_KERNEL_AUTO)):
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
        in_u, in_v, _, _ = species.in_out()
        for what, field in (("U", in_u), ("V", in_v)):
            plane = field.make_scalar_view(sim.context)
            planes.setdefault(what, plane)
            assert plane.tobytes() == planes[what].tobytes(), f"{what} of the {name} kernel ({sim.context.info()[0]}) under {rule}"
            for f in (3, 4, 8):
                assert_image(field.make_scalar_view(sim.context, reduce=f), reduce_ref.reduce(plane, f),
                             f"{what} after the {name} kernel ({sim.context.info()[0]}), {rule}, f = {f}")
        sim.context.close()
    assert {"marching", "streaming", "auto"} <= set(ran), ran
    if rule in ("clipped", "zero_halo"):
        assert "window" in ran and "tile" in ran, ran


@pytest.mark.parametrize("slabs", [1, 2])
def test_overlapped_form_is_a_snapshot(built, slabs):
    """The reduced image enqueued after N steps holds the state after exactly N steps although more steps (which overwrite
    that plane) are enqueued right behind it; two images in flight; full and reduced images interleaved."""
    rows, cols = 192, 520
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * slabs))
    species = sim.make_species([rows, cols])
    plan = [(8, 4), (5, 1), (12, 8), (3, 3), (7, 1), (6, 16)]            # (steps, factor)
    images, done = [], []
    for i, (n, f) in enumerate(plan):
        sim.prepare_steps(species, n)
        image = pinned_empty(reduce_ref.shape(rows, cols, f))
        image[...] = -1.0
        species.write_result_view_after(image, reduce=f)
        images.append(image)
        done.append(n + (done[-1] if done else 0))
        if i:
            sim.context.download_wait(in_flight=1)                       # the image before this one is complete
            u0, v0 = oracle.init_species(rows, cols)
            want = reduce_ref.reduce(oracle.run(u0, v0, done[i - 1])[1], plan[i - 1][1])
            assert_image(np.array(images[i - 1]), want, f"image {i - 1} when handed over")
    sim.prepare_steps(species, 40)                                       # keeps the GPU busy behind the copies
    sim.context.download_wait()
    u0, v0 = oracle.init_species(rows, cols)
    for image, n, (_, f) in zip(images, done, plan):
        assert_image(np.array(image), reduce_ref.reduce(oracle.run(u0, v0, n)[1], f), f"image after {n} steps, f = {f}")
    sim.context.sync()
    assert species.make_result_view().tobytes() == oracle.run(u0, v0, done[-1] + 40)[1].tobytes()
    sim.context.close()


def _window_run(monkeypatch, give_up_from, calls=6, n=64, factors=(8, 3)):
    """The driver loop on the pinned window kernel at 1080 x 1920: per call the full image and two reduced ones, all
    enqueued behind the launch."""
    rows, cols = 1080, 1920
    u0, v0 = stress_fields((rows, cols), 11)
    monkeypatch.delenv("GS_HIP_WINDOW_PATIENCE", raising=False)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0], kernel=capi.GS_KERNEL_WINDOW))
    sp = species_from_arrays(sim, u0, v0)
    fulls = [pinned_empty((rows, cols)) for _ in range(calls)]
    reduced = [[pinned_empty(reduce_ref.shape(rows, cols, f)) for f in factors] for _ in range(calls)]
    for i in range(calls):
        if give_up_from is not None and i == give_up_from:
            monkeypatch.setenv("GS_HIP_WINDOW_PATIENCE", "1")
        sim.prepare_steps(sp, n)
        sp.write_result_view_after(reduced[i][0], reduce=factors[0])
        sp.write_result_view_after(fulls[i])
        sp.write_result_view_after(reduced[i][1], reduce=factors[1])
        sim.context.download_wait(in_flight=1)
    sim.context.download_wait()
    monkeypatch.delenv("GS_HIP_WINDOW_PATIENCE", raising=False)
    st, label = sim.context.stats(), sim.context.info()[0]
    sim.context.sync()
    final = sp.make_result_view()
    final_reduced = sp.make_result_view(reduce=factors[0])               # the blocking call after window launches
    sim.context.close()
    return [np.array(x) for x in fulls], [[np.array(x) for x in r] for r in reduced], final, final_reduced, st, label


def test_behind_window_launches_and_after_a_launch_that_gave_up(built, monkeypatch):
    """Reduced images enqueued behind persistent window launches are right; and when launches give up (a patience of one
    poll from the third call on: the library's own fallback, a replay by the marching kernel) each reduced image is formed
    again from the replayed plane."""
    factors = (8, 3)
    fulls, reduced, final, final_reduced, st, label = _window_run(monkeypatch, None, factors=factors)
    assert st["window_fallbacks"] == 0 and label.startswith("window"), (st, label)
    for i, full in enumerate(fulls):
        for f, image in zip(factors, reduced[i]):
            assert_image(image, reduce_ref.reduce(full, f), f"image {i} behind a window launch, f = {f}")
    assert final.tobytes() == fulls[-1].tobytes()
    assert_image(final_reduced, reduce_ref.reduce(final, factors[0]), "blocking call after window launches")
    # the kernels are bit-exact, so the planes of the run above are what the run with give-ups must show
    fulls2, reduced2, final2, final_reduced2, st2, label2 = _window_run(monkeypatch, 2, factors=factors)
    for i, full in enumerate(fulls):
        assert fulls2[i].tobytes() == full.tobytes(), f"full image {i} ({st2})"
        for f, image in zip(factors, reduced2[i]):
            assert_image(image, reduce_ref.reduce(full, f), f"image {i} with launches giving up from call 2, f = {f} ({st2})")
    assert final2.tobytes() == final.tobytes()
    assert_image(final_reduced2, final_reduced, "blocking call after the fallback")
    if st2["window_fallbacks"] == 0:
        pytest.skip("every single poll matched at once on this box: no launch gave up")
    assert label2.startswith("tb-k"), label2


@pytest.mark.parametrize("slabs", [1, 2])
def test_colormap_of_the_reduced_image(built, slabs):
    shape = (301, 517) if slabs == 1 else (480, 517)                     # (slabs of 240 rows: every factor below goes)
    rng = np.random.default_rng(4)
    palette = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * slabs))
    species = sim.make_species(shape)
    sim.perform_steps(species, 200)
    v = species.in_out()[1]
    plane = v.make_scalar_view(sim.context)
    for f in (2, 4, 5, 8):
        want = colormap_ref.colormap(reduce_ref.reduce(plane, f), palette)
        got = v.colormap(sim.context, palette, reduce=f)
        assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want), f
    special = reduce_ref.special_plane(shape, 8)                         # NaN pixels land on entry 0
    sp2 = species_from_arrays(sim, special, special)
    for f in (3, 4, 16):
        with np.errstate(all="ignore"):
            want = colormap_ref.colormap(reduce_ref.reduce(special, f), palette, scale=0.5)
        assert np.array_equal(sp2.in_out()[1].colormap(sim.context, palette, scale=0.5, reduce=f), want), f
    assert np.array_equal(v.colormap(sim.context, palette, reduce=1), v.colormap(sim.context, palette))
    sim.context.close()


def test_driver_writes_reduced_images(built, tmp_path):
    base = ["-n", "5", "-e", "40", "-r", "120", "-c", "250", "--output-buffer", "2"]
    plain, one, four = tmp_path / "plain.h5", tmp_path / "one.h5", tmp_path / "four.h5"
    driver.run(driver.parse(base + ["-o", str(plain)]))
    info1 = driver.run(driver.parse(base + ["-o", str(one), "--hip-image-reduce", "1"]))
    info4 = driver.run(driver.parse(base + ["-o", str(four), "--hip-image-reduce", "4"]))
    assert plain.read_bytes() == one.read_bytes()                        # F = 1: the file of a run without the option
    from grayscott_amd import hdf5_min

    full, small = hdf5_min.read(str(one)), hdf5_min.read(str(four))
    assert full.shape == (5, 120, 250) and small.shape == (5, 30, 63) and small.dtype == np.float32
    for i in range(5):
        assert_image(small[i], reduce_ref.reduce(full[i], 4), f"image {i} of the file")
    u, v = oracle.init_species(120, 250)
    assert full[4].tobytes() == oracle.run(u, v, 200)[1].tobytes()
    assert info1["image_bytes"] == 5 * 120 * 250 * 4 and info4["image_bytes"] == 5 * 30 * 63 * 4
    assert info4["image_reduce"] == 4 and tuple(info4["image_shape"]) == (30, 63)
    # .npy targets too
    npy = tmp_path / "four.npy"
    driver.run(driver.parse(base + ["-o", str(npy), "--hip-image-reduce", "4"]))
    assert np.load(npy).tobytes() == small.tobytes()
