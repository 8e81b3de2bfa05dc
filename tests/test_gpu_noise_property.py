"""Randomised parity of the noise kernels (gs_ctx_set_noise): hypothesis draws the shape (edge-biased strips and row chunks
of the marching kernel, grids of fewer rows than K under the periodic rule), the boundary rule (all four), the flavour,
the kernel and the schedule (fused steps, columns per lane, unit height, row bands, in-process slabs, graph replay,
general kernels, pitch padding), the parameters (power-of-two weights, the side weights at 0.5 half of the time so that
the .op variant runs), the sigmas (zeros, ordinary ones and -- strict math -- ones whose products are sub-normal), the
seed, the start step (values at and beyond 2^32 included) and the step counts and how they are delivered.  Every drawn
case is compared with the restatement (tests/noise_ref.py) bit for bit, after the refusal it must meet has been checked
by its code: gs_ctx_create's for what the boundary rule refuses, gs_ctx_set_noise's GS_ERR_UNSUPPORTED for a pinned
kernel without a noise form and for use_graph = 1; the case then runs its nearest legal form.  No case is left out."""
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, example, given, settings, strategies as st

from grayscott_amd import GsError, HipArgs, Parameters, Simulation, capi

from . import noise_ref as N
from .helpers import assert_bits_equal, oracle_params, species_from_arrays
from .test_gpu_noise import RULE_SUFFIX
from .test_gpu_property import POW2, RULE_WORD, RULES, refusal, tb_cols_per_wave

pytestmark = pytest.mark.gpu

NO_NOISE_FORM = (capi.GS_KERNEL_TILE, capi.GS_KERNEL_WINDOW, capi.GS_KERNEL_LDS)
DELIVERIES = ["run", "calls", "step"]
STARTS = [0, 1, 2 ** 32 - 2, 2 ** 32, 2 ** 40 + 7, 2 ** 64 - 3]


def legal(c):
    """The options a drawn case runs with after its refusals: (kernel, fuse, rpb, slabs, split, graph, refused at create,
    refused by set_noise)."""
    kernel, fuse, rpb, split, graph = c["kernel"], c["fuse"], c["rpb"], c["split"], c["graph"]
    slabs = min(c["slabs"], c["rows"])
    at_create = refusal(c["boundary"], kernel, slabs, split)
    if at_create is not None:
        if kernel == capi.GS_KERNEL_WINDOW:
            fuse = rpb = 0
        if kernel in (capi.GS_KERNEL_WINDOW, capi.GS_KERNEL_LDS) or slabs > 1 or split > 1:
            kernel = capi.GS_KERNEL_AUTO
        slabs, split = 1, 0
    at_noise = kernel in NO_NOISE_FORM or bool(graph)
    if kernel in NO_NOISE_FORM:
        if kernel == capi.GS_KERNEL_WINDOW:
            fuse = rpb = 0
        kernel = capi.GS_KERNEL_AUTO
    assert refusal(c["boundary"], kernel, slabs, split) is None
    return kernel, fuse, rpb, slabs, split, 0, at_create, at_noise


def pinned_case(**kw):
    base = dict(rows=17, cols=61, calls=[7], delivery="run", seed=1, kernel=capi.GS_KERNEL_TB, fuse=4, rpb=8, split=0, slabs=1,
                p=Parameters(), cpl=0, general=0, graph=0, pitch_pad=0, boundary=capi.GS_BOUNDARY_CLIPPED, math=capi.GS_MATH_STRICT,
                sigma_u=0.02, sigma_v=0.01, noise_seed=5, start=0)
    base.update(kw)
    return base


@st.composite
def noise_cases(draw):
    rows = draw(st.integers(1, 140))
    cols = draw(st.one_of(st.integers(1, 40), st.integers(240, 270), st.integers(480, 530), st.integers(990, 1040)))
    kernel = draw(st.sampled_from([capi.GS_KERNEL_AUTO, capi.GS_KERNEL_AUTO, capi.GS_KERNEL_TB, capi.GS_KERNEL_TB,
                                   capi.GS_KERNEL_STREAM, capi.GS_KERNEL_SIMPLE, capi.GS_KERNEL_TILE, capi.GS_KERNEL_WINDOW,
                                   capi.GS_KERNEL_LDS]))
    fuse = draw(st.integers(0, 4))
    rpb = draw(st.sampled_from([0, 1, 2, 3, 5, 8, 16, 33]))
    cpl = draw(st.sampled_from([0, 1, 2, 4]))
    boundary = draw(st.sampled_from(RULES))
    math = draw(st.sampled_from([capi.GS_MATH_STRICT, capi.GS_MATH_FUSED]))
    if kernel in (capi.GS_KERNEL_AUTO, capi.GS_KERNEL_TB) and draw(st.integers(0, 2)) == 0:
        # edge-biased shapes: the last strip 0 .. K + 1 or W - K - 1 .. W - 1 columns wide, the last row chunk likewise
        k = fuse if 1 <= fuse <= 4 else draw(st.integers(1, 4))
        c = cpl or draw(st.sampled_from([1, 2, 4]))
        w = tb_cols_per_wave(k, c)
        cols = draw(st.integers(1, 3 if w < 200 else 2)) * w + draw(st.sampled_from(sorted(set(range(k + 2)) | set(range(w - k - 1, w)))))
        if rpb < k + 2:
            rpb = draw(st.sampled_from([8, 16, 33]))
        rows = max(1, draw(st.integers(0, max(1, 140 // rpb))) * rpb
                   + draw(st.sampled_from(sorted(set(range(k + 2)) | set(range(rpb - k - 1, rpb))))))
    elif boundary == capi.GS_BOUNDARY_PERIODIC and draw(st.integers(0, 3)) == 0:
        rows = draw(st.integers(1, 3))            # fewer rows than K: the row wrap of a level reaches past the grid
    delivery = draw(st.sampled_from(DELIVERIES))
    calls = draw(st.lists(st.integers(1, 9), min_size=2, max_size=4)) if delivery == "calls" else [draw(st.integers(1, 13))]
    w = [[draw(st.sampled_from(POW2)) for _ in range(3)] for _ in range(3)]
    if draw(st.booleans()):                       # the default side weights: the .op variant
        w[0][1] = w[1][0] = w[1][2] = w[2][1] = 0.5
    p = Parameters(weights=tuple(tuple(r) for r in w), diffusion_rate_u=draw(st.sampled_from([0.1, 0.2, 0.05])),
                   diffusion_rate_v=draw(st.sampled_from([0.05, 0.1])), time_step=draw(st.sampled_from([1.0, 0.5, 0.75])))
    sigmas = [0.0, 0.001, 0.02, 0.5] + ([1e-38, 2.5e-39] if math == capi.GS_MATH_STRICT else [])
    return dict(rows=rows, cols=cols, calls=calls, delivery=delivery, seed=draw(st.integers(0, 2 ** 16)), kernel=kernel, fuse=fuse,
                rpb=rpb, split=draw(st.integers(0, 4)), slabs=draw(st.integers(1, 4)), p=p, cpl=cpl, general=draw(st.integers(0, 1)),
                graph=draw(st.sampled_from([0, 0, 0, 1])), pitch_pad=draw(st.sampled_from([0, 0, 3, 64])), boundary=boundary,
                math=math, sigma_u=draw(st.sampled_from(sigmas)), sigma_v=draw(st.sampled_from(sigmas)),
                noise_seed=draw(st.one_of(st.integers(0, 2 ** 64 - 1), st.sampled_from([0, 1, 2 ** 32, 2 ** 64 - 1]))),
                start=draw(st.one_of(st.sampled_from(STARTS), st.integers(0, 2 ** 64 - 40))))


OP_PARAMS = Parameters(weights=((0.25, 0.5, 0.125), (0.5, 1.0, 0.5), (0.0, 0.5, 0.25)), diffusion_rate_u=0.2, diffusion_rate_v=0.1)

# The cases that must always run: .op under the clipped rule at K = 4 and every CPL on >= 3 strips and >= 3 row chunks; the
# periodic rule on fewer rows than K with cols % CPL != 0; the zero-flux rule on one row and on one column; 3-slab chains of
# 4-row slabs at K = 4 (ghost rows draw at the neighbour's global rows); row bands; a start step whose run crosses 2^32;
# the refusals of use_graph and of a pinned window kernel.
EDGE_EXAMPLES = ([pinned_case(cpl=c, cols=3 * tb_cols_per_wave(4, c) + 5, rows=3 * 16 + 3, rpb=16, p=OP_PARAMS, seed=c) for c in (1, 2, 4)]
                 + [pinned_case(boundary=capi.GS_BOUNDARY_PERIODIC, rows=r, cols=n, cpl=c, p=OP_PARAMS)
                    for r, n, c in ((2, 61, 4), (3, 37, 2), (1, 130, 4))]
                 + [pinned_case(boundary=capi.GS_BOUNDARY_NEUMANN, rows=r, cols=n, p=OP_PARAMS, math=m)
                    for r, n in ((1, 61), (37, 1)) for m in (capi.GS_MATH_STRICT, capi.GS_MATH_FUSED)]
                 + [pinned_case(boundary=b, rows=12, cols=300, slabs=3, kernel=k, start=2 ** 32 - 3)
                    for b in (capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_NEUMANN) for k in (capi.GS_KERNEL_TB, capi.GS_KERNEL_AUTO)]
                 + [pinned_case(boundary=capi.GS_BOUNDARY_ZERO_HALO, rows=60, cols=300, split=2, calls=[11], p=OP_PARAMS)]
                 + [pinned_case(graph=1), pinned_case(kernel=capi.GS_KERNEL_WINDOW, rows=90, cols=300),
                    pinned_case(sigma_u=1e-38, sigma_v=0.0, delivery="step", calls=[3])])


def _with_examples(test):
    for ex in reversed(EDGE_EXAMPLES):
        test = example(case=ex)(test)
    return test


def run_noisy_case(c, u0, v0, noise):
    """The case on the GPU, refusals checked first.  Returns (U, V, kernel name, the noise term afterwards, what ran)."""
    kernel, fuse, rpb, slabs, split, graph, at_create, at_noise = legal(c)
    boundary, p = c["boundary"], c["p"]
    opts = dict(cols_per_lane=c["cpl"], general_kernels=c["general"], pitch_pad=c["pitch_pad"], boundary=boundary, math=c["math"])
    drawn = dict(kernel=c["kernel"], fuse_steps=c["fuse"], rows_per_block=c["rpb"], split=c["split"], use_graph=c["graph"],
                 devices=[0] * min(c["slabs"], c["rows"]))
    if at_create is not None:
        with pytest.raises(GsError) as e:
            Simulation.new(p, HipArgs(**drawn, **opts))
        assert e.value.code == capi.GS_ERR_UNSUPPORTED, e.value
        assert RULE_WORD[boundary] in str(e.value) and at_create in str(e.value), str(e.value)
    elif at_noise:
        sim = Simulation.new(p, HipArgs(**drawn, **opts))
        try:
            with pytest.raises(GsError) as e:
                sim.set_noise(**noise)
            assert e.value.code == capi.GS_ERR_UNSUPPORTED, e.value
            assert sim.noise() is None
        finally:
            sim.context.close()
    if kernel in (capi.GS_KERNEL_STREAM, capi.GS_KERNEL_SIMPLE):
        fuse = 0
    sim = Simulation.new(p, HipArgs(kernel=kernel, fuse_steps=fuse, rows_per_block=rpb, split=split, use_graph=graph,
                                    devices=[0] * slabs, **opts))
    try:
        species = species_from_arrays(sim, u0, v0)
        sim.set_noise(**noise)
        for n in c["calls"]:
            if c["delivery"] == "step":
                for _ in range(n):
                    sim.perform_step(species)
            else:
                sim.perform_steps(species, n)
        iu, iv, _, _ = species.in_out()
        name = sim.context.info()[0]
        ran = (f"kernel={name} ({kernel}) fuse={fuse} rpb={rpb} split={split} slabs={slabs} {c['delivery']} calls={c['calls']} "
               + " ".join(f"{k}={v}" for k, v in opts.items()))
        return iu.make_scalar_view(sim.context), iv.make_scalar_view(sim.context), name, sim.noise(), ran
    finally:
        sim.context.close()


@settings(max_examples=int(os.environ.get("GS_PROPERTY_EXAMPLES_NOISE", "100")), deadline=None, suppress_health_check=list(HealthCheck))
@given(noise_cases())
@_with_examples
def test_any_noisy_schedule_matches_the_reference(built, case):
    c = dict(case)
    rows, cols, boundary, math, p = c["rows"], c["cols"], c["boundary"], c["math"], c["p"]
    rng = np.random.default_rng(c["seed"])
    u0 = rng.random((rows, cols), dtype=np.float32)
    v0 = (rng.random((rows, cols), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    noise = dict(sigma_u=c["sigma_u"], sigma_v=c["sigma_v"], seed=c["noise_seed"], step=c["start"])
    steps = sum(c["calls"])
    ref_u, ref_v = N.run(u0, v0, steps, noise, params=oracle_params(p), rule=boundary, ftz=math == capi.GS_MATH_STRICT)
    got_u, got_v, name, after, ran = run_noisy_case(c, u0, v0, noise)
    what = f"{rows}x{cols} {ran} {noise} {p}"
    assert name.split("@")[0].endswith(RULE_SUFFIX[boundary]), f"{name}: {what}"
    assert after["step"] == (c["start"] + steps) % 2 ** 64 and after["seed"] == c["noise_seed"], f"{after}: {what}"
    assert_bits_equal(got_u, ref_u, "U " + what)
    assert_bits_equal(got_v, ref_v, "V " + what)
