"""Randomised parity of the parameter map's kernels (gs_ctx_set_param_map): hypothesis draws the shape (edge-biased strips
and row chunks of the marching kernel, grids of fewer rows than K under the periodic rule), the steps and how they are
delivered (one gs_run, several of drawn lengths, or gs_step), the kernel, the schedule (fused steps, columns per lane,
unit height, row bands, in-process slabs, graph replay, general kernels, pitch padding, difference sharing), the boundary
rule (all four), the flavour, the parameters (power-of-two weights, the side weights at 0.5 half of the time so that the
.op variant runs; "patrakarttunen" in strict math), the map (random, uniform, constant in row or column bands, or with
+-0, zero kill, sub-normal feed and sub-normal feed + kill planted) and, optionally, sub-normal values in the state.
Every combination must equal the mapped reference (tests/param_map_ref.py) bit for bit -- in fused math too, unless the
state or the map holds sub-normals, where the contract is 1e-37 absolute (include/gs_hip.h, gs_math).  The kernel that
ran carries the rule's map suffix, is the marching kernel whenever gs_run ran with the kernel auto or TB (auto: unless
its last pass was a single step, which auto runs with the streaming kernel as it does a gs_step), and is its .op
variant exactly when the strict flavour, the default side weights and dt == 1 allow it and general kernels are not
pinned.  Kernels without a map form (tile, window, LDS) must be refused by gs_ctx_set_param_map; combinations a rule
refuses must be refused by gs_ctx_create; the example then runs its nearest legal case."""
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, example, given, settings, strategies as st

from grayscott_amd import GsError, HipArgs, Parameters, Simulation, capi
from grayscott_amd.simulation import STENCILS

from . import param_map_ref as R
from .helpers import assert_bits_equal, species_from_arrays
from .test_gpu_param_map import RULE_SUFFIX
from .test_gpu_property import POW2, RULE_WORD, RULES, refusal, tb_cols_per_wave

pytestmark = pytest.mark.gpu

NO_MAP_FORM = (capi.GS_KERNEL_TILE, capi.GS_KERNEL_WINDOW, capi.GS_KERNEL_LDS)
MAP_KINDS = ["random", "uniform", "row-bands", "col-bands", "planted"]
DELIVERIES = ["run", "calls", "step"]


def make_map(kind, shape, rng):
    """(feed, kill) of `kind` for a grid of `shape`: planes, or two scalars for the uniform map."""
    rows, cols = shape
    if kind == "uniform":
        return (np.float32(rng.choice([0.0, 0.014, 0.03, 0.055])), np.float32(rng.choice([0.0, 0.045, 0.054, 0.062])))
    if kind == "planted":
        return R.planted_map(shape, rng)
    if kind in ("row-bands", "col-bands"):
        n = rows if kind == "row-bands" else cols
        edges = np.sort(rng.integers(0, n + 1, rng.integers(0, 4)))
        band = np.searchsorted(edges, np.arange(n), side="right")
        f = rng.uniform(0.01, 0.06, band.max() + 1).astype(np.float32)[band]
        k = rng.uniform(0.04, 0.07, band.max() + 1).astype(np.float32)[band]
        if kind == "row-bands":
            return np.repeat(f[:, None], cols, axis=1), np.repeat(k[:, None], cols, axis=1)
        return np.repeat(f[None, :], rows, axis=0), np.repeat(k[None, :], rows, axis=0)
    return (rng.uniform(0.01, 0.06, shape).astype(np.float32), rng.uniform(0.04, 0.07, shape).astype(np.float32))


def uses_op(p, math, general):
    """Does the marching kernel's map form run its .op variant (tb_map_fast: strict, side weights 0.5, dt == 1)?"""
    w = p.weights
    sides = all(np.float32(x) == np.float32(0.5) for x in (w[0][1], w[1][0], w[1][2], w[2][1]))
    return math == capi.GS_MATH_STRICT and not general and sides and np.float32(p.time_step) == np.float32(1.0)


def legal(c):
    """The options a drawn case runs with after the refusals: (kernel, fuse, rpb, slabs, split, refused at create, refused
    by set_param_map).  Also the strategy's own check (tests/test_param_map_cpu.py draws cases on the CPU)."""
    kernel, fuse, rpb, split = c["kernel"], c["fuse"], c["rpb"], c["split"]
    slabs = min(c["slabs"], c["rows"])
    at_create = refusal(c["boundary"], kernel, slabs, split)
    if at_create is not None:
        if kernel == capi.GS_KERNEL_WINDOW:
            fuse = rpb = 0
        if kernel in (capi.GS_KERNEL_WINDOW, capi.GS_KERNEL_LDS) or slabs > 1 or split > 1:
            kernel = capi.GS_KERNEL_AUTO
        slabs, split = 1, 0
    at_map = kernel in NO_MAP_FORM
    if at_map:
        if kernel == capi.GS_KERNEL_WINDOW:
            fuse = rpb = 0
        kernel = capi.GS_KERNEL_AUTO
    assert refusal(c["boundary"], kernel, slabs, split) is None and kernel not in NO_MAP_FORM
    assert 0 <= fuse <= 4 and c["cpl"] in (0, 1, 2, 4) and 1 <= slabs <= 4 and c["rows"] >= 1 and c["cols"] >= 1
    assert c["math"] == capi.GS_MATH_STRICT or all(np.float32(x) == 0 or np.frexp(np.float32(abs(x)))[0] == 0.5
                                                   for r in c["p"].weights for x in r), "fused math takes power-of-two weights"
    assert c["map"] in MAP_KINDS and c["delivery"] in DELIVERIES and sum(c["calls"]) >= 1
    return kernel, fuse, rpb, slabs, split, at_create, at_map


def pinned_case(**kw):
    """A case of `map_cases` with every field at its plainest value but those given (the @example cases)."""
    base = dict(rows=17, cols=61, calls=[11], delivery="run", seed=1, kernel=capi.GS_KERNEL_TB, fuse=4, rpb=8, split=0,
                slabs=1, p=Parameters(), tiny=False, cpl=0, general=0, graph=0, pitch_pad=0, boundary=capi.GS_BOUNDARY_CLIPPED,
                math=capi.GS_MATH_STRICT, share_taps=0, map="random")
    base.update(kw)
    return base


@st.composite
def map_cases(draw):
    rows = draw(st.integers(1, 140))
    cols = draw(st.one_of(st.integers(1, 40), st.integers(240, 270), st.integers(480, 530), st.integers(990, 1040)))
    seed = draw(st.integers(0, 2 ** 16))
    kernel = draw(st.sampled_from([capi.GS_KERNEL_AUTO, capi.GS_KERNEL_AUTO, capi.GS_KERNEL_TB, capi.GS_KERNEL_TB,
                                   capi.GS_KERNEL_STREAM, capi.GS_KERNEL_SIMPLE, capi.GS_KERNEL_TILE, capi.GS_KERNEL_WINDOW,
                                   capi.GS_KERNEL_LDS]))
    fuse = draw(st.integers(0, 4))
    rpb = draw(st.sampled_from([0, 1, 2, 3, 5, 8, 16, 33]))
    split = draw(st.integers(0, 4))
    slabs = draw(st.integers(1, 4))
    cpl = draw(st.sampled_from([0, 1, 2, 4]))
    general = draw(st.integers(0, 1))
    graph = draw(st.integers(0, 1))
    pitch_pad = draw(st.sampled_from([0, 0, 3, 64]))
    boundary = draw(st.sampled_from(RULES))
    math = draw(st.sampled_from([capi.GS_MATH_STRICT, capi.GS_MATH_FUSED]))
    share_taps = draw(st.integers(0, 3))
    if kernel in (capi.GS_KERNEL_AUTO, capi.GS_KERNEL_TB) and draw(st.integers(0, 2)) == 0:
        # edge-biased shapes: the last strip of the marching kernel 0 .. K + 1 or W - K - 1 .. W - 1 columns wide after
        # m full ones, the last row chunk 0 .. K + 1 or rpb - K - 1 .. rpb - 1 rows high (K and CPL as pinned, else drawn)
        k = fuse if 1 <= fuse <= 4 else draw(st.integers(1, 4))
        c = cpl or draw(st.sampled_from([1, 2, 4]))
        w = tb_cols_per_wave(k, c)
        cols = draw(st.integers(1, 3 if w < 200 else 2)) * w + draw(st.sampled_from(sorted(set(range(k + 2)) | set(range(w - k - 1, w)))))
        if rpb < k + 2:
            rpb = draw(st.sampled_from([8, 16, 33]))
        rows = draw(st.integers(0, max(1, 140 // rpb))) * rpb + draw(st.sampled_from(sorted(set(range(k + 2)) | set(range(rpb - k - 1, rpb)))))
        rows = max(rows, 1)
    elif boundary == capi.GS_BOUNDARY_PERIODIC and draw(st.integers(0, 3)) == 0:
        rows = draw(st.integers(1, 3))            # fewer rows than K: the row wrap of a level reaches past the grid
    delivery = draw(st.sampled_from(DELIVERIES))
    if delivery == "calls":
        calls = draw(st.lists(st.integers(1, 9), min_size=2, max_size=4))
    else:
        calls = [draw(st.integers(1, 13))]
    w = [[draw(st.sampled_from(POW2)) for _ in range(3)] for _ in range(3)]
    if draw(st.booleans()):                       # the default side weights: the .op variant
        w[0][1] = w[1][0] = w[1][2] = w[2][1] = 0.5
    weights = tuple(tuple(r) for r in w)
    if math == capi.GS_MATH_STRICT and draw(st.integers(0, 5)) == 0:
        weights = STENCILS["patrakarttunen"]      # not powers of two: strict only
    p = Parameters(weights=weights,
                   diffusion_rate_u=draw(st.sampled_from([0.1, 0.2, 0.05])),
                   diffusion_rate_v=draw(st.sampled_from([0.05, 0.1])),
                   time_step=draw(st.sampled_from([1.0, 0.5, 0.75])))
    kind = draw(st.sampled_from(MAP_KINDS))
    tiny = draw(st.booleans())                    # sprinkle sub-normal values into the state
    return dict(rows=rows, cols=cols, calls=calls, delivery=delivery, seed=seed, kernel=kernel, fuse=fuse, rpb=rpb, split=split,
                slabs=slabs, p=p, tiny=tiny, cpl=cpl, general=general, graph=graph, pitch_pad=pitch_pad, boundary=boundary,
                math=math, share_taps=share_taps, map=kind)


# non-default corners, a centre weight, other diffusion rates: side weights 0.5 and dt = 1 keep the .op variant
OP_PARAMS = Parameters(weights=((0.25, 0.5, 0.125), (0.5, 1.0, 0.5), (0.0, 0.5, 0.25)), diffusion_rate_u=0.2, diffusion_rate_v=0.1)

# The cases that must always run: .op under the clipped rule at K = 4 and every CPL on >= 3 strips and >= 3 row chunks
# (edge kinds 2, 3 and 4 of the strict build); the periodic rule on fewer rows than K with cols % CPL != 0; the zero-flux
# rule on one row and on one column; 3-slab chains of 4-row slabs at K = 4; graph replay of >= 16 passes with row bands;
# fused math at K = 3 with dt = 0.5.
EDGE_EXAMPLES = ([pinned_case(cpl=c, cols=3 * tb_cols_per_wave(4, c) + 5, rows=3 * 16 + 3, rpb=16, p=OP_PARAMS, seed=c)
                  for c in (1, 2, 4)]
                 + [pinned_case(boundary=capi.GS_BOUNDARY_PERIODIC, rows=r, cols=n, cpl=c, p=OP_PARAMS, map=m)
                    for r, n, c, m in ((2, 61, 4, "random"), (3, 37, 2, "planted"), (1, 130, 4, "col-bands"))]
                 + [pinned_case(boundary=capi.GS_BOUNDARY_NEUMANN, rows=r, cols=n, p=OP_PARAMS, map="planted", math=m)
                    for r, n in ((1, 61), (37, 1)) for m in (capi.GS_MATH_STRICT, capi.GS_MATH_FUSED)]
                 + [pinned_case(boundary=b, rows=12, cols=300, slabs=3, kernel=k, p=OP_PARAMS)
                    for b in (capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_NEUMANN) for k in (capi.GS_KERNEL_TB, capi.GS_KERNEL_AUTO)]
                 + [pinned_case(boundary=b, rows=60, cols=300, graph=1, split=2, calls=[11], p=p)
                    for b, p in ((capi.GS_BOUNDARY_ZERO_HALO, OP_PARAMS), (capi.GS_BOUNDARY_NEUMANN, Parameters(time_step=0.5)))]
                 + [pinned_case(math=capi.GS_MATH_FUSED, fuse=3, cpl=2, rows=50, cols=2 * tb_cols_per_wave(3, 2) + 1, rpb=16,
                                p=Parameters(time_step=0.5, diffusion_rate_u=0.2), boundary=b)
                    for b in (capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_PERIODIC)])


def _with_examples(test):
    for ex in reversed(EDGE_EXAMPLES):
        test = example(case=ex)(test)
    return test


def run_mapped_case(c, u0, v0, feed, kill):
    """The case on the GPU, refusals checked first.  Returns (U, V, kernel name, kernel, fuse_steps, slabs, what ran)."""
    kernel, fuse, rpb, slabs, split, at_create, at_map = legal(c)
    boundary, p = c["boundary"], c["p"]
    opts = dict(cols_per_lane=c["cpl"], general_kernels=c["general"], use_graph=c["graph"], pitch_pad=c["pitch_pad"],
                boundary=boundary, math=c["math"], share_taps=c["share_taps"])
    drawn = dict(kernel=c["kernel"], fuse_steps=c["fuse"], rows_per_block=c["rpb"], split=c["split"],
                 devices=[0] * min(c["slabs"], c["rows"]))
    if at_create is not None:
        with pytest.raises(GsError) as e:
            Simulation.new(p, HipArgs(**drawn, **opts))
        assert e.value.code == capi.GS_ERR_UNSUPPORTED, e.value
        assert RULE_WORD[boundary] in str(e.value) and at_create in str(e.value), str(e.value)
    elif at_map:
        sim = Simulation.new(p, HipArgs(**drawn, **opts))
        try:
            with pytest.raises(GsError) as e:
                sim.set_param_map(feed, kill, shape=u0.shape)
            assert e.value.code == capi.GS_ERR_UNSUPPORTED, e.value
        finally:
            sim.context.close()
    if kernel in (capi.GS_KERNEL_STREAM, capi.GS_KERNEL_SIMPLE):
        fuse = 0
    sim = Simulation.new(p, HipArgs(kernel=kernel, fuse_steps=fuse, rows_per_block=rpb, split=split, devices=[0] * slabs, **opts))
    try:
        species = species_from_arrays(sim, u0, v0)
        sim.set_param_map(feed, kill, shape=u0.shape)
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
        return iu.make_scalar_view(sim.context), iv.make_scalar_view(sim.context), name, kernel, fuse, slabs, ran
    finally:
        sim.context.close()


@settings(max_examples=int(os.environ.get("GS_PROPERTY_EXAMPLES_MAP", "120")), deadline=None, suppress_health_check=list(HealthCheck))
@given(map_cases())
@_with_examples
def test_any_mapped_schedule_matches_the_reference(built, case):
    c = dict(case)
    if c["graph"] and c["delivery"] == "run":
        c["calls"] = [c["calls"][0] * 9]          # long enough for at least one batch of 16 passes
    rows, cols, boundary, math, p = c["rows"], c["cols"], c["boundary"], c["math"], c["p"]
    rng = np.random.default_rng(c["seed"])
    u0 = rng.random((rows, cols), dtype=np.float32)
    v0 = (rng.random((rows, cols), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    if c["tiny"]:
        mask = rng.random((rows, cols)) < 0.3
        v0[mask] = (v0[mask] * np.float32(1e-37)).astype(np.float32)
        u0[rng.random((rows, cols)) < 0.05] = np.float32(3e-38)
    feed, kill = make_map(c["map"], (rows, cols), rng)
    strict = math == capi.GS_MATH_STRICT
    ref_u, ref_v = R.run(u0, v0, sum(c["calls"]), feed, kill, params=R.params_of(p), boundary=boundary, ftz=strict)
    got_u, got_v, name, kernel, fuse, slabs, ran = run_mapped_case(c, u0, v0, feed, kill)
    what = f"{rows}x{cols} {ran} map={c['map']} tiny={c['tiny']} {p}"
    assert name.split("@")[0].endswith(RULE_SUFFIX[boundary]), f"{name}: {what}"
    if c["delivery"] != "step" and kernel in (capi.GS_KERNEL_AUTO, capi.GS_KERNEL_TB):
        # (kernel = auto runs a pass of one step with the streaming kernel, as it does a gs_step: a call of one step, or
        # one step per pass -- fuse_steps = 1, or slabs of one row)
        single_steps = c["calls"][-1] == 1 or fuse == 1 or rows // slabs < 2
        assert name.startswith("tb-k") or (kernel == capi.GS_KERNEL_AUTO and single_steps and name.startswith("stream")), \
            f"{name}: {what}"
    if name.startswith("tb-k"):
        assert (".op" in name) == uses_op(p, math, c["general"]), f"{name}: {what}"
    with np.errstate(all="ignore"):
        fpk = np.float32(feed) + np.float32(kill)
    if strict or not (c["tiny"] or R.has_subnormal(np.float32(feed), np.float32(kill), fpk)):
        assert_bits_equal(got_u, ref_u, "U " + what)
        assert_bits_equal(got_v, ref_v, "V " + what)
        return
    for plane, got, ref in (("U", got_u, ref_u), ("V", got_v, ref_v)):
        g, r = got.astype(np.float64), ref.astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = (g == r) | (np.abs(g - r) <= 1e-37) | (np.isnan(g) & np.isnan(r))
        assert ok.all(), f"fused {plane} {what}: {int((~ok).sum())} cells beyond 1e-37, first at {np.argwhere(~ok)[0]}"
