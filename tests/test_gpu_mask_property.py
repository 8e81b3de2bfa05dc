"""Randomised parity of the domain mask's kernels (gs_ctx_set_mask): hypothesis draws what the parameter map's property
test draws (tests/test_gpu_param_map_property.py: the shape with edge-biased strips and row chunks of the marching kernel
and grids of fewer rows than K under the periodic rule, the steps and their delivery, the kernel, the schedule, the
boundary rule, the flavour, the parameters, sub-normal values in the state), grids of 1 to 3 columns under the periodic
rule, and on top of it

* the wall layout (`make_walls`): random at four wall shares, all fluid, all wall, the grid's outer frame or everything
  but it, wall lines with gaps on the seams of the marching kernel's strips and row chunks and on the slabs' boundary
  rows, two checkerboards, one fluid cell among walls, one wall among fluid (half of the time at a corner or an edge's
  midpoint), the maze of tests/mask_ref.py;
* how the walls reach the device (`values`): through Simulation.set_mask, which uploads 0 and 1, or "raw": a field of
  +-0 for fluid and of 1, -3, +-inf, quiet and signalling NaNs, sub-normals of either sign and the smallest normal for
  walls, handed to gs_ctx_set_mask itself, zeroed and destroyed before the steps run -- the device's own `!= 0.0f`
  (include/gs_hip.h) decides what is a wall, as `mask_ref.walls_of` does for the reference;
* `poison`: the wall cells of the state hold NaNs with payloads, +inf and sub-normals.  The reference never reads a
  wall's value, so one tap that does read one shows in a fluid cell.

Every combination must equal the masked reference (tests/mask_ref.py): wall cells keep their input bits always; fluid
cells bit for bit in strict math and in fused math without sub-normals in the state, within the fused flavour's 1e-37
absolute (include/gs_hip.h, gs_math) with them.  An all-fluid layout must also equal the unmasked reference
(helpers.rule_run), an all-wall one its input.  The kernel that ran carries the rule's mask suffix and shares no
differences, is the marching kernel whenever gs_run ran with the kernel auto or TB (auto: unless its last pass was a
single step, which auto runs with the streaming kernel as it does a gs_step), and is its .op variant exactly when
`uses_op` says so.  Kernels without a mask form (tile, window, LDS) must be refused by gs_ctx_set_mask; combinations a
rule refuses must be refused by gs_ctx_create with a message that names the rule; the example then runs its nearest legal
case.  tests/test_mask_cpu.py checks without a GPU that the strategy draws legal cases of every kind, that the layouts
are what they claim, and that every pinned example would notice each single fault of a masked step."""
import collections
import os
import re
import time

import numpy as np
import pytest
from hypothesis import HealthCheck, example, given, settings, strategies as st

from grayscott_amd import GsError, HipArgs, HipConcentration, Parameters, Simulation, capi
from grayscott_amd.simulation import STENCILS

from . import mask_ref as R
from .helpers import assert_bits_equal, oracle_params, rule_run, species_from_arrays
from .param_map_ref import params_of
from .test_gpu_mask import RULE_SUFFIX
from .test_gpu_property import POW2, RULE_WORD, RULES, refusal, tb_cols_per_wave

pytestmark = pytest.mark.gpu

NO_MASK_FORM = (capi.GS_KERNEL_TILE, capi.GS_KERNEL_WINDOW, capi.GS_KERNEL_LDS)
LAYOUTS = ["random", "all-fluid", "all-wall", "frame", "seams", "checker", "one-fluid", "one-wall", "maze"]
SHARES = [0.02, 0.25, 0.5, 0.9]
PLACES = ["nw", "n", "ne", "w", "e", "sw", "s", "se"]      # corners and edge midpoints of one-fluid / one-wall
VALUES = ["api", "raw"]
DELIVERIES = ["run", "calls", "step"]

# What a raw mask holds in its wall cells: every class of float32 that is != 0.0f -- normals of either sign, infinities,
# quiet NaNs of either sign with payloads, a signalling NaN, sub-normals of either sign, the smallest normal
WALL_WORDS = np.array([0x3f800000, 0xc0400000, 0x7f800000, 0xff800000, 0x7fc01234, 0xffc00077, 0x7f800001, 0x00000001,
                       0x80000005, 0x00800000], np.uint32)
# ... and a poisoned state in its wall cells (the words of tests/test_gpu_mask.py::test_walls_keep_their_bits)
POISON_WORDS = np.array([0x7fc01234, 0xffc00077, 0x7f800000, 0x00000003, 0x80000005], np.uint32)

# What ran, for the report of a run (printed when the module is done; shown with pytest -s or -rP)
SEEN = collections.Counter()


def seam_lines(shape, c):
    """(columns, rows) of the `seams` layout for case `c`: the columns m W - 1, m W and m W + 1 at the case's strip width
    W = tb_cols_per_wave(K, CPL) (K and CPL as pinned, else 4), the rows m rpb - 1 and m rpb (rpb as pinned, else 16),
    and every slab's first row and the row before it (the library's k rows // slabs, and round(k rows / slabs))."""
    rows, cols = shape
    k = c["fuse"] if 1 <= c["fuse"] <= 4 else 4
    w = tb_cols_per_wave(k, c["cpl"] or 4)
    rpb = c["rpb"] or 16
    slabs = min(c["slabs"], rows)
    line_cols = sorted({x for m in range(1, cols // w + 2) for x in (m * w - 1, m * w, m * w + 1) if 0 <= x < cols})
    firsts = {m * rpb for m in range(1, rows // rpb + 2)}
    firsts |= {i * rows // slabs for i in range(1, slabs)} | {int(round(i * rows / slabs)) for i in range(1, slabs)}
    line_rows = sorted({x for r in firsts for x in (r - 1, r) if 0 <= x < rows})
    return line_cols, line_rows


def seams_are_mixed(walls, line_cols, line_rows):
    """Does every seam line of 8 cells or more hold a wall and a gap?"""
    lines = ([walls[:, x] for x in line_cols] if walls.shape[0] >= 8 else []) + ([walls[r, :] for r in line_rows] if walls.shape[1] >= 8 else [])
    return all(line.any() and not line.all() for line in lines)


def place_of(name, shape):
    rows, cols = shape
    r = {"n": 0, "s": rows - 1}.get(name[0], rows // 2)
    col = {"w": 0, "e": cols - 1}.get(name[-1], cols // 2)
    return r, col


def make_walls(kind, shape, rng, c):
    """The wall cells of layout `kind` on a grid of `shape` as a boolean plane.  Case `c` gives the variant: `share` of
    a random layout; `flip` for the frame's reverse (only the outer ring is fluid) and the checkerboard of 2 x 2 blocks;
    `at`, a name of PLACES or None for a cell drawn from `rng`; and the schedule the seams follow."""
    rows, cols = shape
    rr, cc = np.mgrid[0:rows, 0:cols]
    if kind == "random":
        return rng.random(shape) < c["share"]
    if kind == "all-fluid":
        return np.zeros(shape, bool)
    if kind == "all-wall":
        return np.ones(shape, bool)
    if kind == "frame":
        ring = (rr == 0) | (rr == rows - 1) | (cc == 0) | (cc == cols - 1)
        return ~ring if c["flip"] else ring
    if kind == "seams":
        line_cols, line_rows = seam_lines(shape, c)
        lines = np.zeros(shape, bool)
        lines[:, line_cols] = True
        lines[line_rows, :] = True
        for _ in range(64):
            walls = lines & (rng.random(shape) < 0.5)    # every line cell opened again half of the time ...
            if seams_are_mixed(walls, line_cols, line_rows):
                break                                    # ... and drawn again until every line has walls and gaps
        return walls
    if kind == "checker":
        return ((rr // 2 + cc // 2) % 2 == 1) if c["flip"] else ((rr + cc) % 2 == 1)
    if kind in ("one-fluid", "one-wall"):
        at = place_of(c["at"], shape) if c["at"] else (int(rng.integers(0, rows)), int(rng.integers(0, cols)))
        walls = np.zeros(shape, bool)
        walls[at] = True
        return walls if kind == "one-wall" else ~walls
    if kind == "maze":
        return R.maze(shape, rng) != 0
    raise ValueError(kind)


def mask_values(walls, values, rng):
    """The mask as the case hands it over: the boolean plane for Simulation.set_mask, or the raw float32 field -- fluid
    +0 or -0, a wall one of WALL_WORDS, per cell."""
    if values == "api":
        return walls
    m = np.where(rng.random(walls.shape) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    m[walls] = WALL_WORDS.view(np.float32)[rng.integers(0, WALL_WORDS.size, int(walls.sum()))]
    return m


def poisoned(u0, v0, walls, rng):
    odd = POISON_WORDS.view(np.float32)
    pick = rng.integers(0, odd.size, walls.shape)
    return np.where(walls, odd[pick], u0).astype(np.float32), np.where(walls, odd[::-1][pick], v0).astype(np.float32)


def fields_of(c):
    """(u0, v0, walls, mask) of case `c`, all drawn from its seed: the state (sub-normals sprinkled in with `tiny`, its
    wall cells poisoned with `poison`), the boolean wall plane and the mask as it is handed over."""
    shape = (c["rows"], c["cols"])
    rng = np.random.default_rng(c["seed"])
    u0 = rng.random(shape, dtype=np.float32)
    v0 = (rng.random(shape, dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    if c["tiny"]:
        small = rng.random(shape) < 0.3
        v0[small] = (v0[small] * np.float32(1e-37)).astype(np.float32)
        u0[rng.random(shape) < 0.05] = np.float32(3e-38)
    walls = make_walls(c["layout"], shape, rng, c)
    mask = mask_values(walls, c["values"], rng)
    if c["poison"]:
        u0, v0 = poisoned(u0, v0, walls, rng)
    return u0, v0, walls, mask


def steps_of(c):
    """The calls of case `c` as they run: with graph replay, one gs_run is lengthened to hold a batch of 16 passes."""
    if c["graph"] and c["delivery"] == "run":
        return [c["calls"][0] * 9]
    return list(c["calls"])


def uses_op(p, math, general, boundary, k, cpl):
    """Does the marching kernel's mask form of K = `k` fused steps and `cpl` columns per lane run its .op variant?
    GsStepArgs::fast (gs_tuner.cpp, fast_possible) has bits 0 and 1 when general kernels are not pinned, the four side
    weights are 0.5f and dt == 1.0f; the mask's launch (gs_step_kernels.hip, tb_fast_of) turns that into .op in the
    strict flavour only, and only where the form is built: gs_tb_mask_kernel_strict lacks the clipped and zero-halo
    rules' .op kernels of 4 columns per lane with 3 or 4 fused steps, where the general form runs."""
    w = p.weights
    sides = all(np.float32(x) == np.float32(0.5) for x in (w[0][1], w[1][0], w[1][2], w[2][1]))
    built = not (boundary in (capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO) and cpl == 4 and k >= 3)
    return math == capi.GS_MATH_STRICT and not general and sides and np.float32(p.time_step) == np.float32(1.0) and built


def tb_form(name):
    """(K, CPL) of a marching kernel's name: tb-k<K>[c1|c2] (no suffix: 4 columns per lane)."""
    m = re.match(r"tb-k([1-4])(c[12])?[./]", name)
    assert m, name
    return int(m.group(1)), int(m.group(2)[1]) if m.group(2) else 4


def legal(c):
    """The options a drawn case runs with after the refusals: (kernel, fuse, rpb, slabs, split, refused at create, refused
    by set_mask).  Also the strategy's own check (tests/test_mask_cpu.py draws cases on the CPU)."""
    kernel, fuse, rpb, split = c["kernel"], c["fuse"], c["rpb"], c["split"]
    slabs = min(c["slabs"], c["rows"])
    at_create = refusal(c["boundary"], kernel, slabs, split)
    if at_create is not None:
        if kernel == capi.GS_KERNEL_WINDOW:
            fuse = rpb = 0
        if kernel in (capi.GS_KERNEL_WINDOW, capi.GS_KERNEL_LDS) or slabs > 1 or split > 1:
            kernel = capi.GS_KERNEL_AUTO
        slabs, split = 1, 0
    at_mask = kernel in NO_MASK_FORM
    if at_mask:
        if kernel == capi.GS_KERNEL_WINDOW:
            fuse = rpb = 0
        kernel = capi.GS_KERNEL_AUTO
    assert refusal(c["boundary"], kernel, slabs, split) is None and kernel not in NO_MASK_FORM
    assert 0 <= fuse <= 4 and c["cpl"] in (0, 1, 2, 4) and 1 <= slabs <= 4 and c["rows"] >= 1 and c["cols"] >= 1
    assert c["math"] == capi.GS_MATH_STRICT or all(np.float32(x) == 0 or np.frexp(np.float32(abs(x)))[0] == 0.5
                                                   for r in c["p"].weights for x in r), "fused math takes power-of-two weights"
    assert c["layout"] in LAYOUTS and c["values"] in VALUES and c["share"] in SHARES and c["at"] in [None] + PLACES
    assert c["delivery"] in DELIVERIES and sum(c["calls"]) >= 1
    assert c["rows"] * c["cols"] * sum(steps_of(c)) <= 140 * 1040 * 117, "the reference's time is capped"
    return kernel, fuse, rpb, slabs, split, at_create, at_mask


def pinned_case(**kw):
    """A case of `mask_cases` with every field at its plainest value but those given (the @example cases)."""
    base = dict(rows=17, cols=61, calls=[11], delivery="run", seed=1, kernel=capi.GS_KERNEL_TB, fuse=4, rpb=8, split=0,
                slabs=1, p=Parameters(), tiny=False, cpl=0, general=0, graph=0, pitch_pad=0, boundary=capi.GS_BOUNDARY_CLIPPED,
                math=capi.GS_MATH_STRICT, share_taps=0, layout="random", share=0.25, flip=False, at=None, values="api",
                poison=False)
    base.update(kw)
    return base


@st.composite
def mask_cases(draw):
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
    elif boundary == capi.GS_BOUNDARY_PERIODIC:
        if draw(st.integers(0, 3)) == 0:
            rows = draw(st.integers(1, 3))            # fewer rows than K: the row wrap of a level reaches past the grid
        if draw(st.integers(0, 3)) == 0:
            cols = draw(st.integers(1, 3))            # the left and right neighbour are one cell, or the cell itself
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
    tiny = draw(st.booleans())                    # sprinkle sub-normal values into the state
    layout = draw(st.sampled_from(LAYOUTS))
    share = draw(st.sampled_from(SHARES))
    flip = draw(st.booleans())
    at = draw(st.sampled_from(PLACES)) if draw(st.booleans()) else None
    values = draw(st.sampled_from(VALUES))
    poison = draw(st.booleans())
    return dict(rows=rows, cols=cols, calls=calls, delivery=delivery, seed=seed, kernel=kernel, fuse=fuse, rpb=rpb, split=split,
                slabs=slabs, p=p, tiny=tiny, cpl=cpl, general=general, graph=graph, pitch_pad=pitch_pad, boundary=boundary,
                math=math, share_taps=share_taps, layout=layout, share=share, flip=flip, at=at, values=values, poison=poison)


# The map test's OP_PARAMS (non-default corners, a centre weight, other diffusion rates; side weights 0.5 and dt = 1 keep
# the .op variant) with its zero corner at 0.0625: every tap of the eight neighbours shows in the result
OP_PARAMS = Parameters(weights=((0.25, 0.5, 0.125), (0.5, 1.0, 0.5), (0.0625, 0.5, 0.25)), diffusion_rate_u=0.2, diffusion_rate_v=0.1)
HALF_DT = Parameters(time_step=0.5, diffusion_rate_u=0.2)

_C, _Z, _P, _N = capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_PERIODIC, capi.GS_BOUNDARY_NEUMANN
_STRICT, _FUSED = capi.GS_MATH_STRICT, capi.GS_MATH_FUSED
# one cell at a corner: the marching kernel by gs_run (pinned, and kernel auto) and the single-step kernels by gs_step
_CORNER_RUNS = {"nw": dict(kernel=capi.GS_KERNEL_TB), "ne": dict(kernel=capi.GS_KERNEL_STREAM, delivery="step", calls=[5]),
                "sw": dict(kernel=capi.GS_KERNEL_SIMPLE, delivery="step", calls=[5]), "se": dict(kernel=capi.GS_KERNEL_AUTO)}

# The cases that must always run, all with weights that leave no tap invisible:
# - .op under the clipped rule at K = 4 and every CPL (CPL 4: the general form, that .op form is not built; K = 2 there
#   for the .op form) on >= 3 strips and >= 3 row chunks, walls on every seam, raw values, poisoned walls;
# - the periodic rule on grids of fewer rows than K and of 1 and 2 columns, raw values;
# - the zero-flux rule on one row and on one column in both flavours;
# - 3-slab chains of 4-row slabs at K = 4, walls on the slabs' boundary rows, poisoned;
# - graph replay of >= 16 passes with row bands through a maze;
# - fused math at K = 3 with dt = 0.5 on a checkerboard, poisoned;
# - one fluid cell, and one wall, at each corner under every rule, by the marching and the single-step kernels;
# - padded pitches with raw values.
EDGE_EXAMPLES = ([pinned_case(cpl=c, fuse=k, cols=3 * tb_cols_per_wave(k, c) + 5, rows=3 * 16 + 3, rpb=16, p=OP_PARAMS, seed=c,
                              layout="seams", values="raw", poison=True) for c, k in ((1, 4), (2, 4), (4, 4), (4, 2))]
                 + [pinned_case(boundary=_P, rows=r, cols=n, cpl=c, p=OP_PARAMS, seed=r + n, values="raw", **lay)
                    for r, n in ((2, 61), (3, 37), (1, 130), (37, 1), (5, 2), (1, 1))
                    for lay in (dict(layout="random", share=0.5), dict(layout="checker")) for c in (4, 2)]
                 + [pinned_case(boundary=_N, rows=r, cols=n, p=OP_PARAMS, math=m, **lay)
                    for r, n in ((1, 61), (37, 1)) for m in (_STRICT, _FUSED)
                    for lay in (dict(layout="frame", flip=True), dict(layout="random"))]
                 + [pinned_case(boundary=b, rows=12, cols=300, slabs=3, kernel=k, math=m, p=OP_PARAMS, layout="seams", poison=True)
                    for b in (_C, _Z, _N) for k in (capi.GS_KERNEL_TB, capi.GS_KERNEL_AUTO) for m in (_STRICT, _FUSED)]
                 + [pinned_case(boundary=b, rows=60, cols=300, graph=1, split=2, calls=[11], p=p, layout="maze")
                    for b, p in ((_Z, OP_PARAMS), (_N, Parameters(time_step=0.5)))]
                 + [pinned_case(math=_FUSED, fuse=3, cpl=2, rows=50, cols=2 * tb_cols_per_wave(3, 2) + 1, rpb=16, p=HALF_DT,
                                boundary=b, layout="checker", poison=True) for b in (_C, _P)]
                 + [pinned_case(boundary=b, layout=lay, at=at, p=OP_PARAMS, values="raw" if lay == "one-wall" else "api", **run)
                    for lay in ("one-fluid", "one-wall") for b in RULES for at, run in _CORNER_RUNS.items()]
                 + [pinned_case(rows=33, cols=257, pitch_pad=pad, p=OP_PARAMS, values="raw") for pad in (3, 64)])


def counts_of(c):
    """What the run report counts an example under."""
    k = c["fuse"] if 1 <= c["fuse"] <= 4 else 4
    kernel, _, _, slabs, _, _, _ = legal(c)
    out = ["examples"]
    if c["values"] == "raw":
        out.append("raw values")
    if c["boundary"] == capi.GS_BOUNDARY_PERIODIC and (c["rows"] < k or c["cols"] <= 2):
        out.append("periodic with rows < K or cols <= 2")
    if slabs > 1:
        out.append("slab chains")
    return out


def _with_examples(test):
    for ex in reversed(EDGE_EXAMPLES):
        test = example(case=ex)(test)
    return test


def attach(sim, mask, values, shape):
    """The mask onto the context: Simulation.set_mask, or the raw field through gs_ctx_set_mask itself -- zeroed and
    destroyed at once, the library has its copy."""
    if values == "api":
        sim.set_mask(mask, shape=shape)
        return
    ctx = sim.context
    field = HipConcentration(ctx, shape)
    try:
        r0, r1 = field.local_rows()
        field.upload(ctx, np.ascontiguousarray(mask[r0:r1]))
        capi.check(ctx._lib.gs_ctx_set_mask(ctx.handle, field.handle))
        field.upload(ctx, np.zeros((r1 - r0, shape[1]), np.float32))
    finally:
        field.destroy()


def run_masked_case(c, u0, v0, mask):
    """The case on the GPU, refusals checked first.  Returns (U, V, kernel name, kernel, fuse_steps, slabs, what ran)."""
    kernel, fuse, rpb, slabs, split, at_create, at_mask = legal(c)
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
    elif at_mask:
        sim = Simulation.new(p, HipArgs(**drawn, **opts))
        try:
            with pytest.raises(GsError) as e:
                attach(sim, mask, c["values"], u0.shape)
            assert e.value.code == capi.GS_ERR_UNSUPPORTED, e.value
        finally:
            sim.context.close()
    if kernel in (capi.GS_KERNEL_STREAM, capi.GS_KERNEL_SIMPLE):
        fuse = 0
    sim = Simulation.new(p, HipArgs(kernel=kernel, fuse_steps=fuse, rows_per_block=rpb, split=split, devices=[0] * slabs, **opts))
    try:
        species = species_from_arrays(sim, u0, v0)
        attach(sim, mask, c["values"], u0.shape)
        for n in steps_of(c):
            if c["delivery"] == "step":
                for _ in range(n):
                    sim.perform_step(species)
            else:
                sim.perform_steps(species, n)
        iu, iv, _, _ = species.in_out()
        name = sim.context.info()[0]
        ran = (f"kernel={name} ({kernel}) fuse={fuse} rpb={rpb} split={split} slabs={slabs} {c['delivery']} calls={steps_of(c)} "
               + " ".join(f"{k}={v}" for k, v in opts.items()))
        return iu.make_scalar_view(sim.context), iv.make_scalar_view(sim.context), name, kernel, fuse, slabs, ran
    finally:
        sim.context.close()


def assert_fluid_matches(got, ref, fluid, exact, what):
    """The fluid cells of (U, V) `got` against `ref`: bit for bit, or (fused math on sub-normals) within 1e-37 absolute,
    NaN matching NaN."""
    for plane, g, r in (("U", got[0], ref[0]), ("V", got[1], ref[1])):
        if exact:
            assert_bits_equal(np.where(fluid, g, np.float32(0)), np.where(fluid, r, np.float32(0)), f"{plane} {what}")
            continue
        g, r = g.astype(np.float64), r.astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = ~fluid | (g == r) | (np.abs(g - r) <= 1e-37) | (np.isnan(g) & np.isnan(r))
        assert ok.all(), f"fused {plane} {what}: {int((~ok).sum())} cells beyond 1e-37, first at {np.argwhere(~ok)[0]}"


@pytest.fixture(scope="module", autouse=True)
def report():
    SEEN.clear()
    yield
    print("\nmask property examples: " + ", ".join(f"{k}: {v:.4g}" for k, v in sorted(SEEN.items())))


@settings(max_examples=int(os.environ.get("GS_PROPERTY_EXAMPLES_MASK", "120")), deadline=None, suppress_health_check=list(HealthCheck))
@given(mask_cases())
@_with_examples
def test_any_masked_schedule_matches_the_reference(built, case):
    c = dict(case)
    started = time.perf_counter()
    rows, cols, boundary, math, p = c["rows"], c["cols"], c["boundary"], c["math"], c["p"]
    u0, v0, walls, mask = fields_of(c)
    steps = sum(steps_of(c))
    strict = math == capi.GS_MATH_STRICT
    ref = R.run(u0, v0, steps, mask, params=params_of(p), boundary=boundary, ftz=strict)
    got_u, got_v, name, kernel, fuse, slabs, ran = run_masked_case(c, u0, v0, mask)
    SEEN.update(counts_of(c))
    SEEN.update({"pinned examples": 1} if case in EDGE_EXAMPLES else {})
    SEEN["seconds in pinned examples" if case in EDGE_EXAMPLES else "seconds in drawn examples"] += time.perf_counter() - started
    what = (f"{rows}x{cols} {ran} layout={c['layout']} share={c['share']} flip={c['flip']} at={c['at']} values={c['values']} "
            f"poison={c['poison']} tiny={c['tiny']} seed={c['seed']} {p}")
    assert name.split("@")[0].endswith(RULE_SUFFIX[boundary]), f"{name}: {what}"
    assert ".ds" not in name and ".dx" not in name, f"{name}: {what}"
    if c["delivery"] != "step" and kernel in (capi.GS_KERNEL_AUTO, capi.GS_KERNEL_TB):
        # (kernel = auto runs a pass of one step with the streaming kernel, as it does a gs_step: a call of one step, or
        # one step per pass -- fuse_steps = 1, or slabs of one row)
        single_steps = steps_of(c)[-1] == 1 or fuse == 1 or rows // slabs < 2
        assert name.startswith("tb-k") or (kernel == capi.GS_KERNEL_AUTO and single_steps and name.startswith("stream")), \
            f"{name}: {what}"
    if name.startswith("tb-k"):
        assert (".op" in name) == uses_op(p, math, c["general"], boundary, *tb_form(name)), f"{name}: {what}"
    # walls keep their bits, always
    assert got_u[walls].tobytes() == u0[walls].tobytes() and got_v[walls].tobytes() == v0[walls].tobytes(), f"walls changed: {what}"
    assert (R.walls_of(mask) == walls).all()
    fluid = ~walls
    exact = strict or not c["tiny"]
    assert_fluid_matches((got_u, got_v), ref, fluid, exact, what)
    if c["layout"] == "all-fluid":
        plain = rule_run(u0, v0, steps, oracle_params(p), boundary, ftz=strict)
        assert_fluid_matches((got_u, got_v), plain, fluid, exact, "against the unmasked reference: " + what)
    if c["layout"] == "all-wall":
        assert got_u.tobytes() == u0.tobytes() and got_v.tobytes() == v0.tobytes(), f"all walls: {what}"
