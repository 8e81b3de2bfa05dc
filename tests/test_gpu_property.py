"""Randomised parity: hypothesis draws shapes, parameters, step counts, the boundary rule (all four), the arithmetic
flavour and scheduling options (kernel incl. the LDS-window kernel and its window shapes, fused steps, unit height, row
bands, in-process slabs, difference sharing, or nothing pinned at all: kernel = auto's own choice); every combination
must be bit-identical to its rule's reference (tests.helpers.rule_run) -- in fused math too, unless values near the
flush-to-zero threshold are sprinkled in, where the contract is 1e-37 absolute.  Scheduling options
never change results -- that is the property.  A combination a rule refuses must be refused with GS_ERR_UNSUPPORTED and
a message that names the rule; the example then runs its nearest legal case."""
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, example, given, settings, strategies as st

from grayscott_amd import GsError, Parameters, capi
from tests.helpers import assert_bits_equal, gpu_run, oracle_params, rule_of, rule_run
from tests.test_gpu_parity import args

pytestmark = pytest.mark.gpu

POW2 = [0.0, 0.125, 0.25, 0.5, 1.0]
RULES = [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_PERIODIC, capi.GS_BOUNDARY_NEUMANN]
RULE_WORD = {capi.GS_BOUNDARY_PERIODIC: "periodic", capi.GS_BOUNDARY_NEUMANN: "zero-flux"}


def tb_cols_per_wave(k, cpl):
    """Output columns of one strip of the marching kernel: gs_march.h's tb_cols_per_wave, (64 - 2 ceil(K / CPL)) CPL
    (its static_assert: 248 at K = 4, CPL = 4; 56 at K = 4, CPL = 1; 120 at K = 3, CPL = 2)."""
    return (64 - 2 * ((k + cpl - 1) // cpl)) * cpl


assert tb_cols_per_wave(4, 4) == 248 and tb_cols_per_wave(4, 1) == 56 and tb_cols_per_wave(3, 2) == 120


def refusal(boundary, kernel, slabs, split):
    """What gs_ctx_create refuses under `boundary`, as the words its message must hold; None where nothing is refused."""
    if boundary == capi.GS_BOUNDARY_PERIODIC and slabs > 1:
        return "single slab"
    if boundary in RULE_WORD and kernel == capi.GS_KERNEL_WINDOW:
        return "window"
    if boundary in RULE_WORD and kernel == capi.GS_KERNEL_LDS:
        return "LDS-staged"
    if boundary == capi.GS_BOUNDARY_PERIODIC and split > 1:
        return "row bands"
    return None


def run_case(u0, v0, steps, p, boundary, kernel, fuse, rpb, slabs, split, **kw):
    """gpu_run with the drawn options; a refused combination must fail as the rule says, then its nearest legal case
    (one slab, no split, kernel = auto) runs.  Returns (U, V, kernel name, what ran)."""
    what = refusal(boundary, kernel, slabs, split)
    if what is not None:
        with pytest.raises(GsError) as e:
            gpu_run(u0, v0, steps, params=p, args=args(kernel=kernel, fuse_steps=fuse, rows_per_block=rpb, split=split,
                                                        devices=[0] * slabs, boundary=boundary, **kw))
        assert e.value.code == capi.GS_ERR_UNSUPPORTED, e.value
        assert RULE_WORD[boundary] in str(e.value) and what in str(e.value), str(e.value)
        if kernel == capi.GS_KERNEL_WINDOW:  # (its fuse_steps / rows_per_block are steps per exchange / window rows)
            fuse = rpb = 0
        if kernel in (capi.GS_KERNEL_WINDOW, capi.GS_KERNEL_LDS) or slabs > 1 or split > 1:
            kernel = capi.GS_KERNEL_AUTO
        slabs, split = 1, 0
    got_u, got_v, info = gpu_run(u0, v0, steps, params=p,
                                 args=args(kernel=kernel, fuse_steps=fuse, rows_per_block=rpb, split=split,
                                           devices=[0] * slabs, boundary=boundary, **kw))
    ran = f"kernel={info[0]} fuse={fuse} rpb={rpb} split={split} slabs={slabs} " + " ".join(f"{k}={v}" for k, v in kw.items())
    return got_u, got_v, info[0], ran


def assert_rule_and_result(got_u, got_v, ref_u, ref_v, name, boundary, math, tiny, what):
    """The kernel that ran is the drawn rule's; strict math and fused math without sub-normal draws are bit-exact, fused
    math with them within 1e-37 absolute."""
    assert rule_of(name) == (boundary if boundary in RULE_WORD else capi.GS_BOUNDARY_CLIPPED), f"{name} under rule {boundary}"
    if math == capi.GS_MATH_STRICT or not tiny:
        assert_bits_equal(got_u, ref_u, "U " + what)
        assert_bits_equal(got_v, ref_v, "V " + what)
        return
    for plane, got, ref in (("U", got_u, ref_u), ("V", got_v, ref_v)):
        g, r = got.astype(np.float64), ref.astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = (g == r) | (np.abs(g - r) <= 1e-37) | (np.isnan(g) & np.isnan(r))
        assert ok.all(), f"fused {plane} {what}: {int((~ok).sum())} cells beyond 1e-37, first at {np.argwhere(~ok)[0]}"


def pinned_case(**kw):
    """A case of `cases` with every field at its plainest value but those given (the @example cases)."""
    base = dict(rows=17, cols=61, steps=11, seed=1, kernel=capi.GS_KERNEL_TB, fuse=4, rpb=8, split=0, slabs=1, p=Parameters(),
                tiny=False, cpl=0, general=0, graph=0, boundary=capi.GS_BOUNDARY_PERIODIC, tile_shape=0, math=capi.GS_MATH_STRICT,
                share_taps=0)
    base.update(kw)
    return base


@st.composite
def cases(draw):
    rows = draw(st.integers(1, 140))
    cols = draw(st.one_of(st.integers(1, 40), st.integers(240, 270), st.integers(480, 530), st.integers(990, 1040)))
    steps = draw(st.integers(1, 13))
    seed = draw(st.integers(0, 2 ** 16))
    kernel = draw(st.sampled_from([capi.GS_KERNEL_AUTO, capi.GS_KERNEL_AUTO, capi.GS_KERNEL_STREAM, capi.GS_KERNEL_TB, capi.GS_KERNEL_SIMPLE,
                                   capi.GS_KERNEL_LDS, capi.GS_KERNEL_TILE, capi.GS_KERNEL_WINDOW]))
    fuse = draw(st.integers(0, 8 if kernel == capi.GS_KERNEL_TILE else 4))
    tile_shape = draw(st.integers(0, 3))
    rpb = draw(st.sampled_from([0, 1, 2, 3, 5, 8, 16, 33]))
    if kernel == capi.GS_KERNEL_WINDOW:           # steps per exchange (even) and full window rows
        fuse = draw(st.sampled_from([0, 2, 4, 6, 8]))
        rpb = draw(st.sampled_from([0, 80]))
    split = draw(st.integers(0, 4))
    slabs = draw(st.integers(1, 4))
    cpl = draw(st.sampled_from([0, 1, 2, 4]))
    general = draw(st.integers(0, 1))
    graph = draw(st.integers(0, 1))
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
    w = [[draw(st.sampled_from(POW2)) for _ in range(3)] for _ in range(3)]
    if draw(st.booleans()):                       # the default side weights: specialised kernels
        w[0][1] = w[1][0] = w[1][2] = w[2][1] = 0.5
    p = Parameters(weights=tuple(tuple(r) for r in w),
                   diffusion_rate_u=draw(st.sampled_from([0.1, 0.2, 0.05])),
                   diffusion_rate_v=draw(st.sampled_from([0.05, 0.1])),
                   feed_rate=draw(st.sampled_from([0.014, 0.03, 0.0])),
                   kill_rate=draw(st.sampled_from([0.054, 0.06])),
                   time_step=draw(st.sampled_from([1.0, 0.5, 0.75])))
    tiny = draw(st.booleans())  # sprinkle values near the flush-to-zero threshold
    if kernel == capi.GS_KERNEL_AUTO and draw(st.booleans()):
        # nothing pinned, one slab: what kernel = auto picks by grid size (resident / window / marching kernel)
        fuse = rpb = split = cpl = graph = share_taps = 0
        slabs = 1
    return dict(rows=rows, cols=cols, steps=steps, seed=seed, kernel=kernel, fuse=fuse, rpb=rpb, split=split, slabs=slabs, p=p,
                tiny=tiny, cpl=cpl, general=general, graph=graph, boundary=boundary, tile_shape=tile_shape, math=math,
                share_taps=share_taps)


# The edge strips and row chunks that must always run: K = 4 at every CPL, one column past a full strip and a last row
# chunk of one row, under the periodic and zero-flux rules in both flavours; the fused LDS-window kernel at K = 8.
EDGE_EXAMPLES = ([pinned_case(boundary=b, cpl=c, cols=tb_cols_per_wave(4, c) + 1, rows=2 * 8 + 1, math=m)
                  for b in (capi.GS_BOUNDARY_PERIODIC, capi.GS_BOUNDARY_NEUMANN) for c in (1, 2, 4)
                  for m in (capi.GS_MATH_STRICT, capi.GS_MATH_FUSED)]
                 + [pinned_case(boundary=b, cpl=2, fuse=3, cols=2 * tb_cols_per_wave(3, 2) + 3, rows=3 * 16 + 2, rpb=16, share_taps=s)
                    for b in (capi.GS_BOUNDARY_PERIODIC, capi.GS_BOUNDARY_NEUMANN) for s in (1, 3)]
                 + [pinned_case(boundary=b, kernel=capi.GS_KERNEL_TILE, fuse=8, rpb=0, tile_shape=t, rows=70, cols=131,
                         math=capi.GS_MATH_FUSED, steps=13) for b in (capi.GS_BOUNDARY_PERIODIC, capi.GS_BOUNDARY_NEUMANN) for t in (1, 3)])


def _with_examples(test):
    for ex in reversed(EDGE_EXAMPLES):
        test = example(case=ex)(test)
    return test


@settings(max_examples=int(os.environ.get("GS_PROPERTY_EXAMPLES", "160")), deadline=None, suppress_health_check=list(HealthCheck))
@given(cases())
@_with_examples
def test_any_schedule_matches_the_oracle(built, case):
    c = dict(case)
    rows, cols, seed, p, tiny, boundary, math = c["rows"], c["cols"], c["seed"], c["p"], c["tiny"], c["boundary"], c["math"]
    steps = c["steps"] * 9 if c["graph"] else c["steps"]   # long enough for at least one batch of 16 passes
    slabs = min(c["slabs"], rows)
    kernel, fuse = c["kernel"], c["fuse"]
    rng = np.random.default_rng(seed)
    u0 = rng.random((rows, cols), dtype=np.float32)
    v0 = (rng.random((rows, cols), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    if tiny:
        mask = rng.random((rows, cols)) < 0.3
        v0[mask] = (v0[mask] * np.float32(1e-37)).astype(np.float32)
        u0[rng.random((rows, cols)) < 0.05] = np.float32(3e-38)
    if kernel in (capi.GS_KERNEL_STREAM, capi.GS_KERNEL_SIMPLE, capi.GS_KERNEL_LDS):
        fuse = 0
    ref_u, ref_v = rule_run(u0, v0, steps, oracle_params(p), boundary)
    got_u, got_v, name, ran = run_case(u0, v0, steps, p, boundary, kernel, fuse, c["rpb"], slabs, c["split"],
                                       cols_per_lane=c["cpl"], general_kernels=c["general"], use_graph=c["graph"],
                                       tile_shape=c["tile_shape"], math=math, share_taps=c["share_taps"])
    what = f"{rows}x{cols} steps={steps} {ran} boundary={boundary} tiny={tiny} {p}"
    assert_rule_and_result(got_u, got_v, ref_u, ref_v, name, boundary, math, tiny, what)


def _window_plan_exists(rows, cols, boundary, window_rows, k):
    """Is the grid one round of windows on this device (the planner's own answer, gs_debug_window_plan)?"""
    import ctypes

    import torch

    lib = capi.load()
    f = lib.gs_debug_window_plan
    f.restype = ctypes.c_int32
    f.argtypes = [ctypes.c_uint64, ctypes.c_uint64] + [ctypes.c_int32] * 5 + [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return f(rows, cols, cus, boundary, 1, window_rows, k, None, 0, None, None) > 0


@st.composite
def larger_cases(draw):
    """Grids from 40 k to 2.7 M cells: the window kernel's three windows, its hand-over to the marching kernel at
    1.5 M cells, single- and multi-round launches of the marching kernel (halved edge units, tapered tails)."""
    rows = draw(st.integers(200, 1300))
    cols = draw(st.integers(200, 2100))
    steps = draw(st.integers(1, 12))
    seed = draw(st.integers(0, 2 ** 16))
    kernel = draw(st.sampled_from([capi.GS_KERNEL_AUTO, capi.GS_KERNEL_AUTO, capi.GS_KERNEL_TB, capi.GS_KERNEL_TILE, capi.GS_KERNEL_WINDOW]))
    pinned = kernel != capi.GS_KERNEL_AUTO or draw(st.booleans())
    fuse = draw(st.integers(0, 8 if kernel == capi.GS_KERNEL_TILE else 4)) if pinned else 0
    rpb = draw(st.sampled_from([0, 0, 3, 8, 10, 16, 21, 39, 64])) if pinned else 0
    if kernel == capi.GS_KERNEL_WINDOW:           # (grids that are not one round of windows: the test falls back to auto)
        fuse = draw(st.sampled_from([0, 4, 8]))
        rpb = draw(st.sampled_from([0, 80]))
    cpl = draw(st.sampled_from([0, 1, 2, 4])) if pinned else 0
    slabs = draw(st.sampled_from([1, 1, 2, 3])) if pinned else 1
    tile_shape = draw(st.integers(0, 3))
    boundary = draw(st.sampled_from(RULES))
    default_params = draw(st.booleans())
    math = draw(st.sampled_from([capi.GS_MATH_STRICT, capi.GS_MATH_FUSED]))
    share_taps = draw(st.integers(0, 3)) if pinned else 0
    return rows, cols, steps, seed, kernel, fuse, rpb, cpl, slabs, tile_shape, boundary, default_params, math, share_taps


@settings(max_examples=int(os.environ.get("GS_PROPERTY_EXAMPLES_LARGER", "24")), deadline=None, suppress_health_check=list(HealthCheck))
@given(larger_cases())
def test_any_schedule_matches_the_oracle_larger_grids(built, case):
    rows, cols, steps, seed, kernel, fuse, rpb, cpl, slabs, tile_shape, boundary, default_params, math, share_taps = case
    rng = np.random.default_rng(seed)
    u0 = rng.random((rows, cols), dtype=np.float32)
    v0 = (rng.random((rows, cols), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    p = Parameters() if default_params else Parameters(feed_rate=0.03, kill_rate=0.06, time_step=0.5)
    ref_u, ref_v = rule_run(u0, v0, steps, oracle_params(p), boundary)
    if (kernel == capi.GS_KERNEL_WINDOW and slabs == 1 and boundary not in RULE_WORD
            and not _window_plan_exists(rows, cols, boundary, rpb, fuse)):
        kernel, fuse, rpb = capi.GS_KERNEL_AUTO, 0, 0
    got_u, got_v, name, ran = run_case(u0, v0, steps, p, boundary, kernel, fuse, rpb, slabs, 0, cols_per_lane=cpl,
                                       tile_shape=tile_shape, math=math, share_taps=share_taps)
    what = f"{rows}x{cols} steps={steps} {ran} boundary={boundary} default_params={default_params}"
    assert_rule_and_result(got_u, got_v, ref_u, ref_v, name, boundary, math, False, what)
