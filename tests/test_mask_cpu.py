"""Domain masks without a GPU: the masked reference of tests/mask_ref.py held to the literal per-cell loop (random masks,
all four rules, small and degenerate shapes, FTZ on and off), to the unmasked references (an all-fluid mask) and to the
identity (an all-wall mask); the new symbol is exported and declared, the ABI version is unchanged; the simulate driver's
``--hip-mask`` option and its refusal next to the parameter map's options."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

import oracle
from grayscott_amd import capi, simulate

from . import mask_ref as R
from .helpers import rule_run, stress_fields
from tests.children import ROOT

RULES = [R.CLIPPED, R.ZERO_HALO, R.PERIODIC, R.NEUMANN]


def random_mask(shape, rng, share=0.3):
    """Walls in about ``share`` of the cells, written as 1, -2.5 or NaN; fluid as +0 or -0."""
    m = np.where(rng.random(shape) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    walls = rng.random(shape) < share
    m[walls] = np.array([1.0, -2.5, np.nan], np.float32)[rng.integers(0, 3, int(walls.sum()))]
    return m


@pytest.mark.parametrize("ftz", [True, False])
@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 3), (4, 4), (5, 7), (9, 6)])
def test_vectorised_reference_is_the_literal_loop(shape, boundary, ftz):
    rng = np.random.default_rng(11)
    u, v = stress_fields(shape, 4)
    for trial in range(3):
        mask = random_mask(shape, rng, share=(0.2, 0.5, 0.8)[trial])
        prev = oracle.set_ftz(ftz)
        try:
            want = R.loop_step(u, v, mask, boundary=boundary)
            got = R.step(u, v, mask, boundary=boundary)
        finally:
            oracle.set_ftz(prev)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (trial, shape, boundary)
        u, v = want


@pytest.mark.parametrize("boundary", RULES)
def test_literal_loop_at_other_parameters(boundary):
    """A centre weight, asymmetric weights and dt != 1: every tap's weight and position matters."""
    p = oracle.numpy_ref.default_params()
    p["w"] = np.array([[0.25, 0.5, 0.125], [1.0, -3.0, 0.75], [0.0625, 0.375, 0.0]], np.float32)
    p["dt"] = np.float32(0.5)
    rng = np.random.default_rng(5)
    u, v = stress_fields((6, 5), 6)
    mask = random_mask((6, 5), rng)
    want = R.loop_step(u, v, mask, p, boundary)
    got = R.step(u, v, mask, p, boundary)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("boundary", RULES)
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (3, 5), (17, 33)])
def test_all_fluid_mask_is_the_unmasked_rule(shape, boundary):
    u0, v0 = stress_fields(shape, 1)
    ref_u, ref_v = rule_run(u0, v0, 5, boundary=boundary)
    fluid = np.where(np.random.default_rng(2).random(shape) < 0.5, np.float32(0.0), np.float32(-0.0))
    for mask in (fluid, 0.0):
        got_u, got_v = R.run(u0, v0, 5, mask, boundary=boundary)
        assert got_u.tobytes() == ref_u.tobytes() and got_v.tobytes() == ref_v.tobytes()


@pytest.mark.parametrize("boundary", RULES)
def test_all_wall_mask_is_the_identity(boundary):
    u0, v0 = stress_fields((9, 11), 2)
    u0[0, 0] = np.float32(np.nan)
    for mask in (np.full((9, 11), np.nan, np.float32), 1.0):
        got_u, got_v = R.run(u0, v0, 3, mask, boundary=boundary)
        assert got_u.tobytes() == u0.tobytes() and got_v.tobytes() == v0.tobytes()


def test_walls_are_nonzero_cells():
    m = np.array([[0.0, -0.0, np.nan, 1e-45, -1.0, np.inf]], np.float32)
    assert R.walls_of(m).tolist() == [[False, False, True, True, True, True]]


def test_maze_walls_about_a_quarter_of_the_cells():
    m = R.maze((256, 256), np.random.default_rng(0))
    assert 0.2 < float(m.mean()) < 0.3


# ---- the randomised GPU parity test's own pieces (tests/test_gpu_mask_property.py), without a GPU -------------------------
def test_the_mask_property_strategy_draws_legal_cases_of_every_kind():
    """The cases tests/test_gpu_mask_property.py draws (no library call): legal option sets after the refusals; every
    rule, flavour, K, CPL, kernel, delivery, layout, way of handing the mask over and poison among a few hundred of them,
    periodic grids of fewer rows than K and of 1 or 2 columns too; and on every drawn shape each layout is what it claims."""
    from hypothesis import HealthCheck, given, settings

    from . import test_gpu_mask_property as P

    seen = set()

    @settings(max_examples=400, deadline=None, database=None, suppress_health_check=list(HealthCheck))
    @given(P.mask_cases())
    def draw(case):
        kernel, fuse, _, slabs, _, _, _ = P.legal(case)
        seen.update({("rule", case["boundary"]), ("math", case["math"]), ("k", fuse), ("cpl", case["cpl"]),
                     ("kernel", case["kernel"]), ("delivery", case["delivery"]), ("layout", case["layout"]),
                     ("values", case["values"]), ("poison", case["poison"]), ("ran", kernel), ("slabs>1", slabs > 1)})
        seen.update(("count", what) for what in P.counts_of(case))
        if case["boundary"] == R.PERIODIC:
            seen.update({("periodic rows<=3", case["rows"] <= 3), ("periodic cols<=3", case["cols"] <= 3)})
        shape = (case["rows"], case["cols"])
        for kind in {case["layout"], P.LAYOUTS[case["seed"] % len(P.LAYOUTS)]}:
            check_layout(P, kind, shape, case)

    draw()
    for case in P.EDGE_EXAMPLES:
        P.legal(case)
        check_layout(P, case["layout"], (case["rows"], case["cols"]), case)
    want = ({("rule", b) for b in RULES} | {("math", m) for m in (capi.GS_MATH_STRICT, capi.GS_MATH_FUSED)}
            | {("k", k) for k in range(5)} | {("cpl", c) for c in (0, 1, 2, 4)}
            | {("kernel", k) for k in (capi.GS_KERNEL_AUTO, capi.GS_KERNEL_TB, capi.GS_KERNEL_STREAM, capi.GS_KERNEL_SIMPLE,
                                       capi.GS_KERNEL_TILE, capi.GS_KERNEL_WINDOW, capi.GS_KERNEL_LDS)}
            | {("delivery", d) for d in P.DELIVERIES} | {("layout", k) for k in P.LAYOUTS} | {("values", v) for v in P.VALUES}
            | {("poison", False), ("poison", True), ("slabs>1", True), ("periodic rows<=3", True), ("periodic cols<=3", True)})
    assert want <= seen, sorted(want - seen, key=str)
    assert not {("ran", k) for k in P.NO_MASK_FORM} & seen


def check_layout(P, kind, shape, case):
    """`make_walls` yields what the layout claims (drawn twice from one seed: the same plane)."""
    rows, cols = shape
    walls = P.make_walls(kind, shape, np.random.default_rng(case["seed"]), case)
    assert walls.dtype == np.bool_ and walls.shape == shape
    assert (walls == P.make_walls(kind, shape, np.random.default_rng(case["seed"]), case)).all()
    ring = np.ones(shape, bool)
    ring[1:-1, 1:-1] = False
    if kind == "all-fluid":
        assert not walls.any()
    elif kind == "all-wall":
        assert walls.all()
    elif kind == "one-fluid":
        assert int((~walls).sum()) == 1
    elif kind == "one-wall":
        assert int(walls.sum()) == 1
    if kind in ("one-fluid", "one-wall") and case["at"]:
        r, c = np.argwhere(walls == (kind == "one-wall"))[0]
        assert r in (0, rows // 2, rows - 1) and c in (0, cols // 2, cols - 1) and (r in (0, rows - 1) or c in (0, cols - 1))
    elif kind == "frame":
        assert (walls[ring] != case["flip"]).all() and (walls[~ring] == case["flip"]).all()
    elif kind == "checker":
        assert not walls[0, 0] and (cols < 2 or walls[0, 1] != case["flip"]) and (cols < 3 or walls[0, 2] == case["flip"])
        assert rows < 3 or cols < 3 or walls[2, 2] == walls[0, 0]
    elif kind == "seams":
        line_cols, line_rows = P.seam_lines(shape, case)
        k = case["fuse"] if 1 <= case["fuse"] <= 4 else 4
        w = P.tb_cols_per_wave(k, case["cpl"] or 4)
        assert all(x in line_cols for m in range(1, cols // w + 1) for x in (m * w - 1, m * w, m * w + 1) if x < cols)
        rpb, slabs = case["rpb"] or 16, min(case["slabs"], rows)
        assert all(x in line_rows for m in range(1, rows // rpb + 1) for x in (m * rpb - 1, m * rpb) if x < rows)
        assert all(x in line_rows for i in range(1, slabs) for x in (int(round(i * rows / slabs)) - 1, int(round(i * rows / slabs)))
                   if 0 <= x < rows)
        on_line = np.zeros(shape, bool)
        on_line[:, line_cols] = True
        on_line[line_rows, :] = True
        assert not (walls & ~on_line).any()
        assert P.seams_are_mixed(walls, line_cols, line_rows)       # a wall and a gap on every line of >= 8 cells
    elif kind == "maze":
        assert walls[0, 0] and walls[::4, ::4].all()


def layout_cases(P):
    """Every layout kind with its variants, as cases whose seams reach tiny grids (chunks of 2 rows, 2 slabs)."""
    out = [dict(layout="random", share=s) for s in P.SHARES]
    out += [dict(layout=k, flip=f) for k in ("frame", "checker") for f in (False, True)]
    out += [dict(layout=k, at=at) for k in ("one-fluid", "one-wall") for at in (None, "nw", "se", "n", "w")]
    out += [dict(layout=k) for k in ("all-fluid", "all-wall", "seams", "maze")]
    return [P.pinned_case(rpb=2, slabs=2, **kw) for kw in out]


@pytest.mark.parametrize("ftz", [True, False])
@pytest.mark.parametrize("boundary", RULES)
def test_new_layouts_are_the_literal_loop(boundary, ftz):
    """The layouts of the randomised GPU test, raw mask values and poisoned walls at tiny and degenerate shapes: the
    vectorised reference, the literal loop and the fault model without a fault agree bit for bit, walls keep their bits."""
    from . import test_gpu_mask_property as P

    q = P.params_of(P.OP_PARAMS)
    for shape in ((1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (5, 2), (3, 5)):
        for n, base in enumerate(layout_cases(P)):
            case = dict(base, rows=shape[0], cols=shape[1], seed=100 + n, values="raw", poison=True)
            u, v, walls, mask = P.fields_of(case)
            assert (R.walls_of(mask) == walls).all()
            prev = oracle.set_ftz(ftz)
            try:
                for _ in range(3):
                    want = R.loop_step(u, v, mask, q, boundary)
                    got = R.step(u, v, mask, q, boundary)
                    mine = faulty_step(None, u, v, mask, q, boundary)
                    for a, b in ((got, want), (mine, want)):
                        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (shape, base["layout"], n)
                    assert want[0][walls].tobytes() == u[walls].tobytes() and want[1][walls].tobytes() == v[walls].tobytes()
                    u, v = want
            finally:
                oracle.set_ftz(prev)


# ---- the pinned examples discriminate -------------------------------------------------------------------------------------
# Single faults of a masked step.  The model is the device's (domain masks): a link word per cell with a bit per
# window position -- wrapped under the periodic rule, never set outside the grid under the others -- and the rule's own
# edge handling on top: the zero-flux rule's clamped neighbour takes the bit of the in-grid position it is clamped to.
TAP_FAULTS = [f"tap({i},{j})" for i in range(3) for j in range(3) if (i, j) != (1, 1)]   # that tap ignores the wall
FAULTS = TAP_FAULTS + ["transposed",        # link bit (i, j) is taken for (j, i)
                       "no-wrap",           # a wall seen only through the periodic wrap is ignored
                       "clamp",             # zero flux: the wall of the clamped neighbour is ignored
                       "not-held",          # wall cells are updated like fluid
                       "zero-for-wall",     # a tap on a wall reads 0 instead of the centre
                       "subnormal-fluid"]   # sub-normal mask values count as fluid (raw values only)


def faulty_walls(fault, mask, shape):
    wall = R.walls_of(mask, shape)
    if fault == "subnormal-fluid" and np.asarray(mask).dtype == np.float32:
        magnitude = np.asarray(mask).view(np.uint32) & np.uint32(0x7fffffff)
        wall = wall & ~((magnitude != 0) & (magnitude < np.uint32(0x00800000)))
    return wall


def tap_flags(fault, wall, boundary):
    """Per tap (i, j) of every cell: does the tap exist (the clipped rule drops taps outside the grid), which cell it
    reads (row, column; None: the zero-halo rule's 0 outside the grid), and `flag`: is what it reads taken for a wall."""
    rows, cols = wall.shape
    rr, cc = np.mgrid[0:rows, 0:cols]
    link = np.zeros((3, 3) + wall.shape, bool)
    outside = np.zeros((3, 3) + wall.shape, bool)
    for i in range(3):
        for j in range(3):
            pr, pc = rr + i - 1, cc + j - 1
            outside[i, j] = (pr < 0) | (pr >= rows) | (pc < 0) | (pc >= cols)
            if boundary == R.PERIODIC:
                link[i, j] = wall[pr % rows, pc % cols]
            else:
                link[i, j] = ~outside[i, j] & wall[np.clip(pr, 0, rows - 1), np.clip(pc, 0, cols - 1)]
    if fault == "no-wrap" and boundary == R.PERIODIC:
        link &= ~outside
    if fault in TAP_FAULTS:
        link[int(fault[4]), int(fault[6])] = False
    if fault == "transposed":
        link = link.transpose(1, 0, 2, 3).copy()
    taps = {}
    for i in range(3):
        for j in range(3):
            pr, pc = rr + i - 1, cc + j - 1
            exists, flag, zero = np.ones(wall.shape, bool), link[i, j], np.zeros(wall.shape, bool)
            if boundary == R.CLIPPED:
                exists = ~outside[i, j]
            elif boundary == R.ZERO_HALO:
                zero = outside[i, j]
            elif boundary == R.PERIODIC:
                pr, pc = pr % rows, pc % cols
            else:
                pr, pc = np.clip(pr, 0, rows - 1), np.clip(pc, 0, cols - 1)
                flag = link[pr - rr + 1, pc - cc + 1, rr, cc]           # the bit of the position the tap is clamped to
                if fault == "clamp":
                    flag = flag & ~outside[i, j]
            taps[i, j] = (exists, np.clip(pr, 0, rows - 1), np.clip(pc, 0, cols - 1), zero, flag)
    return taps


def faulty_step(fault, u, v, mask, p, boundary):
    """One masked step with the single fault `fault` (None: the reference's step, by the link-word model)."""
    f = np.float32
    w = np.asarray(p["w"], np.float32)
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    wall = faulty_walls(fault, mask, u.shape)
    rows, cols = u.shape
    oi = (np.arange(rows) > 0).astype(np.intp)[:, None]
    oj = (np.arange(cols) > 0).astype(np.intp)[None, :]
    acc_u, acc_v = np.zeros_like(u), np.zeros_like(v)
    taps = tap_flags(fault, wall, boundary)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                exists, pr, pc, zero, flag = taps[i, j]
                su, sv = np.where(zero, f(0), u[pr, pc]), np.where(zero, f(0), v[pr, pc])
                su = np.where(flag, f(0) if fault == "zero-for-wall" else u, su)
                sv = np.where(flag, f(0) if fault == "zero-for-wall" else v, sv)
                if boundary == R.CLIPPED:   # the weight table anchored at the window's corner
                    weight = np.broadcast_to(w[np.clip(oi + i - 1, 0, 2), np.clip(oj + j - 1, 0, 2)], u.shape)
                else:
                    weight = w[i, j]
                acc_u = np.where(exists, acc_u + weight * (su - u), acc_u)
                acc_v = np.where(exists, acc_v + weight * (sv - v), acc_v)
        ou, ov = R._react(p, u, v, acc_u, acc_v)
    if fault == "not-held":
        return ou.astype(np.float32), ov.astype(np.float32)
    return np.where(wall, u, ou).astype(np.float32), np.where(wall, v, ov).astype(np.float32)


def fault_applies(fault, mask, walls, boundary, values):
    """Can `fault` show at all: does it change what some existing tap of a fluid cell takes for a wall (or, for the faults
    that leave the taps alone, is there a wall, a tap on a wall, a sub-normal mask value)?"""
    fluid = ~walls
    true = tap_flags(None, walls, boundary)
    if fault == "not-held":
        return bool(walls.any())
    if fault == "zero-for-wall":
        return any(bool((t[0] & t[4] & fluid).any()) for t in true.values())
    if fault == "subnormal-fluid":
        return values == "raw" and bool((faulty_walls(fault, mask, walls.shape) != walls).any())
    if (fault == "no-wrap" and boundary != R.PERIODIC) or (fault == "clamp" and boundary != R.NEUMANN):
        return False
    other = tap_flags(fault, walls, boundary)
    return any(bool((true[k][0] & fluid & (true[k][4] != other[k][4])).any()) for k in true)


_discrimination_cache = {}


def discrimination(n):
    """Pinned example `n` on the CPU: (the true result's fluid cells are finite, has fluid and wall cells, a fluid cell has
    a wall neighbour in the rule's sense, {fault: caught} for the faults that apply).  A fault is caught when the whole
    run with the fault at every step, one faulty step from the input state and one faulty last step from the true state
    before it each change at least one bit."""
    if n in _discrimination_cache:
        return _discrimination_cache[n]
    from . import test_gpu_mask_property as P

    c = P.EDGE_EXAMPLES[n]
    u0, v0, walls, mask = P.fields_of(c)
    boundary, q, steps = c["boundary"], P.params_of(c["p"]), sum(P.steps_of(c))
    ftz = c["math"] == capi.GS_MATH_STRICT
    before = R.run(u0, v0, steps - 1, mask, params=q, boundary=boundary, ftz=ftz)
    true = R.run(before[0], before[1], 1, mask, params=q, boundary=boundary, ftz=ftz)
    first = R.run(u0, v0, 1, mask, params=q, boundary=boundary, ftz=ftz)
    fluid = ~walls
    finite = bool(np.isfinite(true[0][fluid]).all() and np.isfinite(true[1][fluid]).all())
    linked = any(bool((t[0] & t[4] & fluid).any()) for t in tap_flags(None, walls, boundary).values())

    def differs(a, b):
        return a[0].tobytes() != b[0].tobytes() or a[1].tobytes() != b[1].tobytes()

    caught = {}
    prev = oracle.set_ftz(ftz)
    try:
        assert not differs(faulty_step(None, u0, v0, mask, q, boundary), first)
        for fault in FAULTS:
            if not fault_applies(fault, mask, walls, boundary, c["values"]):
                continue
            state = (u0, v0)
            for _ in range(steps):
                state = faulty_step(fault, state[0], state[1], mask, q, boundary)
            caught[fault] = (differs(state, true) and differs(faulty_step(fault, u0, v0, mask, q, boundary), first)
                             and differs(faulty_step(fault, before[0], before[1], mask, q, boundary), true))
    finally:
        oracle.set_ftz(prev)
    out = (finite, bool(fluid.any() and walls.any()), linked, caught)
    _discrimination_cache[n] = out
    return out


def _pinned_count():
    from . import test_gpu_mask_property as P

    return len(P.EDGE_EXAMPLES)


@pytest.mark.parametrize("n", range(_pinned_count()))
def test_pinned_example_discriminates(n):
    """Caps that keep the GPU test from passing vacuously: (a) the true reference's fluid cells are finite at the end,
    (b) with a fluid and a wall cell on the grid some fluid cell has a wall neighbour in the rule's sense, (c) every fault
    that applies changes at least one bit."""
    finite, mixed, linked, caught = discrimination(n)
    assert finite
    assert linked or not mixed
    assert all(caught.values()), sorted(f for f, ok in caught.items() if not ok)


def test_every_fault_is_caught_by_three_pinned_examples():
    """... and across the list every fault is caught by at least 3 examples; raw mask values, periodic grids of fewer
    rows than K or at most 2 columns and slab chains are all among them, whatever the random draws give."""
    from . import test_gpu_mask_property as P

    catches = {f: [n for n in range(len(P.EDGE_EXAMPLES)) if discrimination(n)[3].get(f)] for f in FAULTS}
    assert all(len(v) >= 3 for v in catches.values()), {f: v for f, v in catches.items() if len(v) < 3}
    counts = {}
    for c in P.EDGE_EXAMPLES:
        for what in P.counts_of(c):
            counts[what] = counts.get(what, 0) + 1
    assert all(counts.get(k, 0) > 0 for k in ("raw values", "periodic with rows < K or cols <= 2", "slab chains")), counts


def test_the_symbol_is_exported_and_declared(built):
    assert "gs_ctx_set_mask" in capi.EXPORTS
    lib = ctypes.CDLL(os.path.join(ROOT, "grayscott_amd", "libgs_hip.so"))
    assert hasattr(lib, "gs_ctx_set_mask")
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    assert re.search(r"int32_t gs_ctx_set_mask\(gs_ctx \*ctx, gs_field \*mask\);", header)
    assert "pub fn gs_ctx_set_mask(" in open(os.path.join(ROOT, "rust", "compute_hip", "src", "ffi.rs")).read()
    assert "set_mask(" in open(os.path.join(ROOT, "include", "grayscott_hip.hpp")).read()
    lib.gs_abi_version.restype = ctypes.c_int32
    assert lib.gs_abi_version() == 4


def test_detach_without_a_context_is_refused(built):
    lib = capi.load()
    assert lib.gs_ctx_set_mask(None, None) == capi.GS_ERR_INVALID


def test_driver_option(tmp_path):
    m = (np.arange(24).reshape(4, 6) % 5 == 0).astype(np.int8)
    npy = tmp_path / "m.npy"
    np.save(npy, m)
    args = simulate.parse(["-r", "4", "-c", "6", "--hip-mask", str(npy)])
    got = simulate.domain_mask(args, (4, 6))
    assert got.shape == (4, 6) and (got == m).all()
    npz = tmp_path / "m.npz"
    np.savez(npz, mask=m.astype(np.float32))
    args = simulate.parse(["-r", "4", "-c", "6", "--hip-mask", str(npz)])
    assert (simulate.domain_mask(args, (4, 6)) == m).all()
    # no option: no mask
    args = simulate.parse([])
    assert simulate.domain_mask(args, (args.nbrow, args.nbcol)) is None
    # the wrong shape, a .npz without `mask`
    args = simulate.parse(["-r", "5", "-c", "6", "--hip-mask", str(npy)])
    with pytest.raises(ValueError):
        simulate.domain_mask(args, (5, 6))
    bad = tmp_path / "bad.npz"
    np.savez(bad, walls=m)
    with pytest.raises(ValueError):
        simulate.domain_mask(simulate.parse(["-r", "4", "-c", "6", "--hip-mask", str(bad)]), (4, 6))


@pytest.mark.parametrize("extra", [["--hip-feed-map", "0.01:0.05"], ["--hip-kill-map", "0.06:0.04"], ["--hip-param-map", "x.npz"]])
def test_driver_refuses_a_mask_with_a_parameter_map(tmp_path, extra):
    npy = tmp_path / "m.npy"
    np.save(npy, np.zeros((4, 6), np.float32))
    args = simulate.parse(["-r", "4", "-c", "6", "--hip-mask", str(npy)] + extra)
    with pytest.raises(ValueError, match="--hip-mask excludes"):
        simulate.domain_mask(args, (4, 6))
