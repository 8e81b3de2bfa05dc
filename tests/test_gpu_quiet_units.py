"""Units at rest (profiles/quiet_units.md): the full passes of a ``gs_run`` leave the units of the
marching kernel whose input window and output rows hold nothing but (U, V) = (1.0f, +0.0f) alone.  The planes must be
what they are without it, bytes against bytes, wherever a front enters such a unit, whatever was written between two
calls, and the skipping must really happen (``Context.quiet_stats()``).

The layout is pinned so that the 4-wave march with difference sharing across lanes runs on a small grid and does not
tune: 72 x 1440 cells = 9 chunks of 8 rows x 12 strips of 120 columns.  Chunks 0 and 8 and strips 0 and 11 are edge units,
which never rest; positions with chunk 2..6 and strip 2..9 have an all-interior neighbourhood and are the only ones that
can skip."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from grayscott_amd import HipArgs, Parameters, Simulation, capi

from .helpers import assert_bits_equal, oracle_params, species_from_arrays

pytestmark = pytest.mark.gpu

ROWS, COLS, RPU, WCOLS = 72, 1440, 8, 120
CHUNKS, STRIPS = ROWS // RPU, COLS // WCOLS
ONE = np.float32(1.0).view(np.uint32)


def pinned(**kw) -> HipArgs:
    return HipArgs(devices=[0], kernel=capi.GS_KERNEL_TB, rows_per_block=RPU, cols_per_lane=2, fuse_steps=4, **kw)


def background():
    return np.ones((ROWS, COLS), np.float32), np.zeros((ROWS, COLS), np.float32)


def with_patch(r0, c0, u=None, v=None, h=6, w=10, uv=(0.5, 0.25)):
    if u is None:
        u, v = background()
    u[r0:r0 + h, c0:c0 + w] = np.float32(uv[0])
    v[r0:r0 + h, c0:c0 + w] = np.float32(uv[1])
    return u, v


def planes(sim, sp):
    in_u, in_v, _, _ = sp.in_out()
    return in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)


def check(sim, sp, ref, what):
    got_u, got_v = planes(sim, sp)
    assert_bits_equal(got_u, ref[0], what + " U")
    assert_bits_equal(got_v, ref[1], what + " V")


def rest_positions(u, v):
    """[chunk, strip]: every cell of the position is bitwise (1.0f, +0.0f)."""
    cell = (u.view(np.uint32) == ONE) & (v.view(np.uint32) == 0)
    return cell.reshape(CHUNKS, RPU, STRIPS, WCOLS).all(axis=(1, 3))


def resting_neighbourhoods(u, v, steps):
    """Positions among chunk 2..6 x strip 2..9 whose 3 x 3 neighbourhood of positions is at rest in every state of a call of
    `steps` steps from (u, v), by the oracle; and the oracle's final planes."""
    rest = rest_positions(u, v)
    for _ in range(steps):
        u, v = oracle.run(u, v, 1, ftz=True)
        rest &= rest_positions(u, v)
    n = sum(bool(rest[c - 1:c + 2, s - 1:s + 2].all()) for c in range(2, 7) for s in range(2, 10))
    return n, (u, v)


def assert_marching(sim):
    name, _ = sim.context.info()
    assert name.startswith("tb-k4c2/strict.op.dx"), name


@pytest.mark.parametrize("steps", [40, 41, 43])
def test_rest_stays_rest_and_the_patch_is_right(built, steps):
    u0, v0 = with_patch(33, 655)  # the middle of the unit of chunk 4, strip 5
    full = steps // 4
    n, ref = resting_neighbourhoods(u0, v0, steps)
    floor = n * (full - 2)
    assert n >= 10 and full - 2 >= 8, (n, full)  # by the reference alone
    sim = Simulation.new(Parameters(), pinned())
    sp = species_from_arrays(sim, u0, v0)
    sim.perform_steps(sp, steps)
    check(sim, sp, ref, f"{steps} steps")
    assert_marching(sim)
    launched, skipped, passes, steady = sim.context.quiet_stats()
    print(f"steps={steps}: launched={launched} skipped={skipped} passes={passes} steady={steady} floor={floor}")
    assert passes == full and steady == full - 2, (passes, steady)
    assert launched >= passes * CHUNKS * STRIPS
    assert floor <= skipped <= 40 * steady, (skipped, floor)
    sim.context.close()


# the patch 2 cells from a row seam and 2 from a column seam of the unit of chunk 4 (rows 32..39), strip 5 (columns 600..719)
CORNERS = {"top-left": (34, 602), "top-right": (34, 708), "bottom-left": (32, 602), "bottom-right": (32, 708)}


@pytest.mark.parametrize("corner", sorted(CORNERS))
def test_a_front_enters_a_unit_at_rest(built, corner):
    r0, c0 = CORNERS[corner]
    u0, v0 = with_patch(r0, c0)
    sim = Simulation.new(Parameters(), pinned())
    sp = species_from_arrays(sim, u0, v0)
    u, v = u0, v0
    for call in range(16):
        sim.perform_steps(sp, 4)
        u, v = oracle.run(u, v, 4, ftz=True)
        check(sim, sp, (u, v), f"{corner}: call {call}")
    one = species_from_arrays(sim, u0, v0)
    sim.perform_steps(one, 64)
    check(sim, one, (u, v), f"{corner}: one call of 64 steps")
    assert_marching(sim)
    assert sim.context.quiet_stats()[1] > 0
    sim.context.close()


@pytest.mark.parametrize("writer", ["fill_slice", "upload", "other species"])
def test_calls_do_not_inherit(built, writer):
    u0, v0 = with_patch(33, 655)
    sim = Simulation.new(Parameters(), pinned())
    ctx = sim.context
    sp = species_from_arrays(sim, u0, v0)
    sim.perform_steps(sp, 24)
    u, v = oracle.run(u0, v0, 24, ftz=True)
    check(sim, sp, (u, v), "first call")
    assert ctx.quiet_stats()[1] > 0
    assert rest_positions(u, v)[2:5, 7:10].all()  # the unit of chunk 3, strip 8 was skipped: its neighbourhood rests
    in_u, in_v, _, _ = sp.in_out()
    if writer == "fill_slice":
        in_u.fill_slice(ctx, [range(26, 30), range(1000, 1011)], 0.3)
        in_v.fill_slice(ctx, [range(26, 30), range(1000, 1011)], 0.6)
        u[26:30, 1000:1011] = np.float32(0.3)
        v[26:30, 1000:1011] = np.float32(0.6)
    elif writer == "upload":
        u, v = with_patch(26, 1000, u, v, h=4, w=11, uv=(0.3, 0.6))
        in_u.upload(ctx, u)
        in_v.upload(ctx, v)
    else:
        rng = np.random.default_rng(5)
        ou = rng.random((ROWS, COLS), dtype=np.float32)
        ov = (rng.random((ROWS, COLS), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
        other = species_from_arrays(sim, ou, ov)
        sim.perform_steps(other, 24)
        check(sim, other, oracle.run(ou, ov, 24, ftz=True), "the other species")
    sim.perform_steps(sp, 24)
    check(sim, sp, oracle.run(u, v, 24, ftz=True), "second call after " + writer)
    ctx.close()


def random_case(rng, case):
    u, v = background()
    for _ in range(int(rng.integers(1, 7))):
        h, w = int(rng.integers(1, 9)), int(rng.integers(1, 40))
        if rng.integers(3) == 0:  # astride a seam or a corner of units
            r0 = int(rng.integers(1, CHUNKS)) * RPU - int(rng.integers(0, h + 1)) if rng.integers(2) else int(rng.integers(0, ROWS - h))
            c0 = int(rng.integers(1, STRIPS)) * WCOLS - int(rng.integers(0, w + 1))
        else:
            r0, c0 = int(rng.integers(0, ROWS - h)), int(rng.integers(0, COLS - w))
        r0, c0 = max(0, min(r0, ROWS - h)), max(0, min(c0, COLS - w))
        u[r0:r0 + h, c0:c0 + w] = rng.random((h, w), dtype=np.float32)
        v[r0:r0 + h, c0:c0 + w] = rng.random((h, w), dtype=np.float32) * np.float32(0.5)
    if case % 5 == 1:  # V = -0.0 in an otherwise resting unit: not at rest
        v[42:45, 1210:1230] = np.float32(-0.0)
    if case % 5 == 3:  # U = 1, V = a sub-normal
        v[18:21, 300:330] = np.float32(1e-40)
    return u, v


def test_randomised(built):
    rng = np.random.default_rng(20240611)
    sim = Simulation.new(Parameters(), pinned())
    for case in range(20):
        u, v = random_case(rng, case)
        sp = species_from_arrays(sim, u, v)
        for call in range(int(rng.integers(1, 4))):
            steps = int(rng.integers(12, 61))
            sim.perform_steps(sp, steps)
            u, v = oracle.run(u, v, steps, ftz=True)
            check(sim, sp, (u, v), f"case {case}, call {call} ({steps} steps)")
        for c in sp.u._pair + sp.v._pair:
            c.destroy()
    print("quiet_stats", sim.context.quiet_stats())
    assert sim.context.quiet_stats()[1] > 0
    sim.context.close()


def hip_run(u0, v0, steps, params, args, map_=None):
    sim = Simulation.new(params, args)
    if map_ is not None:
        sim.set_param_map(map_[0], map_[1], shape=(ROWS, COLS))
    sp = species_from_arrays(sim, u0, v0)
    sim.perform_steps(sp, steps)
    out = planes(sim, sp)
    stats = sim.context.quiet_stats()
    sim.context.close()
    return out, stats


NAN_WEIGHTS = ((float("nan"), 0.5, 0.25), (0.5, 0.0, 0.5), (0.25, 0.5, 0.25))
OFF = {
    "feed = +inf": dict(params=Parameters(feed_rate=float("inf"))),
    "a weight = NaN": dict(params=Parameters(weights=NAN_WEIGHTS)),
    "the periodic rule": dict(boundary=capi.GS_BOUNDARY_PERIODIC),
    "a parameter map": dict(map_=(0.014, 0.054)),
    "GS_HIP_QUIET_UNITS=0": dict(env="0"),
}


@pytest.mark.parametrize("what", sorted(OFF))
def test_off_where_it_must_be(built, monkeypatch, what):
    case = OFF[what]
    params = case.get("params", Parameters())
    boundary = case.get("boundary", capi.GS_BOUNDARY_CLIPPED)
    u0, v0 = with_patch(33, 655)
    if "env" in case:
        on, on_stats = hip_run(u0, v0, 40, params, pinned())
        assert on_stats[1] > 0
        monkeypatch.setenv("GS_HIP_QUIET_UNITS", case["env"])
    got, stats = hip_run(u0, v0, 40, params, pinned(boundary=boundary), case.get("map_"))
    assert stats[1] == 0, stats
    ref, _ = hip_run(u0, v0, 40, params, HipArgs(devices=[0], kernel=capi.GS_KERNEL_STREAM, boundary=boundary), case.get("map_"))
    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes(), what
    if "env" in case:
        assert stats == (0, 0, 0, 0), stats
        assert got[0].tobytes() == on[0].tobytes() and got[1].tobytes() == on[1].tobytes()


def test_zero_halo_rule(built):
    u0, v0 = with_patch(33, 655)
    sim = Simulation.new(Parameters(), pinned(boundary=capi.GS_BOUNDARY_ZERO_HALO))
    sp = species_from_arrays(sim, u0, v0)
    sim.perform_steps(sp, 40)
    check(sim, sp, oracle.run(u0, v0, 40, ftz=True, boundary=oracle.ZERO_HALO), "zero halo")
    assert_marching(sim)
    assert sim.context.quiet_stats()[1] > 0
    sim.context.close()
