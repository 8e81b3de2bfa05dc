"""Edge units at rest (profiles/quiet_edges.md): under the clipped rule the units of the marching kernel
on the grid's edges -- first and last strips, chunks that touch the first or last rows, each of them as two half-height
units in a pass that may skip -- keep words like any other and are not recomputed while they and the positions around them
hold nothing but (U, V) = (1.0f, +0.0f); a position outside the grid counts as at rest.  The planes must be what they are
without it, bytes against bytes of ``oracle/libgs_oracle.so``, wherever a front enters an edge unit, a half of one or a
corner, whatever was written between two calls; the skipping must really happen (``Context.quiet_edge_stats()``), and
under the zero-halo rule it must not.

The layouts are the pinned one of tests/test_gpu_quiet_units.py (72 x 1440: 9 chunks of 8 rows x 12 strips of 120 columns,
halves of 4 rows = K) and variants of it: chunks of 6 rows (halves of 3 rows < K), a partial last strip with padding
columns behind it (1430 columns), two right-edge strips (1324 columns: the last strip owns 4), and a grid of two strips, on
which every unit is an edge unit (240 columns)."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from grayscott_amd import HipArgs, Parameters, Simulation, capi

from .helpers import assert_bits_equal, oracle_params, species_from_arrays

pytestmark = pytest.mark.gpu

K, WCOLS, SACRIFICIAL_COLS = 4, 120, 4
ONE = np.float32(1.0).view(np.uint32)
# name -> rows, columns, rows per chunk
LAYOUTS = {"8x1440": (72, 1440, 8), "6x1440": (72, 1440, 6), "8x1430": (72, 1430, 8), "8x1324": (72, 1324, 8), "8x240": (72, 240, 8)}


class Layout:
    def __init__(self, name):
        self.name = name
        self.rows, self.cols, self.rpu = LAYOUTS[name]
        self.chunks = self.rows // self.rpu
        self.strips = -(-self.cols // WCOLS)
        # a strip is a right-edge strip when its window, sacrificial lanes included, reaches the last column
        self.er = 2 if self.strips >= 2 and (self.strips - 1) * WCOLS + SACRIFICIAL_COLS >= self.cols else 1
        assert self.rows % self.rpu == 0 and self.rpu >= K  # only the last chunk touches the last rows: r1 + K > rows

    def args(self, **kw) -> HipArgs:
        return HipArgs(devices=[0], kernel=capi.GS_KERNEL_TB, rows_per_block=self.rpu, cols_per_lane=2, fuse_steps=K, **kw)

    def background(self):
        return np.ones((self.rows, self.cols), np.float32), np.zeros((self.rows, self.cols), np.float32)

    def edge(self):
        """[chunk, strip]: the position is on an edge of the grid (its units come as two halves in these launches)."""
        e = np.zeros((self.chunks, self.strips), bool)
        if self.strips <= 1 + self.er:
            e[:] = True
        else:
            e[0] = e[-1] = True
            e[:, 0] = True
            e[:, self.strips - self.er:] = True
        return e

    def rest_positions(self, u, v):
        """[chunk, strip]: every cell of the grid in the position is bitwise (1.0f, +0.0f)."""
        cell = np.ones((self.rows, self.strips * WCOLS), bool)
        cell[:, :self.cols] = (u.view(np.uint32) == ONE) & (v.view(np.uint32) == 0)
        return cell.reshape(self.chunks, self.rpu, self.strips, WCOLS).all(axis=(1, 3))


def with_patch(lay, r0, c0, u=None, v=None, h=6, w=10, uv=(0.5, 0.25)):
    if u is None:
        u, v = lay.background()
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


def assert_marching(sim):
    name, _ = sim.context.info()
    assert name.startswith("tb-k4c2/strict.op.dx"), name


_REST = {}


# The patch in the middle of every layout.  On the grid of two strips that leaves no position at rest -- the nine positions
# around any one span all columns and 24 of the 72 rows, and the front crosses them within 40 steps, by the reference --
# so that layout is also run with the patch in its first rows, where the floor is positive.
PLACES = [(name, "middle") for name in sorted(LAYOUTS)] + [("8x240", "top")]


def place(lay, where):
    return (lay.rows // 2 - 3 if where == "middle" else 0), lay.cols // 2 - 5


def resting(name, where):
    """By the oracle alone, for the patch of `where` on layout `name`: steps -> (edge positions, interior positions with
    interior positions all around them, and interior positions next to an edge, whose existing 3 x 3 neighbourhood of
    positions is at rest in every state of a call of that many steps; the final planes).  Computed once for the three step
    counts."""
    if (name, where) not in _REST:
        lay = Layout(name)
        u, v = with_patch(lay, *place(lay, where))
        rest = lay.rest_positions(u, v)
        edge = lay.edge()
        out = {}
        for step in range(1, 44):
            u, v = oracle.run(u, v, 1, ftz=True)
            rest &= lay.rest_positions(u, v)
            if step in (40, 41, 43):
                n_edge = n_deep = n_ring = 0
                for c in range(lay.chunks):
                    for s in range(lay.strips):
                        if rest[max(c - 1, 0):c + 2, max(s - 1, 0):s + 2].all():
                            if edge[c, s]:
                                n_edge += 1
                            elif edge[c - 1:c + 2, s - 1:s + 2].any():
                                n_ring += 1
                            else:
                                n_deep += 1
                out[step] = (n_edge, n_deep, n_ring, (u.copy(), v.copy()))
        _REST[(name, where)] = out
    return _REST[(name, where)]


@pytest.mark.parametrize("steps", [40, 41, 43])
@pytest.mark.parametrize("name,where", PLACES)
def test_rest_stays_rest_on_the_edges(built, name, where, steps):
    lay = Layout(name)
    n_edge, n_deep, n_ring, ref = resting(name, where)[steps]
    full = steps // K
    steady = full - 2
    # every edge position comes as two halves in these launches (one round of wave slots and less), and chunks of 8 or 6
    # rows have two halves: two units per position and steady pass
    floor = n_edge * steady * 2
    assert steady >= 8 and (n_edge >= 1 or (name, where) == ("8x240", "middle")), (n_edge, steady)  # by the reference alone
    u0, v0 = with_patch(lay, *place(lay, where))
    sim = Simulation.new(Parameters(), lay.args())
    sp = species_from_arrays(sim, u0, v0)
    sim.perform_steps(sp, steps)
    check(sim, sp, ref, f"{name} ({where}), {steps} steps")
    assert_marching(sim)
    launched, skipped, passes, steady_passes = sim.context.quiet_stats()
    edge_launched, edge_skipped, ring_skipped = sim.context.quiet_edge_stats()
    print(f"{name} ({where}) steps={steps}: launched={launched} (edge {edge_launched}) skipped: interior {skipped} + next to an "
          f"edge {ring_skipped}, edge {edge_skipped}; floor={floor}, resting interior positions {n_deep} + {n_ring}")
    assert passes == full and steady_passes == steady, (passes, steady_passes)
    n_edge_pos = int(lay.edge().sum())
    assert edge_launched == passes * 2 * n_edge_pos, (edge_launched, n_edge_pos)
    assert floor <= edge_skipped <= 2 * n_edge_pos * steady, (edge_skipped, floor)
    # the interior counts are bounded by the positions that can rest, as in tests/test_gpu_quiet_units.py: those with interior
    # positions all around them, and those next to an edge position
    inner = max(lay.chunks - 4, 0) * max(lay.strips - 3 - lay.er, 0) if lay.strips > 1 + lay.er else 0
    interior = (lay.chunks - 2) * (lay.strips - 1 - lay.er) if lay.strips > 1 + lay.er else 0
    assert n_deep * steady <= skipped <= inner * steady, (skipped, n_deep, inner)
    # (an interior unit next to an edge position reads that position's words, and those say "at rest" only when the edge
    # unit's whole input window rests: no floor from the positions alone)
    assert ring_skipped <= (interior - inner) * steady, (ring_skipped, interior, inner)
    sim.context.close()


# Where a front enters an edge unit, on the pinned layout (chunks of 8 rows, strips of 120 columns) unless said otherwise.
FRONTS = {
    "2 cells inside the top edge": ("8x1440", 2, 700),
    "2 cells inside the bottom edge": ("8x1440", 64, 700),
    "2 cells inside the left edge": ("8x1440", 33, 2),
    "2 cells inside the right edge": ("8x1440", 33, 1428),
    "top-left corner": ("8x1440", 2, 2),
    "top-right corner": ("8x1440", 2, 1428),
    "bottom-left corner": ("8x1440", 64, 2),
    "bottom-right corner": ("8x1440", 64, 1428),
    "rows 0..": ("8x1440", 0, 300),
    "columns 0..": ("8x1440", 40, 0),
    "rows 0.. and columns 0..": ("8x1440", 0, 0),
    "the last rows and columns": ("8x1440", 66, 1430),
    "seam between the left edge strip and its neighbour": ("8x1440", 30, 115),
    "seam between the top edge chunk and its neighbour": ("8x1440", 5, 500),
    "inside half 1, next to the half seam (left strip)": ("8x1440", 36, 50),
    "inside half 1 of the top chunk, next to the half seam": ("8x1440", 4, 820),
    "halves of 3 rows: inside half 1 of the bottom chunk": ("6x1440", 69, 400),
    "halves of 3 rows: inside half 1, left strip": ("6x1440", 33, 20),
    "padding columns: 2 cells inside the right edge": ("8x1430", 30, 1418),
    "padding columns: the last rows and columns": ("8x1430", 66, 1420),
    "two right-edge strips: in the strip of 4 columns": ("8x1324", 20, 1314),
    "two right-edge strips: in the strip before it": ("8x1324", 60, 1250),
    "two strips: the seam between them": ("8x240", 33, 115),
    "two strips: top-right corner": ("8x240", 2, 228),
}


@pytest.mark.parametrize("where", sorted(FRONTS))
def test_a_front_enters_an_edge_unit(built, where):
    name, r0, c0 = FRONTS[where]
    lay = Layout(name)
    u0, v0 = with_patch(lay, r0, c0)
    sim = Simulation.new(Parameters(), lay.args())
    sp = species_from_arrays(sim, u0, v0)
    u, v = u0, v0
    for call in range(16):
        sim.perform_steps(sp, 4)
        u, v = oracle.run(u, v, 4, ftz=True)
        check(sim, sp, (u, v), f"{where}: call {call}")
    one = species_from_arrays(sim, u0, v0)
    sim.perform_steps(one, 64)
    check(sim, one, (u, v), f"{where}: one call of 64 steps")
    assert_marching(sim)
    print(where, sim.context.quiet_stats(), sim.context.quiet_edge_stats())
    assert sim.context.quiet_edge_stats()[1] > 0
    sim.context.close()


# what is written between two calls: into an edge unit (left strip), into a corner, and next to the padding columns
WRITES = {"left edge strip": ("8x1440", 26, 3), "bottom-right corner": ("8x1440", 67, 1425), "padding-adjacent column": ("8x1430", 26, 1419)}


@pytest.mark.parametrize("writer", ["fill_slice", "upload"])
@pytest.mark.parametrize("target", sorted(WRITES))
def test_calls_do_not_inherit(built, target, writer):
    name, r0, c0 = WRITES[target]
    lay = Layout(name)
    u0, v0 = with_patch(lay, 33, 655)
    sim = Simulation.new(Parameters(), lay.args())
    ctx = sim.context
    sp = species_from_arrays(sim, u0, v0)
    sim.perform_steps(sp, 24)
    u, v = oracle.run(u0, v0, 24, ftz=True)
    check(sim, sp, (u, v), "first call")
    assert ctx.quiet_edge_stats()[1] > 0
    c, s = r0 // lay.rpu, c0 // WCOLS
    assert lay.edge()[c, s] and lay.rest_positions(u, v)[max(c - 1, 0):c + 2, max(s - 1, 0):s + 2].all()  # that unit was skipped
    in_u, in_v, _, _ = sp.in_out()
    if writer == "fill_slice":
        in_u.fill_slice(ctx, [range(r0, r0 + 4), range(c0, c0 + 11)], 0.3)
        in_v.fill_slice(ctx, [range(r0, r0 + 4), range(c0, c0 + 11)], 0.6)
        u[r0:r0 + 4, c0:c0 + 11] = np.float32(0.3)
        v[r0:r0 + 4, c0:c0 + 11] = np.float32(0.6)
    else:
        u, v = with_patch(lay, r0, c0, u, v, h=4, w=11, uv=(0.3, 0.6))
        in_u.upload(ctx, u)
        in_v.upload(ctx, v)
    sim.perform_steps(sp, 24)
    check(sim, sp, oracle.run(u, v, 24, ftz=True), f"second call after {writer} into the {target}")
    ctx.close()


@pytest.mark.parametrize("name", ["8x1440", "8x1430"])
def test_zero_halo_rule(built, name):
    lay = Layout(name)
    u0, v0 = with_patch(lay, 33, 655)
    sim = Simulation.new(Parameters(), lay.args(boundary=capi.GS_BOUNDARY_ZERO_HALO))
    sp = species_from_arrays(sim, u0, v0)
    sim.perform_steps(sp, 40)
    check(sim, sp, oracle.run(u0, v0, 40, ftz=True, boundary=oracle.ZERO_HALO), "zero halo")
    assert_marching(sim)
    assert sim.context.quiet_edge_stats()[1:] == (0, 0), sim.context.quiet_edge_stats()
    assert sim.context.quiet_stats()[1] > 0
    sim.context.close()


def hip_run(lay, u0, v0, steps, params, args):
    sim = Simulation.new(params, args)
    sp = species_from_arrays(sim, u0, v0)
    sim.perform_steps(sp, steps)
    out = planes(sim, sp)
    stats = sim.context.quiet_stats(), sim.context.quiet_edge_stats()
    sim.context.close()
    return out, stats


def test_switched_off(built, monkeypatch):
    lay = Layout("8x1440")
    u0, v0 = with_patch(lay, 2, 2)
    on, on_stats = hip_run(lay, u0, v0, 40, Parameters(), lay.args())
    assert on_stats[0][1] > 0 and on_stats[1][1] > 0, on_stats
    monkeypatch.setenv("GS_HIP_QUIET_UNITS", "0")
    off, off_stats = hip_run(lay, u0, v0, 40, Parameters(), lay.args())
    assert off_stats == ((0, 0, 0, 0), (0, 0, 0)), off_stats
    ref = oracle.run(u0, v0, 40, ftz=True)
    for got in (on, off):
        assert_bits_equal(got[0], ref[0], "U")
        assert_bits_equal(got[1], ref[1], "V")


def test_another_stencil_and_other_rates(built):
    """The five-point stencil with F, k and dt of its own (whichever entries such parameters take)."""
    lay = Layout("8x1440")
    params = Parameters.with_stencil("5points", feed_rate=0.03, kill_rate=0.06, time_step=0.75)
    for r0, c0 in ((2, 2), (33, 655)):
        u0, v0 = with_patch(lay, r0, c0)
        got, stats = hip_run(lay, u0, v0, 40, params, lay.args())
        print("5points", (r0, c0), stats)
        ref = oracle.run(u0, v0, 40, params=oracle_params(params), ftz=True)
        assert_bits_equal(got[0], ref[0], "U")
        assert_bits_equal(got[1], ref[1], "V")


def random_case(rng, lay):
    u, v = lay.background()
    for _ in range(int(rng.integers(1, 4))):
        h, w = int(rng.integers(1, 9)), int(rng.integers(1, 40))
        kind = int(rng.integers(4))
        if kind == 0:  # on an edge or in a corner of the grid
            r0 = int(rng.choice([0, lay.rows - h, int(rng.integers(0, lay.rows - h + 1))]))
            c0 = int(rng.choice([0, lay.cols - w, int(rng.integers(0, lay.cols - w + 1))]))
        elif kind == 1:  # astride a seam of units or of halves
            r0 = int(rng.integers(1, 2 * lay.chunks)) * (lay.rpu // 2) - int(rng.integers(0, h + 1))
            c0 = int(rng.integers(1, lay.strips)) * WCOLS - int(rng.integers(0, w + 1))
        else:
            r0, c0 = int(rng.integers(0, lay.rows - h + 1)), int(rng.integers(0, lay.cols - w + 1))
        r0, c0 = max(0, min(r0, lay.rows - h)), max(0, min(c0, lay.cols - w))
        u[r0:r0 + h, c0:c0 + w] = rng.random((h, w), dtype=np.float32)
        v[r0:r0 + h, c0:c0 + w] = rng.random((h, w), dtype=np.float32) * np.float32(0.5)
    return u, v


def test_randomised(built):
    rng = np.random.default_rng(20240917)
    sims = {}
    for case in range(20):
        name = sorted(LAYOUTS)[int(rng.integers(len(LAYOUTS)))]
        lay = Layout(name)
        if name not in sims:
            sims[name] = Simulation.new(Parameters(), lay.args())
        sim = sims[name]
        u, v = random_case(rng, lay)
        sp = species_from_arrays(sim, u, v)
        calls = int(rng.integers(1, 4))
        left = int(rng.integers(8, 65))
        for call in range(calls):
            steps = left if call == calls - 1 else int(rng.integers(1, max(2, left - (calls - 1 - call))))
            left -= steps
            sim.perform_steps(sp, steps)
            u, v = oracle.run(u, v, steps, ftz=True)
            check(sim, sp, (u, v), f"case {case} on {name}, call {call} ({steps} steps)")
        for c in sp.u._pair + sp.v._pair:
            c.destroy()
    total = 0
    for name, sim in sims.items():
        print(name, "quiet_stats", sim.context.quiet_stats(), "quiet_edge_stats", sim.context.quiet_edge_stats())
        total += sim.context.quiet_edge_stats()[1]
        sim.context.close()
    assert total > 0
