"""The domain mask's reference (gs_ctx_set_mask): the reference step with walls, in numpy.

A cell is a wall where the mask is nonzero (NaN included).  A wall cell keeps its input bits.  Each tap of a fluid cell
reads one cell of the window as the boundary rule resolves it -- the clipped rule's clipped and shifted window
(compute/naive/src/lib.rs:52-70), the zero-halo rule's 0 outside the grid (never a wall), the periodic rule's wrapped
cell, the zero-flux rule's clamped cell -- and reads the centre's own value instead where that cell is a wall.  The taps,
their order and every rounding are the reference's.

``step`` is the vectorised form: the clipped rule as ``oracle.numpy_ref.step`` computes it (shifted planes, the weight
table anchored at the window's corner), the other rules over a copy padded by one cell (zeros and no walls, wrapped, or
clamped), nine taps in row-major order.  ``loop_step`` walks naive's window one cell at a time.  Strict math
(``ftz=True``) runs under ``oracle.set_ftz(True)``, MXCSR.FTZ, as ``tests/param_map_ref.py`` does.
"""
from __future__ import annotations

import numpy as np

import oracle
from oracle import numpy_ref

CLIPPED, ZERO_HALO, PERIODIC, NEUMANN = 0, 1, 2, 3


def walls_of(mask, shape=None) -> np.ndarray:
    """The wall cells of a mask: nonzero, NaN included (a scalar: a uniform plane of ``shape``)."""
    if np.ndim(mask) == 0:
        return np.full(shape, bool(mask != 0))
    return np.asarray(mask) != 0


def _shifted(a: np.ndarray, di: int, dj: int, fill):
    """(a[r + di, c + dj] where that exists, else ``fill``; where it exists)."""
    rows, cols = a.shape
    val = np.full(a.shape, fill, a.dtype)
    ok = np.zeros(a.shape, bool)
    rs, re = max(0, -di), min(rows, rows - di)
    cs, ce = max(0, -dj), min(cols, cols - dj)
    if rs < re and cs < ce:
        val[rs:re, cs:ce] = a[rs + di:re + di, cs + dj:ce + dj]
        ok[rs:re, cs:ce] = True
    return val, ok


def _react(p, u, v, acc_u, acc_v):
    f = np.float32
    uv_square = (u * v) * v
    du = (f(p["du"]) * acc_u - uv_square) + f(p["feed"]) * (f(1.0) - u)
    dv = (f(p["dv"]) * acc_v + uv_square) - (f(p["feed"]) + f(p["kill"])) * v
    return u + du * f(p["dt"]), v + dv * f(p["dt"])


def step(u, v, mask, params: dict | None = None, boundary: int = CLIPPED):
    """One masked step of boundary rule ``boundary`` (numpy arithmetic of the calling thread's float mode)."""
    p = params or numpy_ref.default_params()
    w = np.asarray(p["w"], np.float32)
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    wall = walls_of(mask, u.shape)
    rows, cols = u.shape
    acc_u, acc_v = np.zeros_like(u), np.zeros_like(v)
    if boundary == CLIPPED:
        oi = (np.arange(rows) > 0).astype(np.intp)[:, None]
        oj = (np.arange(cols) > 0).astype(np.intp)[None, :]
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                su, ok = _shifted(u, di, dj, 0)
                sv, _ = _shifted(v, di, dj, 0)
                sw, _ = _shifted(wall, di, dj, False)
                su, sv = np.where(sw, u, su), np.where(sw, v, sv)
                weight = np.broadcast_to(w[np.clip(oi + di, 0, 2), np.clip(oj + dj, 0, 2)], u.shape)
                acc_u = np.where(ok, acc_u + weight * (su - u), acc_u)
                acc_v = np.where(ok, acc_v + weight * (sv - v), acc_v)
    else:
        if boundary == ZERO_HALO:
            pu, pv, pw = np.pad(u, 1), np.pad(v, 1), np.pad(wall, 1)
        else:
            mode = {PERIODIC: "wrap", NEUMANN: "edge"}[boundary]
            pu, pv, pw = (np.pad(x, 1, mode=mode) for x in (u, v, wall))
        for i in range(3):
            for j in range(3):
                sw = pw[i:i + rows, j:j + cols]
                su = np.where(sw, u, pu[i:i + rows, j:j + cols])
                sv = np.where(sw, v, pv[i:i + rows, j:j + cols])
                acc_u = acc_u + w[i, j] * (su - u)
                acc_v = acc_v + w[i, j] * (sv - v)
    ou, ov = _react(p, u, v, acc_u, acc_v)
    return np.where(wall, u, ou).astype(np.float32), np.where(wall, v, ov).astype(np.float32)


def run(u, v, steps: int, mask, params: dict | None = None, boundary: int = CLIPPED, ftz: bool = True):
    """``steps`` masked steps; ``ftz``: strict math (sub-normal results flushed), else the fused flavour's contract on
    states without sub-normals."""
    prev = oracle.set_ftz(ftz)
    try:
        with np.errstate(all="ignore"):
            for _ in range(steps):
                u, v = step(u, v, mask, params, boundary)
    finally:
        oracle.set_ftz(prev)
    return np.asarray(u, np.float32), np.asarray(v, np.float32)


def loop_step(u, v, mask, params: dict | None = None, boundary: int = CLIPPED):
    """One masked step, literally: per fluid cell the rule's taps in row-major order from acc = 0 (a tap whose cell is a
    wall reads the centre), then the reaction, every operation one f32 operation; a wall cell copied (tiny grids only)."""
    p = params or numpy_ref.default_params()
    f = np.float32
    w = np.asarray(p["w"], np.float32)
    du, dv, dt, feed, kill = f(p["du"]), f(p["dv"]), f(p["dt"]), f(p["feed"]), f(p["kill"])
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    wall = walls_of(mask, u.shape)
    rows, cols = u.shape
    ou, ov = u.copy(), v.copy()
    with np.errstate(all="ignore"):
        for r in range(rows):
            for c in range(cols):
                if wall[r, c]:
                    continue
                cu, cv = u[r, c], v[r, c]
                acc_u, acc_v = f(0), f(0)
                if boundary == CLIPPED:  # naive's window, its weight table anchored at the window's corner
                    r0, c0 = max(r - 1, 0), max(c - 1, 0)
                    taps = [(w[rr - r0, cc - c0], rr, cc) for rr in range(r0, min(r + 2, rows)) for cc in range(c0, min(c + 2, cols))]
                else:
                    taps = []
                    for i in range(3):
                        for j in range(3):
                            rr, cc = r + i - 1, c + j - 1
                            if boundary == ZERO_HALO:
                                inside = 0 <= rr < rows and 0 <= cc < cols
                                taps.append((w[i, j], rr, cc) if inside else (w[i, j], None, None))
                            elif boundary == PERIODIC:
                                taps.append((w[i, j], rr % rows, cc % cols))
                            else:
                                taps.append((w[i, j], min(max(rr, 0), rows - 1), min(max(cc, 0), cols - 1)))
                for wt, rr, cc in taps:
                    if rr is None:
                        su, sv = f(0), f(0)
                    elif wall[rr, cc]:
                        su, sv = cu, cv
                    else:
                        su, sv = u[rr, cc], v[rr, cc]
                    acc_u = f(acc_u + f(wt * f(su - cu)))
                    acc_v = f(acc_v + f(wt * f(sv - cv)))
                uv_square = f(f(cu * cv) * cv)
                d_u = f(f(f(du * acc_u) - uv_square) + f(feed * f(f(1) - cu)))
                d_v = f(f(f(dv * acc_v) + uv_square) - f(f(feed + kill) * cv))
                ou[r, c] = f(cu + f(d_u * dt))
                ov[r, c] = f(cv + f(d_v * dt))
    return ou, ov


def maze(shape, rng) -> np.ndarray:
    """A mask of 1-cell walls worth measuring: wall lines on every 4th row and column, their crossings kept and half of
    their other cells opened at random -- about a quarter of the cells (a float32 array of 0 and 1)."""
    rows, cols = shape
    m = np.zeros(shape, np.float32)
    m[::4, :] = 1.0
    m[:, ::4] = 1.0
    holes = rng.random(shape) < 0.5
    m[holes & ((np.arange(rows)[:, None] % 4 == 0) ^ (np.arange(cols)[None, :] % 4 == 0))] = 0.0
    return m


def ring(shape, centre, r_in: float, r_out: float) -> np.ndarray:
    """A closed ring of walls (r_in <= distance from ``centre`` < r_out) as a float32 mask."""
    rr, cc = np.mgrid[0:shape[0], 0:shape[1]]
    d = np.hypot(rr - centre[0], cc - centre[1])
    return ((d >= r_in) & (d < r_out)).astype(np.float32)
