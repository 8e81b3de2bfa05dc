"""The zero-flux (Neumann) rule's reference, built from the zero-halo oracle without touching it.

One step of the zero-flux rule on an R x C grid is the central R x C block of one zero-halo step on the grid padded by
one copy of its edge cells (``np.pad(x, 1, mode="edge")``): a neighbour outside the grid is the nearest cell inside it.
``run`` does that one step at a time.  Unlike the periodic rule, a pad of n cells and n zero-halo steps is NOT n steps of
the rule: the padded cells evolve from their own neighbourhoods instead of staying copies of the edge
(``run_padded``, kept to show it).  ``clamp_step`` is the rule written literally, one cell at a time with every neighbour
read at clamped indices -- the CPU tests hold the pad-and-crop construction to it.
"""
from __future__ import annotations

import numpy as np

import oracle
from oracle import numpy_ref


def run(u, v, steps: int, params=None, ftz: bool = True):
    """``steps`` steps of the zero-flux rule through the C oracle's zero-halo rule (edge pad 1, step, crop)."""
    u = np.array(u, np.float32, copy=True)
    v = np.array(v, np.float32, copy=True)
    for _ in range(steps):
        pu, pv = oracle.run(np.pad(u, 1, mode="edge"), np.pad(v, 1, mode="edge"), 1, params=params, ftz=ftz,
                            boundary=oracle.ZERO_HALO)
        u, v = pu[1:-1, 1:-1].copy(), pv[1:-1, 1:-1].copy()
    return u, v


def run_padded(u, v, steps: int, params=None, ftz: bool = True):
    """One edge pad of ``steps`` cells, ``steps`` zero-halo steps, crop: NOT the rule for steps > 1 (the trap of fusing
    steps with the pad applied to the input only)."""
    if steps == 0:
        return np.array(u, np.float32), np.array(v, np.float32)
    n = steps
    pu, pv = oracle.run(np.pad(u, n, mode="edge"), np.pad(v, n, mode="edge"), n, params=params, ftz=ftz,
                        boundary=oracle.ZERO_HALO)
    return pu[n:-n, n:-n].copy(), pv[n:-n, n:-n].copy()


def run_numpy(u, v, steps: int, params: dict | None = None):
    """Pad and crop on ``oracle.numpy_ref.step_zero_halo`` (no flushing of sub-normal results)."""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    for _ in range(steps):
        pu, pv = numpy_ref.step_zero_halo(np.pad(u, 1, mode="edge"), np.pad(v, 1, mode="edge"), params)
        u, v = pu[1:-1, 1:-1], pv[1:-1, 1:-1]
    return u, v


def clamp_step(u, v, params: dict | None = None):
    """One step of the zero-flux rule, literally: per cell, the nine taps acc = acc + w[i][j] * (x[clamp(r + i - 1)]
    [clamp(c + j - 1)] - x[r][c]) in row-major order from acc = 0, then the reaction, every operation one f32 operation."""
    p = params or numpy_ref.default_params()
    f = np.float32
    w = np.asarray(p["w"], np.float32)
    du, dv, feed, kill, dt = (f(p[k]) for k in ("du", "dv", "feed", "kill", "dt"))
    rows, cols = u.shape
    ou, ov = np.empty_like(u), np.empty_like(v)
    with np.errstate(all="ignore"):
        for r in range(rows):
            for c in range(cols):
                cu, cv = u[r, c], v[r, c]
                acc_u, acc_v = f(0), f(0)
                for i in range(3):
                    for j in range(3):
                        rr, cc = min(max(r + i - 1, 0), rows - 1), min(max(c + j - 1, 0), cols - 1)
                        acc_u = f(acc_u + f(w[i, j] * f(u[rr, cc] - cu)))
                        acc_v = f(acc_v + f(w[i, j] * f(v[rr, cc] - cv)))
                uv_square = f(f(cu * cv) * cv)
                d_u = f(f(f(du * acc_u) - uv_square) + f(feed * f(f(1) - cu)))
                d_v = f(f(f(dv * acc_v) + uv_square) - f(f(feed + kill) * cv))
                ou[r, c] = f(cu + f(d_u * dt))
                ov[r, c] = f(cv + f(d_v * dt))
    return ou, ov
