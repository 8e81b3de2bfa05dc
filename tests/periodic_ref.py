"""The periodic rule's reference, built from the zero-halo oracle without touching it.

n steps of the periodic rule on an R x C grid are the central R x C block of n zero-halo steps on the grid padded by
n cells of its own periodic extension (``np.pad(x, n, mode="wrap")``): the zero-halo rule's error at the padded edge
moves inward one cell per step and never reaches the centre.  One step at a time with a pad of 1 is the same thing and
is cheaper for long runs; that is what ``run`` does.  ``mod_step`` is the rule written literally, one cell at a time
with every neighbour read at its index modulo the grid's -- the CPU tests hold the pad-and-crop construction to it.
"""
from __future__ import annotations

import numpy as np

import oracle
from oracle import numpy_ref


def run(u, v, steps: int, params=None, ftz: bool = True):
    """``steps`` steps of the periodic rule through the C oracle's zero-halo rule (pad 1, step, crop)."""
    u = np.array(u, np.float32, copy=True)
    v = np.array(v, np.float32, copy=True)
    for _ in range(steps):
        pu, pv = oracle.run(np.pad(u, 1, mode="wrap"), np.pad(v, 1, mode="wrap"), 1, params=params, ftz=ftz,
                            boundary=oracle.ZERO_HALO)
        u, v = pu[1:-1, 1:-1].copy(), pv[1:-1, 1:-1].copy()
    return u, v


def run_padded(u, v, steps: int, params=None, ftz: bool = True):
    """The same by one pad of ``steps`` cells and ``steps`` zero-halo steps."""
    if steps == 0:
        return np.array(u, np.float32), np.array(v, np.float32)
    n = steps
    pu, pv = oracle.run(np.pad(u, n, mode="wrap"), np.pad(v, n, mode="wrap"), n, params=params, ftz=ftz,
                        boundary=oracle.ZERO_HALO)
    return pu[n:-n, n:-n].copy(), pv[n:-n, n:-n].copy()


def run_numpy(u, v, steps: int, params: dict | None = None):
    """Pad and crop on ``oracle.numpy_ref.step_zero_halo`` (no flushing of sub-normal results)."""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    for _ in range(steps):
        pu, pv = numpy_ref.step_zero_halo(np.pad(u, 1, mode="wrap"), np.pad(v, 1, mode="wrap"), params)
        u, v = pu[1:-1, 1:-1], pv[1:-1, 1:-1]
    return u, v


def mod_step(u, v, params: dict | None = None):
    """One step of the periodic rule, literally: per cell, the nine taps acc = acc + w[i][j] * (x[(r + i - 1) mod R]
    [(c + j - 1) mod C] - x[r][c]) in row-major order from acc = 0, then the reaction, every operation one f32 operation."""
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
                        rr, cc = (r + i - 1) % rows, (c + j - 1) % cols
                        acc_u = f(acc_u + f(w[i, j] * f(u[rr, cc] - cu)))
                        acc_v = f(acc_v + f(w[i, j] * f(v[rr, cc] - cv)))
                uv_square = f(f(cu * cv) * cv)
                d_u = f(f(f(du * acc_u) - uv_square) + f(feed * f(f(1) - cu)))
                d_v = f(f(f(dv * acc_v) + uv_square) - f(f(feed + kill) * cv))
                ou[r, c] = f(cu + f(d_u * dt))
                ov[r, c] = f(cv + f(d_v * dt))
    return ou, ov
