"""The parameter map's reference (gs_ctx_set_param_map): the reference step with feed = F[r, c] and kill = K[r, c] at cell
(r, c), restated from ``oracle.numpy_ref`` (whose ``step`` and ``step_zero_halo`` take per-cell ``feed`` / ``kill``
arrays as they are) without touching it.

* clipped rule: ``numpy_ref.step``; zero-halo rule: ``numpy_ref.step_zero_halo``;
* periodic and zero-flux rules: the state AND the map padded by one cell (``np.pad`` with ``mode="wrap"`` /
  ``mode="edge"``), one zero-halo step, crop -- one step at a time (a padded cell takes the map at its wrapped or
  clamped position, as the kernels do).

Strict math (``ftz=True``) runs under ``oracle.set_ftz(True)``: MXCSR.FTZ, the reference's DenormalsFlusher, for the
numpy arithmetic of the calling thread.  ``loop_step`` is the rule written literally, one cell at a time.

``linear(a, b, n)``: the driver's linear map values, ``np.float32(a + (b - a) * i / (n - 1))`` computed in float64,
a single value taking ``a``.
"""
from __future__ import annotations

import numpy as np

import oracle
from oracle import numpy_ref

CLIPPED, ZERO_HALO, PERIODIC, NEUMANN = 0, 1, 2, 3


def linear(a: float, b: float, n: int) -> np.ndarray:
    """n values from a to b (float64 arithmetic, rounded once to float32); n == 1 gives [a]."""
    if n == 1:
        return np.array([np.float32(a)], np.float32)
    i = np.arange(n, dtype=np.float64)
    return (float(a) + (float(b) - float(a)) * i / (n - 1)).astype(np.float32)


def plane(x, shape) -> np.ndarray:
    """A scalar as a uniform plane of ``shape``, an array as float32."""
    return np.full(shape, np.float32(x), np.float32) if np.ndim(x) == 0 else np.asarray(x, np.float32)


def params_of(p) -> dict:
    """``grayscott_amd.Parameters`` as the reference's parameter dict (every value rounded once to float32, as the C ABI's
    ``gs_params`` holds it)."""
    f = np.float32
    return dict(w=np.array(p.weights, np.float32), du=f(p.diffusion_rate_u), dv=f(p.diffusion_rate_v), feed=f(p.feed_rate),
                kill=f(p.kill_rate), dt=f(p.time_step))


# (F, K) pairs at the edges of the rates' range: +-0 feed, zero kill, a sub-normal feed, and feed + kill rounding to a
# sub-normal -- from two normal rates (3e-38 - 2.5e-38) and from two sub-normal ones -- which strict math must flush
EDGE_RATES = [(0.0, 0.06), (-0.0, 0.06), (0.03, 0.0), (0.03, -0.0), (0.0, 0.0), (-0.0, -0.0), (1e-39, 0.05), (-1e-39, 0.05),
              (3e-38, -2.5e-38), (1e-39, 2e-39)]


def planted_map(shape, rng, share: float = 0.3):
    """A random map (F in [0.01, 0.06], K in [0.04, 0.07]) with EDGE_RATES planted in about ``share`` of its cells."""
    feed = rng.uniform(0.01, 0.06, shape).astype(np.float32)
    kill = rng.uniform(0.04, 0.07, shape).astype(np.float32)
    pick = rng.integers(0, len(EDGE_RATES), shape)
    where = rng.random(shape) < share
    edge = np.array(EDGE_RATES, np.float32)
    feed[where], kill[where] = edge[pick[where], 0], edge[pick[where], 1]
    return feed, kill


def has_subnormal(*planes) -> bool:
    """Does any of the planes hold a sub-normal f32 (non-zero, below the smallest normal one)?"""
    tiny = np.finfo(np.float32).tiny
    return any(bool(np.any((x != 0) & (np.abs(x) < tiny))) for x in planes)


def _params(params, feed, kill):
    p = dict(params or numpy_ref.default_params())
    p["feed"], p["kill"] = feed, kill
    return p


def step(u, v, feed, kill, params: dict | None = None, boundary: int = CLIPPED):
    """One mapped step of boundary rule ``boundary`` (numpy arithmetic of the calling thread's float mode)."""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    feed, kill = plane(feed, u.shape), plane(kill, u.shape)
    if boundary == CLIPPED:
        return numpy_ref.step(u, v, _params(params, feed, kill))
    if boundary == ZERO_HALO:
        return numpy_ref.step_zero_halo(u, v, _params(params, feed, kill))
    mode = {PERIODIC: "wrap", NEUMANN: "edge"}[boundary]
    pad = [np.pad(x, 1, mode=mode) for x in (u, v, feed, kill)]
    pu, pv = numpy_ref.step_zero_halo(pad[0], pad[1], _params(params, pad[2], pad[3]))
    return pu[1:-1, 1:-1].copy(), pv[1:-1, 1:-1].copy()


def run(u, v, steps: int, feed, kill, params: dict | None = None, boundary: int = CLIPPED, ftz: bool = True):
    """``steps`` mapped steps; ``ftz``: strict math (sub-normal results flushed), else the fused flavour's contract on
    states without sub-normals."""
    prev = oracle.set_ftz(ftz)
    try:
        with np.errstate(all="ignore"):
            for _ in range(steps):
                u, v = step(u, v, feed, kill, params, boundary)
    finally:
        oracle.set_ftz(prev)
    return np.asarray(u, np.float32), np.asarray(v, np.float32)


def loop_step(u, v, feed, kill, params: dict | None = None, boundary: int = CLIPPED):
    """One mapped step, literally: per cell the rule's taps in row-major order from acc = 0, then the reaction with that
    cell's feed and kill, every operation one f32 operation (tiny grids only)."""
    p = params or numpy_ref.default_params()
    f = np.float32
    w = np.asarray(p["w"], np.float32)
    du, dv, dt = f(p["du"]), f(p["dv"]), f(p["dt"])
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    feed, kill = plane(feed, u.shape), plane(kill, u.shape)
    rows, cols = u.shape
    ou, ov = np.empty_like(u), np.empty_like(v)
    with np.errstate(all="ignore"):
        for r in range(rows):
            for c in range(cols):
                cu, cv = u[r, c], v[r, c]
                acc_u, acc_v = f(0), f(0)
                for i in range(3):
                    for j in range(3):
                        rr, cc = r + i - 1, c + j - 1
                        if boundary == CLIPPED:
                            if not (0 <= rr < rows and 0 <= cc < cols):
                                continue
                            # the window's weights are anchored at its top-left corner
                            wt = w[rr - max(r - 1, 0), cc - max(c - 1, 0)]
                            su, sv = u[rr, cc], v[rr, cc]
                        else:
                            wt = w[i, j]
                            if boundary == ZERO_HALO:
                                inside = 0 <= rr < rows and 0 <= cc < cols
                                su, sv = (u[rr, cc], v[rr, cc]) if inside else (f(0), f(0))
                            elif boundary == PERIODIC:
                                su, sv = u[rr % rows, cc % cols], v[rr % rows, cc % cols]
                            else:
                                rr, cc = min(max(rr, 0), rows - 1), min(max(cc, 0), cols - 1)
                                su, sv = u[rr, cc], v[rr, cc]
                        acc_u = f(acc_u + f(wt * f(su - cu)))
                        acc_v = f(acc_v + f(wt * f(sv - cv)))
                fr, kr = feed[r, c], kill[r, c]
                uv_square = f(f(cu * cv) * cv)
                d_u = f(f(f(du * acc_u) - uv_square) + f(fr * f(f(1) - cu)))
                d_v = f(f(f(dv * acc_v) + uv_square) - f(f(fr + kr) * cv))
                ou[r, c] = f(cu + f(d_u * dt))
                ov[r, c] = f(cv + f(d_v * dt))
    return ou, ov
