"""The noise term's reference (gs_ctx_set_noise; include/gs_hip.h holds the definition): Philox2x32-10 restated twice -- on
Python ints (``philox_int``) and vectorised on uint64 arrays (``philox``) --, the step key, the draw's value ``xi`` and the
noisy step: the per-rule restatement the other tests use (``tests.helpers.rule_run``: the C oracle for the clipped and
zero-halo rules, ``periodic_ref`` / ``neumann_ref`` for the other two) followed by one f32 multiply and one f32 add per
species.  Strict math (``ftz=True``) runs the two operations under ``oracle.set_ftz(True)`` -- MXCSR.FTZ for the numpy
arithmetic of the calling thread, as the existing references model the DenormalsFlusher: a sub-normal product or sum is
flushed.  A species whose sigma is 0 is not touched.

A noise term is a dict ``{"sigma_u", "sigma_v", "seed", "step"}``, as ``Simulation.noise()`` returns it.
"""
from __future__ import annotations

import numpy as np

import oracle

M = 0xD256D193
W = 0x9E3779B9
MASK32 = 0xFFFFFFFF

# (c0, c1, k) -> (x0, x1): Random123's known answers for philox2x32-10
KNOWN_ANSWERS = [((0x00000000, 0x00000000, 0x00000000), (0xFF1DAE59, 0x6CD10DF2)),
                 ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0x2C3F628B, 0xAB4FD7AD)),
                 ((0x243F6A88, 0x85A308D3, 0x13198A2E), (0xDD7CE038, 0xF62A4C12))]


def philox_int(c0: int, c1: int, k: int):
    """Philox2x32-10 on Python ints."""
    for i in range(10):
        if i:
            k = (k + W) & MASK32
        p = M * c0
        c0, c1 = ((p >> 32) ^ k ^ c1) & MASK32, p & MASK32
    return c0, c1


def philox(c0, c1, k):
    """Philox2x32-10 on arrays (broadcast against each other); returns two uint32 arrays."""
    c0 = np.asarray(c0).astype(np.uint64)
    c1 = np.asarray(c1).astype(np.uint64)
    k = np.asarray(k).astype(np.uint64)
    c0, c1, k = np.broadcast_arrays(c0, c1, k)
    m32 = np.uint64(MASK32)
    for i in range(10):
        if i:
            k = (k + np.uint64(W)) & m32
        p = np.uint64(M) * c0                       # < 2^64: both factors are below 2^32
        c0, c1 = ((p >> np.uint64(32)) ^ k ^ c1) & m32, p & m32
    return c0.astype(np.uint32), c1.astype(np.uint32)


def key(seed: int, s: int) -> int:
    """The step key of step ``s`` (u64) for ``seed`` (u64)."""
    seed &= 0xFFFFFFFFFFFFFFFF
    s &= 0xFFFFFFFFFFFFFFFF
    return philox_int(s & MASK32, s >> 32, seed & MASK32)[0] ^ (seed >> 32)


def xi(x) -> np.ndarray:
    """A draw as a value: the top 24 bits as a multiple of 2^-23 in [-1, 1); every operation exact in f32."""
    x = np.asarray(x, np.uint32)
    return ((x >> np.uint32(8)).astype(np.int32).astype(np.float32) - np.float32(8388608.0)) * np.float32(2.0 ** -23)


def draws(shape, seed: int, s: int, row0: int = 0, col0: int = 0):
    """(x0, x1) of every cell of a ``shape`` block whose first cell is global (row0, col0), in step ``s``."""
    rows = (np.arange(shape[0], dtype=np.uint64) + np.uint64(row0))[:, None]
    cols = (np.arange(shape[1], dtype=np.uint64) + np.uint64(col0))[None, :]
    return philox(cols, rows, key(seed, s))


def add_noise(nu, nv, noise: dict, s: int, ftz: bool = True):
    """The two noise operations of step ``s`` on the reference step's outputs."""
    nu, nv = np.asarray(nu, np.float32), np.asarray(nv, np.float32)
    su, sv = np.float32(noise["sigma_u"]), np.float32(noise["sigma_v"])
    if su == 0 and sv == 0:
        return nu, nv
    x0, x1 = draws(nu.shape, int(noise["seed"]), s)
    prev = oracle.set_ftz(ftz)
    try:
        with np.errstate(all="ignore"):
            if su != 0:
                nu = nu + su * xi(x0)
            if sv != 0:
                nv = nv + sv * xi(x1)
    finally:
        oracle.set_ftz(prev)
    return np.asarray(nu, np.float32), np.asarray(nv, np.float32)


def step(u, v, params, rule: int, noise: dict, s: int, ftz: bool = True):
    """One noisy step ``s`` under boundary rule ``rule`` (gs_boundary); ``params``: ``oracle.Params`` or None."""
    from .helpers import rule_run

    nu, nv = rule_run(np.asarray(u, np.float32), np.asarray(v, np.float32), 1, params=params, boundary=rule, ftz=ftz)
    return add_noise(nu, nv, noise, s, ftz)


def run(u, v, steps: int, noise: dict, params=None, rule: int = 0, ftz: bool = True):
    """``steps`` noisy steps from step ``noise["step"]`` on."""
    s0 = int(noise.get("step", 0))
    for i in range(steps):
        u, v = step(u, v, params, rule, noise, (s0 + i) & 0xFFFFFFFFFFFFFFFF, ftz)
    return np.asarray(u, np.float32), np.asarray(v, np.float32)
