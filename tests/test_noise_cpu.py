"""The noise term's definition on the CPU (tests/noise_ref.py; no GPU): the generator's known answers, the two restatements
against each other, the exactness and the first two moments of the draws, and the layout of ``gs_noise``."""
from __future__ import annotations

import ctypes
import math
import os
import re

import numpy as np

from grayscott_amd import capi

from . import noise_ref as N
from tests.children import ROOT

# seeds for the moment checks: fixed, so the checks are deterministic
MEAN_SEED = 2024
VAR_SEED = 7


def test_known_answers():
    for (c0, c1, k), want in N.KNOWN_ANSWERS:
        assert N.philox_int(c0, c1, k) == want, (hex(c0), hex(c1), hex(k))
        got = N.philox(np.array([c0]), np.array([c1]), np.array([k]))
        assert (int(got[0][0]), int(got[1][0])) == want


def test_int_and_numpy_restatements_agree():
    rng = np.random.default_rng(1)
    t = rng.integers(0, 2 ** 32, (10_000, 3), dtype=np.uint64)
    x0, x1 = N.philox(t[:, 0], t[:, 1], t[:, 2])
    for i in range(t.shape[0]):
        assert N.philox_int(int(t[i, 0]), int(t[i, 1]), int(t[i, 2])) == (int(x0[i]), int(x1[i])), i


def test_xi_is_exact():
    x0, x1 = N.draws((512, 512), 3, 5)
    for x in (x0, x1, np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)):
        v = N.xi(x).astype(np.float64) * 2.0 ** 23
        assert np.all(v == np.floor(v)) and v.min() >= -(2 ** 23) and v.max() < 2 ** 23
        # ... and is the top 24 bits, re-centred
        assert np.array_equal(v.astype(np.int64), (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.int64) - 2 ** 23)
    assert N.xi(np.uint32(0)) == -1.0 and N.xi(np.uint32(0xFFFFFFFF)) == np.float32(1.0 - 2.0 ** -23)


def test_mean_of_a_fixed_draw():
    n = 512 * 512
    for x in N.draws((512, 512), MEAN_SEED, 0):
        assert abs(float(N.xi(x).astype(np.float64).mean())) <= 6.0 / math.sqrt(3.0 * n)


def test_variance_of_a_fixed_draw():
    for x in N.draws((512, 512), VAR_SEED, 0):
        var = float(N.xi(x).astype(np.float64).var())
        assert abs(var - 1.0 / 3.0) <= 0.01 / 3.0, var


def test_u_and_v_draws_differ():
    x0, x1 = N.draws((64, 64), 11, 0)
    assert not np.any(x0 == x1) or np.count_nonzero(x0 == x1) <= 1
    assert not np.array_equal(N.xi(x0), N.xi(x1))


def test_keys_of_consecutive_steps_differ():
    for seed in (0, 1, 0xDEADBEEFCAFEF00D):
        keys = [N.key(seed, s) for s in list(range(64)) + [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 64 - 1]]
        assert len(set(keys)) == len(keys), seed
    # the high word of the step and of the seed both count
    assert N.key(5, 1) != N.key(5, 1 + 2 ** 32) and N.key(5, 1) != N.key(5 + 2 ** 32, 1)


def test_steps_and_seeds_give_different_planes():
    a = N.xi(N.draws((32, 32), 1, 0)[0])
    assert not np.array_equal(a, N.xi(N.draws((32, 32), 1, 1)[0]))
    assert not np.array_equal(a, N.xi(N.draws((32, 32), 2, 0)[0]))
    # a block's draws are the global ones at its position (slabs, row bands)
    whole = N.draws((40, 50), 9, 3)
    part = N.draws((10, 20), 9, 3, row0=7, col0=13)
    assert np.array_equal(part[0], whole[0][7:17, 13:33]) and np.array_equal(part[1], whole[1][7:17, 13:33])


def test_capi_and_header_agree_on_the_layout():
    text = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    m = re.search(r"typedef struct gs_noise \{(.*?)\} gs_noise;", text, re.S)
    assert m, "gs_noise is not in the header"
    ctype = {"float": ctypes.c_float, "uint64_t": ctypes.c_uint64}
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(n.strip(), ctype[typ]) for n in names.split(",")]
    assert fields == list(capi.GsNoise._fields_), fields
    assert ctypes.sizeof(capi.GsNoise) == 24
    assert [getattr(capi.GsNoise, n).offset for n, _ in fields] == [0, 4, 8, 16]
    for sym in ("gs_ctx_set_noise", "gs_ctx_get_noise"):
        assert sym in capi.EXPORTS and re.search(r"int32_t %s\(" % sym, text), sym
