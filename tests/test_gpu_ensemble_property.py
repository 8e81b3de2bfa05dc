"""Ensembles under every boundary rule and both arithmetic flavours, against tests.helpers.rule_run member by member.

* Randomised: hypothesis draws the rule, the flavour, member counts on both sides of the CU count, member shapes whose
  cells straddle the resident form's limits (1024, 1536, 2048, 4096 and 8192 cells, and thin members that cross its LDS
  limit), per-member parameters and the split of the steps into calls.  The form (resident or windowed), the .op
  specialisation and the rule are asserted from the reported name against restatements of the library's own choices.
* A deterministic sweep of the resident form's launch table (rule x .op x cells per thread: 30 entries in the strict
  build, 15 in the fused one), each entry reached by the smallest member count and shape that selects it.
* The resident form's launch split above 2^21 workgroups, with every member checked.

Strict math is bit-exact; so is fused math here, whose draws hold no sub-normal values."""
from __future__ import annotations

import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

from grayscott_amd import HipArgs, Parameters, Simulation, capi

from .helpers import assert_bits_equal, oracle_params, rule_of, rule_run, stress_fields

pytestmark = pytest.mark.gpu

RULES = [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_PERIODIC, capi.GS_BOUNDARY_NEUMANN]
MATHS = [capi.GS_MATH_STRICT, capi.GS_MATH_FUSED]
RESIDENT_CELLS = 1536  # kGsResidentCells (gs_kernels.h)
ENS_MAX_GROUPS = 1 << 21  # kGsEnsMaxGroups (gs_kernels.h)


def cu_count():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def resident_cpt(rows, cols, boundary):
    """gs_ens_resident_cpt (gs_kernels.h): cells per thread of the resident form, 0 = not resident.  Four planes of
    (rows + 2) x (cols + 2) floats within 160 KiB of LDS; 1, 2, 4 or 8 cells per thread of a 1024-thread workgroup, 8
    not under the clipped rule."""
    cells = rows * cols
    if 16 * (rows + 2) * (cols + 2) > 160 * 1024:
        return 0
    need = -(-cells // 1024)
    return 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8 if need <= 8 and boundary != capi.GS_BOUNDARY_CLIPPED else 0


def is_resident(rows, cols, boundary, members, cus):
    """gs_ensemble_run: the resident form while a member fits it, above 1536 cells only when the members fill the chip."""
    return resident_cpt(rows, cols, boundary) > 0 and (rows * cols <= RESIDENT_CELLS or members >= cus)


def fast_of_all(params, math):
    """fast_of_all (gs_ensemble.cpp): the .op kernels only in strict math, when every member has side weights 0.5 and
    dt == 1 (compared in f32, as the library does)."""
    if math != capi.GS_MATH_STRICT:
        return False
    f = np.float32
    return all(all(f(p.weights[i][j]) == f(0.5) for i, j in ((0, 1), (1, 0), (1, 2), (2, 1))) and f(p.time_step) == f(1.0)
               for p in params)


def run_ensemble(params, u0, v0, calls, boundary, math):
    sim = Simulation.new(params[0], HipArgs(devices=[0], boundary=boundary, math=math))
    ens = sim.make_ensemble(u0.shape[1:], params, seed=False)
    try:
        ens.upload(u0, v0)
        for n in calls:
            ens.prepare_steps(n)
        u, v = ens.u_views(), ens.result_views()
        name = sim.context.info()[0]
    finally:
        ens.destroy()
        sim.context.close()
    return u, v, name


def member_fields(members, shape, seed):
    rng = np.random.default_rng(seed)
    u = rng.random((members,) + tuple(shape), dtype=np.float32)
    v = (rng.random((members,) + tuple(shape), dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    return u, v


def check_members(which, params, u0, v0, steps, boundary, u, v, name):
    for i in which:
        ref_u, ref_v = rule_run(u0[i], v0[i], steps, oracle_params(params[i]), boundary)
        assert_bits_equal(u[i], ref_u, f"U of member {i} ({name}, {params[i]})")
        assert_bits_equal(v[i], ref_v, f"V of member {i} ({name}, {params[i]})")


def check_name(name, rows, cols, members, boundary, math, params, cus):
    resident = is_resident(rows, cols, boundary, members, cus)
    assert name.startswith("ensemble-resident/" if resident else "ensemble-tile"), (name, rows, cols, members, cus)
    variant = name.split("@")[0].split("/")[1]
    assert variant.startswith("fused" if math == capi.GS_MATH_FUSED else "strict"), name
    assert variant.endswith(".op") == fast_of_all(params, math), (name, params)
    assert rule_of(name) == (boundary if boundary >= capi.GS_BOUNDARY_PERIODIC else capi.GS_BOUNDARY_CLIPPED), (name, boundary)


# ---- randomised --------------------------------------------------------------------------------------------------------
def _shapes():
    """Members whose cells are the resident form's limits and their neighbours (the squarest factorisation, both ways
    round), and 1 x N / N x 1 members on both sides of its LDS limit (16 (1 + 2) (N + 2) <= 160 KiB: N <= 3411)."""
    out = set()
    for limit in (1024, RESIDENT_CELLS, 2048, 4096, 8192):
        for cells in (limit - 1, limit, limit + 1):
            r = max(d for d in range(1, int(cells ** 0.5) + 1) if cells % d == 0)
            out |= {(r, cells // r), (cells // r, r)}
    for n in (1023, 1025, 2049, 3411, 3412, 4097):
        out |= {(1, n), (n, 1)}
    return sorted(out)


SHAPES = _shapes()
WEIGHTS = [0.0, 0.125, 0.25, 0.5]   # powers of two (fused math), at most 4 in all: the explicit step stays stable at dt = 2


@st.composite
def parameter_sets(draw, all_op):
    w = [[draw(st.sampled_from(WEIGHTS)) for _ in range(3)] for _ in range(3)]
    if all_op or draw(st.booleans()):
        w[0][1] = w[1][0] = w[1][2] = w[2][1] = 0.5
    return Parameters(weights=tuple(tuple(r) for r in w),
                      diffusion_rate_u=draw(st.sampled_from([0.05, 0.1])),
                      diffusion_rate_v=draw(st.sampled_from([0.025, 0.05])),
                      feed_rate=draw(st.sampled_from([0.0, 0.014, 0.03, 0.055])),
                      kill_rate=draw(st.sampled_from([0.045, 0.054, 0.062])),
                      time_step=1.0 if all_op else draw(st.sampled_from([0.25, 0.5, 1.0, 2.0])))


@st.composite
def ensemble_cases(draw):
    boundary = draw(st.sampled_from(RULES))
    math = draw(st.sampled_from(MATHS))
    shape = draw(st.sampled_from(SHAPES + [(8, 16), (1, 5), (37, 53)]))
    many = draw(st.booleans())
    members = draw(st.integers(0, 4)) if many else draw(st.integers(1, 9))   # many: CUs + 0 ... 4
    all_op = draw(st.booleans())
    sets = draw(st.lists(parameter_sets(all_op), min_size=1, max_size=4))
    calls = draw(st.lists(st.integers(0, 9), min_size=1, max_size=4))
    if sum(calls) == 0:
        calls.append(1)
    seed = draw(st.integers(0, 2 ** 16))
    return boundary, math, shape, many, members, sets, calls, seed


@settings(max_examples=int(os.environ.get("GS_ENSEMBLE_PROPERTY_EXAMPLES", "200")), deadline=None,
          suppress_health_check=list(HealthCheck))
@given(ensemble_cases())
def test_ensembles_match_each_rules_reference(built, case):
    boundary, math, shape, many, members, sets, calls, seed = case
    cus = cu_count()
    members = cus + members if many else members
    rng = np.random.default_rng(seed)
    params = [sets[int(k)] for k in rng.integers(0, len(sets), members)]
    u0, v0 = member_fields(members, shape, seed)
    u, v, name = run_ensemble(params, u0, v0, calls, boundary, math)
    check_name(name, shape[0], shape[1], members, boundary, math, params, cus)
    which = sorted({0, members - 1} | {int(i) for i in rng.integers(0, members, 3)})
    check_members(which, params, u0, v0, sum(calls), boundary, u, v, name)


# ---- the resident form's launch table, entry by entry -------------------------------------------------------------------
# The smallest shape per cells per thread (1: 8 x 16; 2: 25 x 41 = 1025 cells; 4: 33 x 63 = 2079; 8: 65 x 64 = 4160, within
# the LDS limit); above 1536 cells the members must fill the chip.
CPT_SHAPES = {1: (8, 16), 2: (25, 41), 4: (33, 63), 8: (65, 64)}
TABLE = [(math, boundary, op, cpt) for math in MATHS for boundary in RULES for op in ((0, 1) if math == capi.GS_MATH_STRICT else (0,))
         for cpt in (1, 2, 4, 8) if cpt < 8 or boundary != capi.GS_BOUNDARY_CLIPPED]
assert sum(m == capi.GS_MATH_STRICT for m, *_ in TABLE) == 30 and sum(m == capi.GS_MATH_FUSED for m, *_ in TABLE) == 15


def _table_id(entry):
    math, boundary, op, cpt = entry
    return f"{'fused' if math else 'strict'}-rule{boundary}-{'op' if op else 'general'}-cpt{cpt}"


@pytest.mark.parametrize("entry", TABLE, ids=_table_id)
def test_resident_launch_table(built, entry):
    math, boundary, op, cpt = entry
    shape = CPT_SHAPES[cpt]
    assert resident_cpt(*shape, boundary) == cpt
    cus = cu_count()
    members = 3 if shape[0] * shape[1] <= RESIDENT_CELLS else cus
    if op:
        params = [Parameters(feed_rate=0.01 + 0.04 * i / members, kill_rate=0.05 + 0.01 * (i % 3)) for i in range(members)]
    else:  # one member with dt != 1 is enough to leave the .op form
        params = [Parameters(feed_rate=0.01 + 0.04 * i / members, time_step=0.5 if i == members // 2 else 1.0,
                             diffusion_rate_u=0.2 if i % 2 else 0.1) for i in range(members)]
    u0, v0 = member_fields(members, shape, 1000 + cpt)
    calls = (4, 0, 7)
    u, v, name = run_ensemble(params, u0, v0, calls, boundary, math)
    check_name(name, shape[0], shape[1], members, boundary, math, params, cus)
    assert name.startswith("ensemble-resident/"), name
    check_members((0, members // 2, members - 1), params, u0, v0, sum(calls), boundary, u, v, name)


# ---- the resident form's launch split ----------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_PERIODIC])
def test_resident_launch_split(built, boundary):
    """2^21 + 5 members of one cell: two launches, the second from member 2^21.  Each member starts from one of 64 states,
    those past the split from other states than members 0 ... 4; every member is checked against its state's result."""
    members, steps = ENS_MAX_GROUPS + 5, (3, 4)
    pool_u, pool_v = stress_fields((64, 1), 77)
    rng = np.random.default_rng(5)
    pick = rng.integers(0, 64, members)
    pick[ENS_MAX_GROUPS:] = (pick[:5] + 1 + np.arange(5)) % 64
    p = Parameters(feed_rate=0.03, kill_rate=0.06)
    ref = [rule_run(pool_u[k:k + 1], pool_v[k:k + 1], sum(steps), oracle_params(p), boundary) for k in range(64)]
    ref_u = np.array([r[0][0, 0] for r in ref], np.float32)
    ref_v = np.array([r[1][0, 0] for r in ref], np.float32)
    assert not np.array_equal(ref_u, pool_u[:, 0]), "the pool must change under the steps"
    sim = Simulation.new(p, HipArgs(devices=[0], boundary=boundary))
    ens = sim.make_ensemble((1, 1), p, members=members, seed=False)
    try:
        ens.upload(pool_u[pick, 0].reshape(members, 1, 1), pool_v[pick, 0].reshape(members, 1, 1))
        for n in steps:
            ens.prepare_steps(n)
        u, v = ens.u_views().reshape(members), ens.result_views().reshape(members)
        name = sim.context.info()[0]
    finally:
        ens.destroy()
        sim.context.close()
    assert name.startswith("ensemble-resident/") and name.split("/")[1].endswith(".op"), name
    assert rule_of(name) == (boundary if boundary == capi.GS_BOUNDARY_PERIODIC else capi.GS_BOUNDARY_CLIPPED), name
    for plane, got, want in (("U", u, ref_u[pick]), ("V", v, ref_v[pick])):
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (f"{plane}: {bad.size} of {members} members differ ({name}); first {bad[:5].tolist()}, "
                               f"{int((bad >= ENS_MAX_GROUPS).sum())} past the split")
