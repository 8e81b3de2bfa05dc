"""tests.helpers.rule_run and rule_of without a GPU: one reference per boundary rule, each the existing reference of that
rule, and the rule read back from a reported kernel name."""
from __future__ import annotations

import pytest

import oracle
from grayscott_amd import Parameters, capi

from . import neumann_ref, periodic_ref
from .helpers import oracle_params, rule_of, rule_run, stress_fields

SHAPES = [(1, 1), (1, 6), (5, 1), (3, 4), (9, 13)]
P = Parameters(weights=((0.25, 0.5, 0.125), (0.5, 0.0, 1.0), (0.0, 0.5, 0.25)), feed_rate=0.03, kill_rate=0.06,
               time_step=0.5, diffusion_rate_u=0.2)


@pytest.mark.parametrize("params", [None, P], ids=["default", "skew"])
@pytest.mark.parametrize("shape", SHAPES)
def test_rule_run_is_each_rules_reference(shape, params):
    u0, v0 = stress_fields(shape, 17)
    q = oracle_params(params) if params else None
    refs = {capi.GS_BOUNDARY_CLIPPED: lambda: oracle.run(u0, v0, 5, params=q, ftz=True, boundary=oracle.CLIPPED),
            capi.GS_BOUNDARY_ZERO_HALO: lambda: oracle.run(u0, v0, 5, params=q, ftz=True, boundary=oracle.ZERO_HALO),
            capi.GS_BOUNDARY_PERIODIC: lambda: periodic_ref.run(u0, v0, 5, params=q),
            capi.GS_BOUNDARY_NEUMANN: lambda: neumann_ref.run(u0, v0, 5, params=q)}
    got = {}
    for rule, ref in refs.items():
        gu, gv = rule_run(u0, v0, 5, q, rule)
        ru, rv = ref()
        assert gu.tobytes() == ru.tobytes() and gv.tobytes() == rv.tobytes(), (shape, rule)
        got[rule] = gu.tobytes() + gv.tobytes()
    if shape[0] * shape[1] > 1:  # (a 1 x 1 grid is its own neighbourhood under the periodic and zero-flux rules)
        assert len(set(got.values())) == 4, f"two rules agree on {shape}: the dispatch is wrong"
    assert rule_run(u0, v0, 0, q, capi.GS_BOUNDARY_PERIODIC)[0].tobytes() == u0.tobytes()
    with pytest.raises(ValueError):
        rule_run(u0, v0, 1, q, 4)


def test_rule_of_reads_the_name():
    assert rule_of("tb-k4c2/strict.op.dx") == capi.GS_BOUNDARY_CLIPPED
    assert rule_of("tile32x64/fused/periodic") == capi.GS_BOUNDARY_PERIODIC
    assert rule_of("tb-k3c1/strict.op/periodic@r12") == capi.GS_BOUNDARY_PERIODIC
    assert rule_of("ensemble-resident/strict.op/neumann") == capi.GS_BOUNDARY_NEUMANN
    assert rule_of("tb-k4c4f/fused/neumann@tail") == capi.GS_BOUNDARY_NEUMANN
    assert rule_of("resident-lds/strict@periodic") == capi.GS_BOUNDARY_CLIPPED  # (only what precedes "@" counts)
