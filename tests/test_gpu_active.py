"""Active sets of ensembles on the MI355X: retired members stop advancing and keep their bits through any number and parity
of runs, for every reader; the members that run stay bit for bit what a lone Species is after their own step count -- under
all four boundary rules, in both kernel forms (resident, windowed) and both math flavours; writes into retired members
hold; the sweep's --steady-retire against the rule restated on the CPU oracle."""
from __future__ import annotations

import ctypes
import json
import os
import sys

import numpy as np
import pytest

import oracle
from grayscott_amd import HipArgs, Parameters, Simulation, capi, hdf5_min

from .helpers import assert_bits_equal, gpu_run, oracle_params, rule_run
from .test_gpu_ensemble import PARAMS, member_fields
from tests.children import ROOT, build_program, run_program

pytestmark = pytest.mark.gpu
RULES = [capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO, capi.GS_BOUNDARY_PERIODIC, capi.GS_BOUNDARY_NEUMANN]
SHAPES = [(8, 16),     # resident, one cell per thread
          (13, 21),    # resident, ragged (273 cells: the last wave partly idle); cells % 4 != 0: the mirror's dword path
          (37, 53),    # 1961 cells: windowed with these few members (resident once they fill the chip); the dword path
          (100, 300)]  # windowed, several windows per member


def make(params, shape, boundary=capi.GS_BOUNDARY_CLIPPED, math=capi.GS_MATH_STRICT, seed=1, fields=True):
    sim = Simulation.new(params[0], HipArgs(devices=[0], boundary=boundary, math=math))
    ens = sim.make_ensemble(shape, params, seed=not fields)
    u0 = v0 = None
    if fields:
        u0, v0 = member_fields(len(params), shape, seed=seed)
        ens.upload(u0, v0)
    return sim, ens, u0, v0


def close(sim, *ensembles):
    for e in ensembles:
        e.destroy()
    sim.context.close()


def lone(u0, v0, steps, p, boundary, math):
    """What a lone Species with parameters ``p`` is after ``steps`` steps: the CPU references in strict math (the C oracle
    where it has the rule, tests/periodic_ref.py and tests/neumann_ref.py else), gs_run in fused math."""
    if math == capi.GS_MATH_STRICT:
        return rule_run(u0, v0, steps, params=oracle_params(p), boundary=boundary)
    ru, rv, _ = gpu_run(u0, v0, steps, p, HipArgs(devices=[0], boundary=boundary, math=math))
    return ru, rv


def assert_members_are_lone_runs(ens, members, params, u0, v0, counts, boundary, math, what):
    u, v = ens.u_views(), ens.result_views()
    for i in members:
        ru, rv = lone(u0[i], v0[i], int(counts[i]), params[i], boundary, math)
        assert_bits_equal(u[i], ru, f"U of member {i} after {counts[i]} steps ({what})")
        assert_bits_equal(v[i], rv, f"V of member {i} after {counts[i]} steps ({what})")


# (shape, rule, math, the member retired before the third run)
SCHEDULE_CASES = [(s, b, capi.GS_MATH_STRICT, 0) for s in SHAPES for b in RULES] + \
                 [((37, 53), capi.GS_BOUNDARY_CLIPPED, capi.GS_MATH_FUSED, 0), ((100, 300), capi.GS_BOUNDARY_PERIODIC, capi.GS_MATH_FUSED, 0),
                  ((8, 16), capi.GS_BOUNDARY_ZERO_HALO, capi.GS_MATH_STRICT, 4), ((100, 300), capi.GS_BOUNDARY_CLIPPED, capi.GS_MATH_STRICT, 4)]


@pytest.mark.parametrize("shape,boundary,math,late", SCHEDULE_CASES)
def test_schedule_against_lone_runs(shape, boundary, math, late):
    """Calls of odd and even length around the changes of the active set: a retired member left in the wrong slot, or one
    that took a step too many, fails here.  Schedule: run 7; retire {1, 3}; run 9; retire {late}, reactivate {3}; run 4; run 5.
    (The issue that asked for this test names member 0 as the late one and the counts 25, 7, 25, 16, 16, which are those of
    member 4 as the late one: a retired first entry and a retired last entry of the list are both run.)"""
    params = PARAMS[:5]
    sim, ens, u0, v0 = make(params, shape, boundary, math)
    names = []

    def run(n):
        ens.perform_steps(n)
        names.append(sim.context.info()[0])

    assert ens.active().tolist() == [True] * 5 and ens.active_count() == 5 and ens.steps_taken().tolist() == [0] * 5
    run(7)
    ens.retire([1, 3])
    assert ens.active().tolist() == [True, False, True, False, True] and ens.active_count() == 3
    run(9)
    assert ens.steps_taken().tolist() == [16, 7, 16, 7, 16]
    ens.retire([late])
    ens.reactivate([3])
    assert ens.active().tolist() == [i not in (1, late) for i in range(5)] and ens.active_count() == 3
    run(4)
    run(5)
    counts = [16 if i == late else c for i, c in enumerate([25, 7, 25, 16, 25])]
    assert ens.steps_taken().tolist() == counts and ens.steps_taken().dtype == np.int64
    assert ens.active().dtype == np.bool_
    assert "/listed" not in names[0] and all(n.endswith("/listed") for n in names[1:]), names
    assert_members_are_lone_runs(ens, range(5), params, u0, v0, counts, boundary, math, names[-1])
    close(sim, ens)


@pytest.mark.parametrize("shape", [(8, 16), (100, 300)])
def test_every_reader_sees_the_held_state(shape):
    params = PARAMS[:5]
    sim, ens, _, _ = make(params, shape)
    ens.perform_steps(6)
    ens.retire([1, 4])
    held = [1, 4]

    def read():
        fresh = sim.make_ensemble(shape, Parameters(), seed=False, members=5)
        fresh.copy_from(ens)
        out = {"v": ens.result_views(), "u": ens.u_views(), "summaries": ens.summaries(), "histograms": ens.histograms(bins=64),
               "copy_u": fresh.u_views(), "copy_v": fresh.result_views()}
        fresh.destroy()
        return out

    before, snap = read(), ens.snapshot()
    for n in (3, 1, 5):  # three runs of odd length: the newest slot changes sides every time
        ens.perform_steps(n)
        assert sim.context.info()[0].endswith("/listed")
        after = read()
        for key, was in before.items():
            for i in held:
                assert after[key][i].tobytes() == was[i].tobytes(), (key, i, n)
            if key in ("u", "v", "copy_u", "copy_v"):
                assert after[key][0].tobytes() != was[0].tobytes(), (key, n)  # (the others do move)
        changes = ens.changes_since(snap)
        for i in held:
            for s in (0, 1):
                c = changes[i, s]
                assert c["differing"] == 0 and c["nonfinite"] == 0, (i, s, n)
                assert c["max_abs"] == 0.0 and c["sum_abs"] == 0.0 and c["sum_sq"] == 0.0, (i, s, n)
        assert changes[0, 0]["differing"] > 0
        # a subset read that starts at a retired member
        assert_bits_equal(ens.result_views(4, 1)[0], before["v"][4], f"V of member 4 read alone after run({n})")
    close(sim, ens, snap)


@pytest.mark.parametrize("shape", [(8, 16), (37, 53), (100, 300)])
def test_writes_into_retired_members(shape):
    params = PARAMS[:4]
    sim, ens, u0, v0 = make(params, shape)
    wu, wv = member_fields(2, shape, seed=77)
    ens.perform_steps(2)
    ens.retire([1, 2])
    ens.perform_steps(1)
    # upload into a retired member, then runs: the uploaded bits
    ens.upload(wu[:1], wv[:1], first=1)
    ens.perform_steps(3)
    assert_bits_equal(ens.u_views(1, 1)[0], wu[0], "U uploaded into retired member 1, after run(3)")
    assert_bits_equal(ens.result_views(1, 1)[0], wv[0], "V uploaded into retired member 1, after run(3)")
    ens.perform_steps(2)
    assert_bits_equal(ens.result_views(1, 1)[0], wv[0], "V uploaded into retired member 1, after run(3); run(2)")
    # copy_from into a retired member, then one step: the copied bits
    src = sim.make_ensemble(shape, Parameters(), seed=False, members=4)
    src.upload(np.stack([wu[1]] * 4), np.stack([wv[1]] * 4))
    ens.copy_from(src, 2, 1)
    ens.perform_steps(1)
    assert_bits_equal(ens.u_views(2, 1)[0], wu[1], "U copied into retired member 2, after run(1)")
    assert_bits_equal(ens.result_views(2, 1)[0], wv[1], "V copied into retired member 2, after run(1)")
    assert_bits_equal(ens.result_views(1, 1)[0], wv[0], "V of retired member 1 beside it")
    assert ens.steps_taken().tolist() == [9, 2, 2, 9]
    assert_members_are_lone_runs(ens, [0, 3], params, u0, v0, [9, 2, 2, 9], capi.GS_BOUNDARY_CLIPPED, capi.GS_MATH_STRICT, "active")
    # a reactivated member goes on from what was written into it
    ens.reactivate([1])
    ens.perform_steps(3)
    ru, rv = lone(wu[0], wv[0], 3, params[1], capi.GS_BOUNDARY_CLIPPED, capi.GS_MATH_STRICT)
    assert_bits_equal(ens.result_views(1, 1)[0], rv, "V of member 1, reactivated, 3 steps after the upload")
    assert_bits_equal(ens.u_views(1, 1)[0], ru, "U of member 1, reactivated, 3 steps after the upload")
    assert ens.steps_taken().tolist() == [12, 5, 2, 12]
    close(sim, ens, src)


@pytest.mark.parametrize("shape", [(8, 16), (100, 300)])
def test_seed_with_retired_members(shape):
    params = PARAMS[:4]
    sim, ens, _, _ = make(params, shape)
    ens.perform_steps(3)
    ens.retire([0, 2])
    ens.seed()
    ens.perform_steps(3)
    su, sv = oracle.init_species(*shape)
    u, v = ens.u_views(), ens.result_views()
    for i in (0, 2):
        assert_bits_equal(u[i], su, f"U of retired member {i}: Species::new's pattern")
        assert_bits_equal(v[i], sv, f"V of retired member {i}: Species::new's pattern")
    for i in (1, 3):
        ru, rv = oracle.run(su, sv, 3, params=oracle_params(params[i]), ftz=True)
        assert_bits_equal(u[i], ru, f"U of active member {i}: the pattern advanced")
        assert_bits_equal(v[i], rv, f"V of active member {i}: the pattern advanced")
    close(sim, ens)


def test_many_members():
    """300 members that fill the chip, 60 of them retired: the 240 that run may run in another form than the 300 did."""
    n, shape, boundary = 300, (64, 64), capi.GS_BOUNDARY_ZERO_HALO
    rng = np.random.default_rng(11)
    params = [Parameters(feed_rate=float(f), kill_rate=float(k)) for f, k in zip(rng.uniform(0.01, 0.05, n), rng.uniform(0.045, 0.065, n))]
    sim, ens, u0, v0 = make(params, shape, boundary, seed=5)
    ens.perform_steps(5)
    first = sim.context.info()[0]
    retired = np.arange(2, n, 5)  # 60 of them, spread over the range
    assert len(retired) == 60
    ens.retire(retired)
    ens.perform_steps(11)
    second = sim.context.info()[0]
    print(f"300 active: {first}; 240 active: {second}")
    assert ens.active_count() == 240
    counts = np.full(n, 16)
    counts[retired] = 5
    assert ens.steps_taken().tolist() == counts.tolist()
    assert_members_are_lone_runs(ens, [2, 147, 297, 0, 148, 299], params, u0, v0, counts, boundary, capi.GS_MATH_STRICT,
                                 f"{first} then {second}")
    close(sim, ens)


@pytest.mark.parametrize("shape", [(8, 16), (100, 300)])
def test_edges(shape):
    params = PARAMS[:5]
    sim, ens, u0, v0 = make(params, shape)
    plain = sim.make_ensemble(shape, params, seed=False)  # never touched by set_active
    plain.upload(u0, v0)
    ens.perform_steps(3)
    # all retired: the run returns, launches nothing and changes nothing
    ens.set_active(np.zeros(5, np.bool_))
    assert ens.active_count() == 0
    u, v = ens.u_views(), ens.result_views()
    name, launches = sim.context.info()
    for k in (1, 4, 7):
        ens.perform_steps(k)
    assert tuple(sim.context.info()) == (name, launches)
    assert_bits_equal(ens.u_views().reshape(-1, shape[1]), u.reshape(-1, shape[1]), "U with every member retired")
    assert_bits_equal(ens.result_views().reshape(-1, shape[1]), v.reshape(-1, shape[1]), "V with every member retired")
    assert ens.steps_taken().tolist() == [3] * 5
    # a sub-range changes only that range (uint8 flags, first > 0); a proper subset runs the listed forms
    ens.set_active(np.array([1, 0, 1], np.uint8), first=1)
    assert ens.active().tolist() == [False, True, False, True, False]
    ens.perform_steps(2)
    listed_name = sim.context.info()[0]
    assert listed_name.startswith("ensemble-") and listed_name.endswith("/listed"), listed_name
    assert ens.steps_taken().tolist() == [3, 5, 3, 5, 3]
    # all reactivated: the kernels and the states of an ensemble that never had an active set
    ens.set_active(np.ones(5, np.uint8))
    ens.retire([])
    assert ens.active().all() and ens.active_count() == 5
    plain.perform_steps(3)
    plain.perform_steps(4)
    plain_name = sim.context.info()[0]
    ens.perform_steps(4)
    assert sim.context.info()[0] == plain_name and "/listed" not in plain_name
    counts = [7, 9, 7, 9, 7]
    assert ens.steps_taken().tolist() == counts
    assert_members_are_lone_runs(ens, range(5), params, u0, v0, counts, capi.GS_BOUNDARY_CLIPPED, capi.GS_MATH_STRICT, "reactivated")
    assert plain.steps_taken().tolist() == [7] * 5 and plain.active().all()
    for i in (0, 2, 4):
        assert_bits_equal(ens.result_views(i, 1)[0], plain.result_views(i, 1)[0], f"V of member {i} against the plain ensemble")
        assert_bits_equal(ens.u_views(i, 1)[0], plain.u_views(i, 1)[0], f"U of member {i} against the plain ensemble")
    # a snapshot is all active, its counts start at 0
    ens.retire([2])
    snap = ens.snapshot()
    assert snap.active().all() and snap.steps_taken().tolist() == [0] * 5
    close(sim, ens, plain, snap)


def test_refusals():
    sim, ens, _, _ = make(PARAMS[:3], (8, 16))
    lib, flags = sim.context._lib, (ctypes.c_uint8 * 4)(1, 1, 1, 1)
    steps, total = (ctypes.c_uint64 * 4)(), ctypes.c_uint64()
    INV = capi.GS_ERR_INVALID
    for first, count in ((0, 4), (3, 1), (1, 3), (0, 0)):  # outside the ensemble (or empty)
        assert lib.gs_members_set_active(sim.context.handle, ens.handle, first, count, flags) == INV
        assert lib.gs_members_get_active(sim.context.handle, ens.handle, first, count, flags, steps, ctypes.byref(total)) == INV
    assert lib.gs_members_set_active(sim.context.handle, ens.handle, 0, 3, None) == INV
    assert lib.gs_members_get_active(sim.context.handle, ens.handle, 0, 3, None, None, None) == INV
    assert lib.gs_members_get_active(sim.context.handle, ens.handle, 0, 3, None, None, ctypes.byref(total)) == capi.GS_OK
    assert total.value == 3
    # the Python side checks a mask's length and type before the call
    for bad in (np.ones(4, np.bool_), np.ones(0, np.bool_), np.ones((3, 1), np.bool_)):
        with pytest.raises(ValueError):
            ens.set_active(bad)
    with pytest.raises(ValueError):
        ens.set_active(np.ones(2, np.bool_), first=2)
    with pytest.raises(TypeError):
        ens.set_active(np.ones(3, np.float32))
    with pytest.raises(IndexError):
        ens.retire([3])
    # a foreign context
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    assert lib.gs_members_set_active(other.context.handle, ens.handle, 0, 3, flags) == INV
    assert lib.gs_members_get_active(other.context.handle, ens.handle, 0, 3, flags, None, None) == INV
    assert ens.active().all() and ens.active_count() == 3  # nothing was changed by any of them
    other.context.close()
    close(sim, ens)


def test_cpp_mirror(tmp_path):
    exe, out = build_program("active_mirror", tmp_path), tmp_path / "o.bin"
    members, rows, cols, steps = 4, 8, 16, 5
    r = run_program([str(exe), str(members), str(rows), str(cols), str(steps), str(out)])
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    cells = members * rows * cols
    v = np.frombuffer(raw, np.float32, cells).reshape(members, rows, cols)
    taken = np.frombuffer(raw, np.uint64, members, 4 * cells)
    flags = np.frombuffer(raw, np.uint8, members, 4 * cells + 8 * members)
    assert flags.tolist() == [1, 0, 1, 0] and taken.tolist() == [3 * steps + 2, steps, 3 * steps + 2, steps]
    su, sv = oracle.init_species(rows, cols)
    for i in range(members):
        _, rv = oracle.run(su, sv, int(taken[i]), params=oracle_params(Parameters()), ftz=True)
        assert_bits_equal(v[i], rv, f"V of member {i} through the C++ mirror")


SWEEP = ["--feed", "0.02:0.04:2", "--kill", "0.06:0.07:2", "-r", "40", "-c", "64", "-s", "600", "--steady-every", "50",
         "--steady-tol", "4e-4"]


def run_sweep(out, extra):
    r = run_program([sys.executable, "-m", "grayscott_amd.sweep"] + SWEEP + extra + ["-o", str(out)], cwd=ROOT, limit=300)
    assert r.returncode == 0, r.stderr


@pytest.fixture(scope="module")
def oracle_rule():
    """The rule of --steady-retire restated per member on the CPU oracle: advance 50 steps, take the largest |change| in f64
    for U and V, stop at the first sample at which both are at most T.  -> {(feed, kill): (steps_taken, settled_step, V)}"""
    rows, cols, steps, every, tol = 40, 64, 600, 50, 4e-4
    out = {}
    for kill in (0.06, 0.07):
        for feed in (0.02, 0.04):
            p = oracle_params(Parameters(feed_rate=feed, kill_rate=kill))
            u, v = oracle.init_species(rows, cols)
            at, settled = 0, -1
            while at < steps:
                nu, nv = oracle.run(u, v, every, params=p, ftz=True)
                at += every
                du = float(np.max(np.abs(nu.astype(np.float64) - u.astype(np.float64))))
                dv = float(np.max(np.abs(nv.astype(np.float64) - v.astype(np.float64))))
                u, v = nu, nv
                print(f"F = {feed}, k = {kill}: step {at}: max |dU| = {du:.3e}, max |dV| = {dv:.3e}")
                if du <= tol and dv <= tol:
                    settled = at
                    break
            out[(feed, kill)] = (at, settled, v)
    return out


def test_sweep_retires_settled_members(tmp_path, oracle_rule):
    out = tmp_path / "retire.h5"
    run_sweep(out, ["--steady-retire"])
    side = json.load(open(tmp_path / "retire.json"))
    npz = np.load(tmp_path / "retire.steady.npz")
    images = hdf5_min.read(str(out))
    assert images.shape == (4, 40, 64) and len(side["members"]) == 4
    taken = [m["steps_taken"] for m in side["members"]]
    # the inputs do what the test is about: a member retires before the end and one is active to the end
    assert min(taken) < 600 and max(taken) == 600, taken
    assert side["steps"] == max(taken)
    for m in side["members"]:
        want_taken, want_settled, want_v = oracle_rule[(m["feed"], m["kill"])]
        i = m["index"]
        assert (m["steps_taken"], m["settled_step"]) == (want_taken, want_settled), m
        assert (int(npz["steps_taken"][i]), int(npz["settled_step"][i])) == (want_taken, want_settled), m
        assert_bits_equal(images[i], want_v, f"image {i} (F = {m['feed']}, k = {m['kill']}) after {want_taken} steps")
        # a retired member equals its snapshot from then on: its later records are zeros
        later = npz["steps"] > want_taken
        assert not npz["max_abs"][i][later].any() and not npz["differing"][i][later].any(), m
    assert oracle_rule[(0.02, 0.07)][0] == 400 and oracle_rule[(0.04, 0.06)][1] == -1


def test_sweep_without_the_flag_writes_what_it_wrote(tmp_path, oracle_rule):
    """Without --steady-retire: no new key, no new field, and every member at step 600 -- the files of the sweep as it was
    (its records and images are held to the oracle by tests/test_gpu_change.py and tests/test_gpu_ensemble.py)."""
    a, b = tmp_path / "a" / "run.h5", tmp_path / "b" / "run.h5"
    os.makedirs(a.parent)
    os.makedirs(b.parent)
    run_sweep(a, [])
    run_sweep(b, [])
    for name in ("run.h5", "run.json", "run.steady.npz"):
        assert open(a.parent / name, "rb").read() == open(b.parent / name, "rb").read(), name
    side = json.load(open(a.parent / "run.json"))
    assert side["steps"] == 600 and all("steps_taken" not in m and set(m) == {"index", "feed", "kill", "settled_step"} for m in side["members"])
    npz = np.load(a.parent / "run.steady.npz")
    assert set(npz.files) == {"steps", "settled_step", "max_abs", "sum_abs", "sum_sq", "differing", "nonfinite"}
    images = hdf5_min.read(str(a))
    for m in side["members"]:
        want_taken, want_settled, want_v = oracle_rule[(m["feed"], m["kill"])]
        assert m["settled_step"] == want_settled, m
        if want_taken == 600:  # (a member the rule never stops: the same image with and without the flag)
            assert_bits_equal(images[m["index"]], want_v, f"image {m['index']} without the flag")
