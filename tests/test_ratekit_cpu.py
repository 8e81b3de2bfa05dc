"""tools/ratekit.py without a GPU: the measuring protocol it states (order and number of the calls, which clock brackets
which), its parsing and its files, driven with a context whose timer returns scripted values and with Simulation / Species
stand-ins that record what is done to them."""
from __future__ import annotations

import json
import os
import sys

import pytest

from tests.children import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

import ratekit  # noqa: E402


class FakeContext:
    def __init__(self, log, ms=()):
        self.log, self.ms, self.closed = log, list(ms), False

    def timer_start(self):
        self.log.append("timer_start")

    def timer_stop(self):
        self.log.append("timer_stop")
        return self.ms.pop(0)

    def close(self):
        self.closed = True
        self.log.append("close")


class FakePlane:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def destroy(self):
        self.log.append(f"destroy {self.name}")


class FakeSubject:
    """A Species (in_out) or an ensemble (destroy)."""

    def __init__(self, log):
        self.log = log
        self.planes = [FakePlane(log, n) for n in ("in_u", "in_v", "out_u", "out_v")]

    def in_out(self):
        return tuple(self.planes)

    def destroy(self):
        self.log.append("destroy ensemble")


class FakeSimulation:
    def __init__(self, log, params, hip):
        self.log, self.params, self.hip, self.context = log, params, hip, FakeContext(log)

    def make_species(self, shape):
        self.log.append(f"make_species {tuple(shape)}")
        return FakeSubject(self.log)

    def make_ensemble(self, shape, params, members=None):
        self.log.append(f"make_ensemble {tuple(shape)} {params} {members}")
        return FakeSubject(self.log)


@pytest.fixture
def fake_simulation(monkeypatch):
    log, made = [], []

    def make(params, hip):
        made.append(FakeSimulation(log, params, hip))
        return made[-1]

    monkeypatch.setattr(ratekit, "_simulation", make)
    return log, made


def _calls(log, names="abc"):
    return [x for x in log if x in tuple(names)]


@pytest.mark.parametrize("warm", [True, False])
def test_medians_round_robin_with_one_warm_up_each(warm):
    log = []
    # the timer's values in the order they are handed out: a, b, c of round 1, then of rounds 2 and 3
    ctx = FakeContext(log, [5.0, 1.0, 9.0, 3.0, 2.0, 7.0, 4.0, 6.0, 8.0])
    fns = {name: (lambda name=name: log.append(name)) for name in "abc"}
    got = ratekit.medians(ctx, fns, 3, warm=warm)
    assert got == {"a": 4.0, "b": 2.0, "c": 8.0}
    assert list(got) == ["a", "b", "c"]
    timed = ["timer_start", "a", "timer_stop", "timer_start", "b", "timer_stop", "timer_start", "c", "timer_stop"] * 3
    assert log == (["a", "b", "c"] if warm else []) + timed       # one warm-up call each, untimed, before the first timed one
    assert _calls(log).count("a") == 3 + warm


def test_medians_of_both_clocks(monkeypatch):
    log = []
    clock = iter([0.0, 0.002, 1.0, 1.004, 2.0, 2.006])
    monkeypatch.setattr(ratekit.time, "perf_counter", lambda: next(clock))
    ctx = FakeContext(log, [0.5, 0.7, 0.9])
    got = ratekit.medians(ctx, {"a": lambda: log.append("a")}, 3, warm=False, both=True)
    assert got["a"] == (pytest.approx(4.0), 0.7)                    # (wall ms, device ms)


def test_both_clocks_have_the_device_timer_outside(monkeypatch):
    log = []
    ticks = iter([10.0, 10.25])

    def perf_counter():
        log.append("clock")
        return next(ticks)

    monkeypatch.setattr(ratekit.time, "perf_counter", perf_counter)
    ctx = FakeContext(log, [1.5])
    assert ratekit.both_ms(ctx, lambda: log.append("call")) == (250.0, 1.5)
    assert log == ["timer_start", "clock", "call", "clock", "timer_stop"]
    log.clear()
    ctx.ms = [2.5]
    assert ratekit.device_ms(ctx, lambda: log.append("call")) == 2.5
    assert log == ["timer_start", "call", "timer_stop"]


def test_parse_grids():
    assert ratekit.parse_grids("96x160,64x128x2", slabs=True) == [(96, 160, 1), (64, 128, 2)]
    assert ratekit.parse_grids("16384x16384,4096x4096,1080x1920") == [(16384, 16384), (4096, 4096), (1080, 1920)]
    assert ratekit.parse_grids("") == [] and ratekit.parse_grids("96x160,") == [(96, 160)]
    for bad, slabs in (("96", True), ("96x", True), ("96xab", True), ("96x160x2x2", True), ("96x160x2", False), ("0x160", True),
                       ("96-160", False)):
        with pytest.raises(ValueError) as e:
            ratekit.parse_grids("64x64," + bad, slabs=slabs)
        assert type(e.value) is ValueError and bad in str(e.value)


def test_report_writes_a_json_list(tmp_path, capsys):
    path, md = tmp_path / "sub" / "dir" / "rows.json", tmp_path / "table.md"
    report = ratekit.Report(str(path), str(md))
    report.row({"grid": "96x160", "ms": 1.5})
    assert json.loads(path.read_text()) == [{"grid": "96x160", "ms": 1.5}]      # what a run that is cut short leaves
    report.row({"grid": "64x128", "ms": 2.5})
    report.rows[0]["derived"] = 3.0
    report.table("| grid | ms |", "|---|---|")
    report.table("| 96x160 | 1.500 |")
    report.finish()
    assert json.loads(path.read_text()) == [{"grid": "96x160", "ms": 1.5, "derived": 3.0}, {"grid": "64x128", "ms": 2.5}]
    assert md.read_text() == "| grid | ms |\n|---|---|\n| 96x160 | 1.500 |\n"
    out = capsys.readouterr().out.splitlines()
    assert [json.loads(x) for x in out[:2]] == [{"grid": "96x160", "ms": 1.5}, {"grid": "64x128", "ms": 2.5}]
    assert out[2:] == ["| grid | ms |", "|---|---|", "| 96x160 | 1.500 |"]


def test_report_appends_json_lines(tmp_path, capsys):
    path, md = tmp_path / "sub" / "rows.jsonl", tmp_path / "table.md"
    path.parent.mkdir()
    path.write_text('{"earlier": 1}\n')
    report = ratekit.Report(str(path), str(md), json_lines=True)
    report.table("| grid | rate |", "|---|---|")
    report.table("| 96 x 160 | 12 |")
    report.row({"rows": 96, "rate": 12.0})
    report.row({"rows": 64, "rate": 7.0})
    report.finish()
    assert [json.loads(x) for x in path.read_text().splitlines()] == [{"earlier": 1}, {"rows": 96, "rate": 12.0},
                                                                       {"rows": 64, "rate": 7.0}]
    assert md.read_text() == "| grid | rate |\n|---|---|\n| 96 x 160 | 12 |\n"
    assert capsys.readouterr().out.splitlines() == ["| grid | rate |", "|---|---|", "| 96 x 160 | 12 |"]   # no JSON on stdout
    ratekit.Report(str(tmp_path / "new" / "rows.jsonl"), None, json_lines=True).row({"a": 1})             # the directory is made
    assert (tmp_path / "new" / "rows.jsonl").read_text() == '{"a": 1}\n'
    ratekit.Report(None, None, json_lines=True).row({"a": 1})                                              # no file asked for


def test_species_subject_tears_down_when_the_body_raises(fake_simulation):
    log, made = fake_simulation
    with pytest.raises(KeyError):
        with ratekit.species_subject(96, 160, boundary=3, devices=[0, 0]) as (sim, ctx, species):
            assert sim is made[0] and ctx is sim.context and not ctx.closed
            assert sim.hip == {"boundary": 3, "devices": [0, 0]} and sim.params is None
            raise KeyError("in the body")
    assert log == ["make_species (96, 160)", "destroy in_u", "destroy in_v", "destroy out_u", "destroy out_v", "close"]
    assert made[0].context.closed


def test_ensemble_subject_tears_down_when_the_body_raises(fake_simulation):
    log, made = fake_simulation
    with pytest.raises(KeyError):
        with ratekit.ensemble_subject(2, 64, 128, ["p0", "p1"], boundary=2) as (sim, ctx, ens):
            assert sim.params == "p0" and sim.hip == {"boundary": 2}
            raise KeyError("in the body")
    assert log == ["make_ensemble (64, 128) ['p0', 'p1'] None", "destroy ensemble", "close"]
    assert made[0].context.closed


def test_subjects_tear_down_after_a_clean_body_and_when_the_subject_cannot_be_made(fake_simulation, monkeypatch):
    log, made = fake_simulation
    with ratekit.species_subject(8, 8):
        pass
    assert log[-1] == "close" and log.count("destroy in_u") == 1
    monkeypatch.setattr(FakeSimulation, "make_species", lambda self, shape: 1 / 0)
    with pytest.raises(ZeroDivisionError):
        with ratekit.species_subject(8, 8):
            raise AssertionError("the body must not run")
    assert made[1].context.closed


def test_timed_steps_sets_the_boundary_rule_only_when_told(built, monkeypatch):
    seen = []

    def subject(rows, cols, **hip):
        seen.append(hip)
        raise KeyError("far enough")

    monkeypatch.setattr(ratekit, "species_subject", subject)
    for kw in ({}, {"boundary": 3, "slabs": 2}):
        with pytest.raises(KeyError):
            ratekit.timed_steps(96, 160, 16, 2, **kw)
    assert seen == [{"kernel": 0, "devices": [0]}, {"kernel": 0, "devices": [0, 0], "boundary": 3}]   # else: GS_HIP_BOUNDARY


def test_entry_of_reproduces_the_mapping_of_the_two_tools():
    # the names in the docstrings of entry_of in param_map_rate.py and mask_rate.py as they were, and their neighbours
    assert ratekit.entry_of("tb-k4c2/strict.op/map", "map") == "gs_step_tb_mk_strict<4, 3, 2, 0>"
    assert ratekit.entry_of("tb-k4c2/strict.op/mask", "mask") == "gs_step_tb_wk_strict<4, 3, 2, 0>"
    assert ratekit.entry_of("tb-k4c2/strict.op/map@r8w4", "map") == "gs_step_tb_mk_strict<4, 3, 2, 0>"
    assert ratekit.entry_of("tb-k2/fused/periodic/map", "map") == "gs_step_tb_mk_fused<2, 0, 4, 1>"
    assert ratekit.entry_of("tb-k4c1/strict.op/neumann/mask", "mask") == "gs_step_tb_wk_strict<4, 3, 1, 2>"
    assert ratekit.RULE_SET == {"/periodic": 1, "/neumann": 2}
    for name, form in (("stream/strict/map", "map"), ("tile16x64/strict.op/mask", "mask"), ("tb-k4c2/strict.op", "map"),
                       ("tb-k4c2/strict.op/map", "mask"), ("window/strict", "mask")):
        assert ratekit.entry_of(name, form) is None


def test_registers_of_a_reported_kernel():
    class K:
        vgpr = 84

    kernels = {"gs_step_tb_mk_strict<4, 3, 2, 0>": K}
    assert ratekit.registers(kernels, "tb-k4c2/strict.op/map@r8w4", "map") == ("gs_step_tb_mk_strict<4, 3, 2, 0>", 84, 5)
    assert ratekit.registers(kernels, "stream/strict/map", "map") == (None, None, None)
    assert ratekit.registers({}, "tb-k4c2/strict.op/map", "map") == ("gs_step_tb_mk_strict<4, 3, 2, 0>", None, None)


def test_rules_in_turn_adds_the_marching_kernel_where_auto_runs_another():
    asked = []

    def time_rule(rule, pin):
        asked.append((rule, pin))
        return {"kernel": "window/strict" if (rule, pin) == (0, 0) else "tb-k4c2/strict.op", "rate": 100.0 if pin == 0 else 50.0}

    got = [(label, over) for label, _, over in ratekit.rules_in_turn([("clipped", 0), ("periodic", 2)], time_rule)]
    assert asked == [(0, 0), (0, 3), (2, 0)]
    assert got == [("clipped", 1.0), ("clipped, kernel = TB", 0.5), ("periodic", 1.0)]
