"""The measuring kit of the ``tools/*_rate.py`` tools: what they share, stated once.

Two families use it.  The observable tools (summary, change, histogram, morphology, correlation, components, component_list)
time blocking calls on a Species or an ensemble that read its planes; the step-rule tools (periodic, neumann, param_map, mask)
time ``prepare_steps`` calls and prove the planes they leave against a replay with the single-step cross-check kernel.

* clocks: ``device_ms`` (device events on the context's compute stream), ``wall_ms`` (host clock), ``both_ms``, and
  ``medians`` -- the named calls in turn, round-robin, so that all of them see the same chip state;
* inputs: ``fill`` brings a fresh Species into the state ``new`` / ``developed`` / ``random``;
* subjects: ``species_subject`` and ``ensemble_subject`` build a Simulation with its Species or ensemble and tear it down;
* ``timed_steps`` (timed steps with their proof), ``rules_in_turn``, ``ensemble_against_sequential``, ``entry_of`` /
  ``registers``;
* reporting: ``parse_grids``, ``Report`` and ``observable_args``, the command line the observable tools share.

The modules that need the GPU are imported where they are used, so the kit itself loads without one.
"""
from __future__ import annotations

import contextlib
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GRIDS = "16384x16384,4096x4096,1080x1920"  # the Species grids of the observable tools
ENSEMBLE = (512, 64, 128)  # members, rows, cols
KINDS = ("new", "developed", "random")


# --- clocks

def device_ms(ctx, fn):
    """Milliseconds between device events on the context's compute stream around one blocking call."""
    ctx.timer_start()
    fn()
    return ctx.timer_stop()


def wall_ms(fn):
    """Host milliseconds of one blocking call."""
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def both_ms(ctx, fn):
    """(wall ms, device-event ms) of one blocking call: the device timer brackets the host clock."""
    ctx.timer_start()
    wall = wall_ms(fn)
    return wall, ctx.timer_stop()


def medians(ctx, fns, calls, warm=True, both=False):
    """{name: median device ms} of the calls ``fns`` ({name: fn}), timed in turn (round-robin, in the dict's order) ``calls``
    times each, after one warm-up call each unless the caller has made them (``warm=False``).  ``both``: every value is
    (median wall ms, median device ms) of the same calls."""
    if warm:
        for fn in fns.values():
            fn()
    got = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            got[k].append(both_ms(ctx, fn) if both else device_ms(ctx, fn))
    if both:
        return {k: (statistics.median(w for w, _ in v), statistics.median(e for _, e in v)) for k, v in got.items()}
    return {k: statistics.median(v) for k, v in got.items()}


# --- inputs

def fill(sim, species, kind):
    """Bring ``species`` (fresh from make_species) into the state ``kind``: ``new`` leaves it, ``random`` uploads U uniform
    in [0, 1) and V = U / 2, ``developed`` runs 64 steps from there."""
    import numpy as np

    if kind == "new":
        return
    rng = np.random.default_rng(3)
    in_u, in_v, _, _ = species.in_out()
    u = rng.random(tuple(species.shape()), dtype=np.float32)
    in_u.upload(sim.context, u)
    u *= np.float32(0.5)
    in_v.upload(sim.context, u)
    if kind == "developed":
        sim.perform_steps(species, 64)


# --- subjects

def _simulation(params, hip):
    from grayscott_amd import HipArgs, Parameters, Simulation

    return Simulation.new(Parameters() if params is None else params, HipArgs(**{"devices": [0], **hip}))


@contextlib.contextmanager
def species_subject(rows, cols, **hip):
    """(sim, ctx, species) of a fresh Species of rows x cols on a context of its own; ``hip``: HipArgs fields (``boundary``,
    ``kernel``, ``devices``).  On the way out the planes are destroyed and the context is closed."""
    sim = _simulation(None, hip)
    species = None
    try:
        species = sim.make_species((rows, cols))
        yield sim, sim.context, species
    finally:
        for plane in species.in_out() if species is not None else ():
            plane.destroy()
        sim.context.close()


@contextlib.contextmanager
def ensemble_subject(members, rows, cols, params=None, **hip):
    """(sim, ctx, ens) of an ensemble of ``members`` grids of rows x cols: default parameters, or ``params`` (one Parameters
    per member; the context gets the first).  On the way out the ensemble is destroyed and the context is closed."""
    sim = _simulation(None if params is None else params[0], hip)
    ens = None
    try:
        if params is None:
            from grayscott_amd import Parameters

            ens = sim.make_ensemble((rows, cols), Parameters(), members=members)
        else:
            ens = sim.make_ensemble((rows, cols), params)
        yield sim, sim.context, ens
    finally:
        if ens is not None:
            ens.destroy()
        sim.context.close()


# --- timed steps with proof

def _planes(ctx, species):
    in_u, in_v, _, _ = species.in_out()
    return in_u.make_scalar_view(ctx), in_v.make_scalar_view(ctx)


def timed_steps(rows, cols, steps, calls, *, boundary=None, kernel=0, slabs=1, attach=None, prove=True):
    """``calls`` calls of ``steps`` steps on a Species seeded with Species::new's pattern, timed with device events around each
    call, after warm-up calls until the on-line tuner has settled on the marching kernel's configuration (gs_ctx_info names a
    tuned one; at most 40).  ``attach(sim)`` sets what the context carries (a parameter map, a mask) before the first step.
    ``prove``: a second context of the same rule, slabs and attachment replays the same number of steps from the same initial
    state with the single-step cross-check kernel (GS_KERNEL_SIMPLE, one gs_step per step); ``proof`` says whether U and V
    are bit for bit the same."""
    import numpy as np

    from grayscott_amd import capi

    hip = {"devices": [0] * slabs}
    if boundary is not None:  # (left to HipArgs otherwise: GS_HIP_BOUNDARY, or the clipped rule)
        hip["boundary"] = boundary
    with species_subject(rows, cols, kernel=kernel, **hip) as (sim, ctx, species):
        if attach:
            attach(sim)
        warm = 0
        while True:
            sim.perform_steps(species, steps)
            warm += 1
            name = ctx.info()[0]
            if warm >= 40 or not name.startswith("tb-") or "@" in name:
                break
        times = [device_ms(ctx, lambda: sim.prepare_steps(species, steps)) for _ in range(calls)]
        ctx.sync()
        ms = statistics.median(times)
        out = {"rows": rows, "cols": cols, "steps_per_call": steps, "calls": calls, "warmup_calls": warm,
               "kernel": ctx.info()[0], "ms": ms, "ms_all": times, "rate": rows * cols * steps / (ms * 1e3)}
        if prove:
            got_u, got_v = _planes(ctx, species)
    if not prove:
        return out
    total = steps * (calls + warm)
    with species_subject(rows, cols, kernel=capi.GS_KERNEL_SIMPLE, **hip) as (ref, rctx, rs):
        if attach:
            attach(ref)
        for _ in range(total):
            ref.perform_step(rs)
        ref_u, ref_v = _planes(rctx, rs)
        out.update(replay_kernel=rctx.info()[0], replay_steps=total,
                   proof=bool(got_u.tobytes() == ref_u.tobytes() and got_v.tobytes() == ref_v.tobytes()),
                   sum_v=float(np.sum(got_v, dtype=np.float64)))
    return out


def rules_in_turn(rules, time_rule):
    """(label, record, rate / the clipped rule's rate) of ``time_rule(boundary, pinned kernel)`` for every (label, boundary)
    of ``rules``, the clipped rule first.  Where kernel = AUTO runs another kernel than the marching one for the clipped
    rule, the clipped rule's marching kernel (kernel = TB) is timed right after it."""
    todo = [(label, rule, 0) for label, rule in rules]
    base = None
    while todo:
        label, rule, pin = todo.pop(0)
        r = time_rule(rule, pin)
        if rule == 0 and pin == 0:
            base = r["rate"]
            if not r["kernel"].startswith("tb-"):
                todo.insert(0, ("clipped, kernel = TB", 0, 3))
        yield label, r, r["rate"] / base


def ensemble_against_sequential(members, rows, cols, steps, calls, sample, boundary):
    """An ensemble of ``members`` grids (ensemble_rate.member_params) under ``boundary`` against ``sample`` of the same
    members run one after another through gs_run on the same context, with a bit-check of one member."""
    import numpy as np

    from ensemble_rate import member_params

    params = member_params(members)
    with ensemble_subject(members, rows, cols, params, boundary=boundary) as (sim, ctx, ens):
        ens.perform_steps(steps)
        times = [device_ms(ctx, lambda: ens.prepare_steps(steps)) for _ in range(calls)]
        ctx.sync()
        kernel = ctx.info()[0]
        idx = sorted({int(round(i * (members - 1) / max(1, sample - 1))) for i in range(sample)})
        solo = [sim.make_species((rows, cols)) for _ in idx]
        try:
            def members_in_turn():
                for j, i in enumerate(idx):
                    ctx.set_params(params[i])
                    sim.prepare_steps(solo[j], steps)

            seq, solo_kernel = [], None
            for call in range(calls + 1):  # the first call of every member is its warm-up
                ms = device_ms(ctx, members_in_turn)
                if call:
                    seq.append(ms)
                solo_kernel = ctx.info()[0]
            ctx.sync()
            j = len(idx) // 2
            got, ref = ens.result_views(idx[j], 1)[0], solo[j].make_result_view()
        finally:
            for s in solo:
                for plane in s.in_out():
                    plane.destroy()
    out = {"members": members, "rows": rows, "cols": cols, "kernel": kernel, "sequential_kernel": solo_kernel,
           "ensemble_rate": members * rows * cols * steps / (statistics.median(times) * 1e3),
           "sequential_rate": rows * cols * steps / (statistics.median(seq) / len(idx) * 1e3),
           "bitcheck_member": idx[j], "bitcheck": bool(got.tobytes() == ref.tobytes()),
           "bitcheck_max_abs_diff": float(np.max(np.abs(got.astype(np.float64) - ref)))}
    out["speedup"] = out["ensemble_rate"] / out["sequential_rate"]
    return out


RULE_SET = {"/periodic": 1, "/neumann": 2}
FORMS = {"map": "mk", "mask": "wk", "noise": "zk"}  # the attachment in a reported kernel name -> the infix of the entry's name


def entry_of(name, form):
    """The kernel instance behind a reported name of the marching kernel's ``form`` ("map" or "mask"), e.g.
    tb-k4c2/strict.op/map@.. -> gs_step_tb_mk_strict<4, 3, 2, 0>; None for a name that is not the marching kernel's."""
    m = re.match(r"tb-k(\d)(c\d)?/(strict|fused)(\.op)?(/periodic|/neumann)?/" + form, name)
    if not m:
        return None
    k, c, flavour, op, rule = m.groups()
    cpl = int(c[1:]) if c else 4
    return f"gs_step_tb_{FORMS[form]}_{flavour}<{k}, {3 if op else 0}, {cpl}, {RULE_SET.get(rule, 0)}>"


def registers(kernels, name, form):
    """(entry, VGPRs, waves per SIMD they allow) of the reported kernel ``name``; ``kernels``: {name: tools/codeobj.py entry}."""
    entry = entry_of(name.split("@")[0], form)
    k = kernels.get(entry) if entry else None
    vgpr = k.vgpr if k else None
    return entry, vgpr, min(8, 512 // (((vgpr + 7) // 8) * 8)) if vgpr else None


# --- reporting

def parse_grids(text, slabs=False):
    """[(rows, cols)] of a comma-separated list of ROWSxCOLS; with ``slabs`` [(rows, cols, slabs)] of ROWSxCOLS or
    ROWSxCOLSxSLABS.  Empty items are skipped; anything else that is malformed is a ValueError."""
    grids = []
    for item in filter(None, text.split(",")):
        try:
            g = tuple(int(x) for x in item.split("x"))
        except ValueError:
            g = ()
        if len(g) not in ((2, 3) if slabs else (2,)) or min(g) < 1:
            raise ValueError(f"not a grid (ROWSxCOLS{'[xSLABS]' if slabs else ''}): {item!r}")
        grids.append((g + (1,))[:3] if slabs else g)
    return grids


class Report:
    """The records and the markdown table of one run.  ``row`` keeps a record, ``table`` adds and prints markdown lines,
    ``finish`` writes the files.  The records go to ``json_path`` in one of two conventions: a JSON list, written anew after
    every row and again by ``finish`` (a run that is cut short leaves what it measured), the rows printed as they come; or,
    with ``json_lines``, one line per record appended to the file."""

    def __init__(self, json_path=None, md_path=None, json_lines=False):
        self.json_path, self.md_path, self.json_lines = json_path, md_path, json_lines
        self.rows, self.lines = [], []
        if json_path:
            os.makedirs(os.path.dirname(os.path.abspath(json_path)), exist_ok=True)

    def _write_list(self):
        if self.json_path and not self.json_lines:
            with open(self.json_path, "w") as f:
                json.dump(self.rows, f, indent=1)

    def row(self, rec):
        self.rows.append(rec)
        if not self.json_lines:
            print(json.dumps(rec), flush=True)
            self._write_list()
        elif self.json_path:
            with open(self.json_path, "a") as f:
                f.write(json.dumps(rec) + "\n")
        return rec

    def table(self, *lines):
        self.lines += lines
        print("\n".join(lines), flush=True)

    def finish(self):
        self._write_list()
        if self.md_path:
            with open(self.md_path, "w") as f:
                f.write("\n".join(self.lines) + "\n")


def observable_args(doc, argv, calls, add=None):
    """The parsed command line of an observable tool: --calls, --grids, --no-ensemble, --json, --md and what ``add(parser)``
    adds of the tool's own; then the ``import torch`` that these tools start from."""
    import argparse

    ap = argparse.ArgumentParser(description=doc.split("\n")[0])
    ap.add_argument("--calls", type=int, default=calls)
    if add:
        add(ap)
    ap.add_argument("--grids", default=GRIDS)
    ap.add_argument("--no-ensemble", action="store_true")
    ap.add_argument("--json", default=None, help="also write the rows as a JSON list")
    ap.add_argument("--md", default=None, help="also write the table as markdown")
    args = ap.parse_args(argv)
    import torch  # noqa: F401  (the process's HIP runtime is torch's, as in bench.py and the tests)

    return args
