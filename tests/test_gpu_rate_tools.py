"""The eleven rate tools on tools/ratekit.py, each run once at the smallest arguments that go through every branch of the kit,
against what the tools printed at the same arguments before they were rewritten on the kit.

EXPECTED was recorded on an MI355X from the tools as they stood before the rewrite (summary_rate.py and change_rate.py with
nothing but their --grids flag added), run twice.  Per tool it holds the first two markdown lines, and per JSON row

* the fields that were the same in both runs, compared by value: kernel names, ``warmup_calls``, ``replay_steps``, ``sum_v``,
  counts, fractions, the kernel entry and its registers;
* the name of the row's list under ``timed``: the keys of that row whose values differed between the two runs somewhere in
  the tool's output -- times, and rates and ratios computed from times.  Their values are left out of the comparison; the
  keys are not: the set of keys of every row must be exactly the recorded fields plus the row's timed keys.

``largest_fraction`` of components_rate.py's ``developed`` row is 0 / 0 = NaN in both runs and is compared as NaN.

The recorded values describe the library as much as the tools: ``vgpr`` and ``waves_per_simd`` are the compiler's register
allocation, ``warmup_calls`` and the kernel names are the tuner's schedule and choice at these sizes.  When a kernel, the
compiler or the tuner changes them, record them anew from the tools; that is not a regression of the tools.

Every tool runs in a fresh process of its own, one after another; after an abort, a segmentation fault or a timeout no further
tool is started."""
from __future__ import annotations

import math

import pytest

from tests.children import run_rate_tool

pytestmark = pytest.mark.gpu
NAN = float("nan")

OBSERVABLE = ["--grids", "96x160", "--calls", "2"]
STEP_RULE = ["--steps", "16", "--calls", "2"]
ARGS = {"summary": OBSERVABLE, "change": OBSERVABLE, "histogram": OBSERVABLE, "morphology": OBSERVABLE, "correlation": OBSERVABLE,
        "components": OBSERVABLE + ["--label-calls", "0"], "component_list": OBSERVABLE,
        "periodic": ["--grids", "96x160", "--sample", "4"] + STEP_RULE, "neumann": ["--grids", "96x160", "--sample", "4"] + STEP_RULE,
        "param_map": ["--grids", "96x160,96x160x2"] + STEP_RULE, "mask": ["--grids", "96x160,96x160x2"] + STEP_RULE}

EXPECTED = {
    'summary': {
        'header': [('| grid | summary, device (ms) | summary, host call (ms) | plane reads (TB/s) | single step (ms) | ke'
                    'rnel of the step | summary / step |'),
                   '|---|---|---|---|---|---|---|'],
        'timed': {
            'grid': ['summary_device_ms', 'summary_host_ms', 'step_ms', 'read_tb_per_s', 'summary_over_step'],
        },
        'rows': [
            ('grid', {'grid': '96x160', 'cells': 15360, 'step_kernel': 'stream-g2/strict'}),
            ('grid', {'grid': '512 x 64x128', 'cells': 4194304, 'step_kernel': 'ensemble-tile32x64/strict.op'}),
        ]},
    'change': {
        'header': [('| grid | change_since, device (ms) | host call (ms) | plane reads (TB/s) | summary, device (ms) | ho'
                    'st call (ms) | plane reads (TB/s) | read rate, change / summary | snapshot() (ms) | update (ms) | up'
                    'date, read + write (TB/s) |'),
                   '|---|---|---|---|---|---|---|---|---|---|---|'],
        'timed': {
            'grid': ['change_device_ms', 'change_host_ms', 'summary_device_ms', 'summary_host_ms', 'update_ms',
             'snapshot_ms', 'first_snapshot_ms', 'change_read_tb_per_s', 'summary_read_tb_per_s', 'read_rate_ratio',
             'copy_tb_per_s'],
        },
        'rows': [
            ('grid', {'grid': '96x160', 'cells': 15360}),
            ('grid', {'grid': '512 x 64x128', 'cells': 4194304}),
        ]},
    'histogram': {
        'header': [('| grid | input | bins | histogram (ms) | summary (ms) | histogram / summary | plane reads (TB/s) | /'
                    ' random input |'),
                   '|---|---|---|---|---|---|---|---|'],
        'timed': {
            'grid': ['histogram_ms', 'summary_ms', 'histogram_over_summary', 'read_tb_per_s', 'over_random'],
        },
        'rows': [
            ('grid', {'grid': '96x160', 'input': 'new', 'cells': 15360, 'bins': 256, 'filled_bins_u': 2, 'filled_bins_v': 1,
             'largest_share_u': 0.99609375}),
            ('grid', {'grid': '96x160', 'input': 'developed', 'cells': 15360, 'bins': 256, 'filled_bins_u': 22,
             'filled_bins_v': 14, 'largest_share_u': 0.251171875}),
            ('grid', {'grid': '96x160', 'input': 'random', 'cells': 15360, 'bins': 256, 'filled_bins_u': 256,
             'filled_bins_v': 256, 'largest_share_u': 0.005403645833333333}),
            ('grid', {'grid': '512 x 64x128', 'input': 'new + 16 steps', 'cells': 4194304, 'bins': 256}),
        ]},
    'morphology': {
        'header': [('| grid | input | nt = 1 (ms) | nt = 4 (ms) | summary (ms) | nt = 1 / summary | nt = 4 / summary | pl'
                    'ane reads, nt = 1 (TB/s) |'),
                   '|---|---|---|---|---|---|---|---|'],
        'timed': {
            'grid': ['nt1_ms', 'nt4_ms', 'summary_ms', 'nt1_over_summary', 'nt4_over_summary', 'nt1_read_tb_per_s'],
        },
        'rows': [
            ('grid', {'grid': '96x160', 'input': 'new', 'cells': 15360, 'v_area_fraction': 0.00390625, 'v_euler8': 1}),
            ('grid', {'grid': '96x160', 'input': 'developed', 'cells': 15360, 'v_area_fraction': 0.0, 'v_euler8': 0}),
            ('grid', {'grid': '96x160', 'input': 'random', 'cells': 15360, 'v_area_fraction': 0.4998046875,
             'v_euler8': -841}),
            ('grid', {'grid': '512 x 64x128', 'input': 'new + 16 steps', 'cells': 4194304}),
        ]},
    'correlation': {
        'header': [('| grid | input | L = 16 (ms) | L = 32 (ms) | L = 64 (ms) | nt = 4, L = 32 (ms) | summary (ms) | morp'
                    'hology (ms) | L = 32 / summary | L = 32 / morphology | L = 64 / morphology | plane reads, L = 32 (TB'
                    '/s) |'),
                   '|---|---|---|---|---|---|---|---|---|---|---|---|'],
        'timed': {
            'grid': ['l16_ms', 'l32_ms', 'l64_ms', 'nt4_l32_ms', 'summary_ms', 'morphology_ms', 'l32_over_summary',
             'l32_over_morphology', 'l64_over_morphology', 'l32_read_tb_per_s'],
        },
        'rows': [
            ('grid', {'grid': '96x160', 'input': 'new', 'cells': 15360, 'v_fraction': 0.00390625,
             'v_first_minimum_rows': 10}),
            ('grid', {'grid': '96x160', 'input': 'developed', 'cells': 15360, 'v_fraction': 0.0,
             'v_first_minimum_rows': None}),
            ('grid', {'grid': '96x160', 'input': 'random', 'cells': 15360, 'v_fraction': 0.4998046875,
             'v_first_minimum_rows': 1}),
            ('grid', {'grid': '512 x 64x128', 'input': 'new + 16 steps', 'cells': 4194304}),
        ]},
    'components': {
        'header': [('| grid | input | components | components, 8 (ms) | components, 4 (ms) | morphology (ms) | 8 / morpho'
                    'logy | download + label (ms) | label / components |'),
                   '|---|---|---|---|---|---|---|---|---|'],
        'timed': {
            'grid': ['components8_ms', 'components4_ms', 'morphology_ms', 'components8_event_ms', 'components4_event_ms',
             'morphology_event_ms', 'components8_over_morphology'],
        },
        'rows': [
            ('grid', {'grid': '96x160', 'input': 'new', 'cells': 15360, 'components': 1, 'largest_fraction': 1.0,
             'label_memory_bytes': 122880, 'download_label_ms': None, 'label_over_components8': None}),
            ('grid', {'grid': '96x160', 'input': 'developed', 'cells': 15360, 'components': 0, 'largest_fraction': NAN,
             'label_memory_bytes': 122880, 'download_label_ms': None, 'label_over_components8': None}),
            ('grid', {'grid': '96x160', 'input': 'random', 'cells': 15360, 'components': 16,
             'largest_fraction': 0.9965760989617849, 'label_memory_bytes': 122880, 'download_label_ms': None,
             'label_over_components8': None}),
            ('grid', {'grid': '512 x 64x128', 'input': 'new + 16 steps, U and V', 'cells': 8388608, 'components': None,
             'largest_fraction': None, 'label_memory_bytes': 33554432, 'download_label_ms': None,
             'label_over_components8': None}),
        ]},
    'component_list': {
        'header': [('| grid | input | records | largest (cells) | list (ms) | list, min_size 5 (ms) | components (ms) | l'
                    'ist / components | download + label + measure (ms) | host / list |'),
                   '|---|---|---|---|---|---|---|---|---|---|'],
        'timed': {
            'grid': ['list_ms', 'list_min5_ms', 'components_ms', 'list_event_ms', 'list_min5_event_ms',
             'components_event_ms', 'download_label_ms'],
        },
        'rows': [
            ('grid', {'grid': '96x160', 'input': 'new', 'cells': 15360, 'records': 1, 'largest': 60}),
            ('grid', {'grid': '96x160', 'input': 'developed', 'cells': 15360, 'records': 52, 'largest': 19}),
            ('grid', {'grid': '96x160', 'input': 'full', 'cells': 15360, 'records': 1, 'largest': 15360}),
            ('grid', {'grid': '96x160', 'input': 'random', 'cells': 15360, 'records': 16, 'largest': 9023}),
            ('grid', {'grid': '512 x 64x128', 'input': 'new + 16 steps, V (components: U and V)', 'cells': 4194304,
             'records': 512, 'largest': 56}),
        ]},
    'periodic': {
        'header': ['| grid | rule | kernel | Mcells x steps / s | / clipped | replay (simple kernel) |',
                   '|---|---|---|---|---|---|'],
        'timed': {
            'grid': ['ms', 'ms_all', 'rate'],
            'ensemble': ['ensemble_rate', 'sequential_rate', 'speedup'],
        },
        'rows': [
            ('grid', {'rows': 96, 'cols': 160, 'boundary': 0, 'steps_per_call': 16, 'calls': 2, 'warmup_calls': 1,
             'kernel': 'tile16x64/strict.op', 'replay_kernel': 'simple/strict', 'replay_steps': 48, 'proof': True,
             'sum_v': 55.84440504425566}),
            ('grid', {'rows': 96, 'cols': 160, 'boundary': 0, 'steps_per_call': 16, 'calls': 2, 'warmup_calls': 40,
             'kernel': 'tb-k4c1/strict.op', 'replay_kernel': 'simple/strict', 'replay_steps': 672, 'proof': True,
             'sum_v': 101.75749078345555}),
            ('grid', {'rows': 96, 'cols': 160, 'boundary': 1, 'steps_per_call': 16, 'calls': 2, 'warmup_calls': 1,
             'kernel': 'tile16x64/strict.op', 'replay_kernel': 'simple/strict', 'replay_steps': 48, 'proof': True,
             'sum_v': 55.84440504425566}),
            ('grid', {'rows': 96, 'cols': 160, 'boundary': 2, 'steps_per_call': 16, 'calls': 2, 'warmup_calls': 1,
             'kernel': 'tile16x64/strict.op/periodic', 'replay_kernel': 'simple/strict/periodic', 'replay_steps': 48,
             'proof': True, 'sum_v': 55.84440504425566}),
            ('ensemble', {'members': 512, 'rows': 64, 'cols': 128, 'kernel': 'ensemble-resident/strict.op/periodic',
             'sequential_kernel': 'tile16x64/strict.op/periodic', 'bitcheck_member': 341, 'bitcheck': True,
             'bitcheck_max_abs_diff': 0.0}),
        ]},
    'neumann': {
        'header': ['| grid | rule | kernel | Mcells x steps / s | / clipped | replay (simple kernel) |',
                   '|---|---|---|---|---|---|'],
        'timed': {
            'grid': ['ms', 'ms_all', 'rate'],
            'ensemble': ['ensemble_rate', 'sequential_rate', 'speedup'],
        },
        'rows': [
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 1, 'boundary': 0, 'steps_per_call': 16, 'calls': 2,
             'warmup_calls': 1, 'kernel': 'tile16x64/strict.op', 'replay_kernel': 'simple/strict', 'replay_steps': 48,
             'proof': True, 'sum_v': 55.84440504425566}),
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 1, 'boundary': 0, 'steps_per_call': 16, 'calls': 2,
             'warmup_calls': 40, 'kernel': 'tb-k4c1/strict.op', 'replay_kernel': 'simple/strict', 'replay_steps': 672,
             'proof': True, 'sum_v': 101.75749078345555}),
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 1, 'boundary': 3, 'steps_per_call': 16, 'calls': 2,
             'warmup_calls': 1, 'kernel': 'tile16x64/strict.op/neumann', 'replay_kernel': 'simple/strict/neumann',
             'replay_steps': 48, 'proof': True, 'sum_v': 55.84440504425566}),
            ('ensemble', {'members': 512, 'rows': 64, 'cols': 128, 'boundary': 0, 'kernel': 'ensemble-tile32x64/strict.op',
             'sequential_kernel': 'tile16x64/strict.op', 'bitcheck_member': 341, 'bitcheck': True}),
            ('ensemble', {'members': 512, 'rows': 64, 'cols': 128, 'boundary': 3,
             'kernel': 'ensemble-resident/strict.op/neumann', 'sequential_kernel': 'tile16x64/strict.op/neumann',
             'bitcheck_member': 341, 'bitcheck': True}),
        ]},
    'param_map': {
        'header': [('| grid | uniform: kernel | Mcells x steps / s | mapped: kernel | Mcells x steps / s | mapped / unifo'
                    'rm | mapped streaming kernel | marching / streaming | VGPRs | waves per SIMD | replay (mapped simple'
                    ' kernel) |'),
                   '|---|---|---|---|---|---|---|---|---|---|---|'],
        'timed': {
            'grid': ['ms', 'ms_all', 'rate'],
        },
        'rows': [
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 1, 'mapped': False, 'pinned_kernel': 0, 'steps_per_call': 16,
             'calls': 2, 'warmup_calls': 1, 'kernel': 'tile16x64/strict.op', 'entry': 'gs_step_tb_mk_strict<4, 3, 1, 0>',
             'vgpr': 95, 'waves_per_simd': 5}),
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 1, 'mapped': True, 'pinned_kernel': 0, 'steps_per_call': 16,
             'calls': 2, 'warmup_calls': 40, 'kernel': 'tb-k4c1/strict.op/map', 'replay_kernel': 'simple/strict/map',
             'replay_steps': 672, 'proof': True, 'sum_v': 337.59180533252476, 'entry': 'gs_step_tb_mk_strict<4, 3, 1, 0>',
             'vgpr': 95, 'waves_per_simd': 5}),
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 1, 'mapped': True, 'pinned_kernel': 2, 'steps_per_call': 16,
             'calls': 2, 'warmup_calls': 1, 'kernel': 'stream-g2/strict/map', 'entry': 'gs_step_tb_mk_strict<4, 3, 1, 0>',
             'vgpr': 95, 'waves_per_simd': 5}),
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 2, 'mapped': False, 'pinned_kernel': 0, 'steps_per_call': 16,
             'calls': 2, 'warmup_calls': 40, 'kernel': 'tb-k4c1/strict.op', 'entry': 'gs_step_tb_mk_strict<4, 3, 1, 0>',
             'vgpr': 95, 'waves_per_simd': 5}),
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 2, 'mapped': True, 'pinned_kernel': 0, 'steps_per_call': 16,
             'calls': 2, 'warmup_calls': 40, 'kernel': 'tb-k4c1/strict.op/map', 'replay_kernel': 'simple/strict/map',
             'replay_steps': 672, 'proof': True, 'sum_v': 337.59180533252476, 'entry': 'gs_step_tb_mk_strict<4, 3, 1, 0>',
             'vgpr': 95, 'waves_per_simd': 5}),
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 2, 'mapped': True, 'pinned_kernel': 2, 'steps_per_call': 16,
             'calls': 2, 'warmup_calls': 1, 'kernel': 'stream-g2/strict/map', 'entry': 'gs_step_tb_mk_strict<4, 3, 1, 0>',
             'vgpr': 95, 'waves_per_simd': 5}),
        ]},
    'mask': {
        'header': [('| grid | no mask: kernel | Mcells x steps / s | masked: kernel | Mcells x steps / s | masked / no ma'
                    'sk | masked streaming kernel | marching / streaming | VGPRs | waves per SIMD | replay (masked simple'
                    ' kernel) |'),
                   '|---|---|---|---|---|---|---|---|---|---|---|'],
        'timed': {
            'grid': ['ms', 'ms_all', 'rate'],
        },
        'rows': [
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 1, 'masked': False, 'pinned_kernel': 0, 'steps_per_call': 16,
             'calls': 2, 'warmup_calls': 1, 'kernel': 'tile16x64/strict.op', 'entry': 'gs_step_tb_wk_strict<4, 3, 1, 0>',
             'vgpr': 105, 'waves_per_simd': 4}),
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 1, 'masked': True, 'pinned_kernel': 0, 'steps_per_call': 16,
             'calls': 2, 'warmup_calls': 40, 'kernel': 'tb-k4c1/strict.op/mask', 'replay_kernel': 'simple/strict/mask',
             'replay_steps': 672, 'proof': True, 'sum_v': 24.12636516611462, 'entry': 'gs_step_tb_wk_strict<4, 3, 1, 0>',
             'vgpr': 105, 'waves_per_simd': 4}),
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 1, 'masked': True, 'pinned_kernel': 2, 'steps_per_call': 16,
             'calls': 2, 'warmup_calls': 1, 'kernel': 'stream-g2/strict/mask', 'entry': 'gs_step_tb_wk_strict<4, 3, 1, 0>',
             'vgpr': 105, 'waves_per_simd': 4}),
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 2, 'masked': False, 'pinned_kernel': 0, 'steps_per_call': 16,
             'calls': 2, 'warmup_calls': 40, 'kernel': 'tb-k4c1/strict.op', 'entry': 'gs_step_tb_wk_strict<4, 3, 1, 0>',
             'vgpr': 105, 'waves_per_simd': 4}),
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 2, 'masked': True, 'pinned_kernel': 0, 'steps_per_call': 16,
             'calls': 2, 'warmup_calls': 40, 'kernel': 'tb-k4c1/strict.op/mask', 'replay_kernel': 'simple/strict/mask',
             'replay_steps': 672, 'proof': True, 'sum_v': 24.12636516611462, 'entry': 'gs_step_tb_wk_strict<4, 3, 1, 0>',
             'vgpr': 105, 'waves_per_simd': 4}),
            ('grid', {'rows': 96, 'cols': 160, 'slabs': 2, 'masked': True, 'pinned_kernel': 2, 'steps_per_call': 16,
             'calls': 2, 'warmup_calls': 1, 'kernel': 'stream-g2/strict/mask', 'entry': 'gs_step_tb_wk_strict<4, 3, 1, 0>',
             'vgpr': 105, 'waves_per_simd': 4}),
        ]},
}


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("tool", list(ARGS))
def test_rate_tool_prints_what_it_printed_before(built, tmp_path, tool):
    want = EXPECTED[tool]
    r, md, rows = run_rate_tool(tool, ARGS[tool], tmp_path)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert md[:2] == want["header"]
    assert len(rows) == len(want["rows"]), rows
    for got, (group, fixed) in zip(rows, want["rows"]):
        assert set(got) == set(fixed) | set(want["timed"][group]), (sorted(got), sorted(fixed), want["timed"][group])
        for key, value in fixed.items():
            assert _same(got[key], value), (key, got[key], value, got)
        for key in ("proof", "bitcheck"):
            assert got.get(key, True) is True, got
