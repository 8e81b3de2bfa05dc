"""tools/time_stats_rate.py run once at a tiny size: every row it promises is there, with the bytes the rule implies."""
import os
import sys

import pytest

from tests.children import ROOT, run_rate_tool


def test_bytes_per_cell():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import time_stats_rate as tool

    assert [tool.bytes_per_cell(g) for _, g in tool.GROUP_SETS] == [20, 36, 20, 68]
    assert [name for name, _ in tool.GROUP_SETS] == ["sum", "sum+squares", "extremes", "all"]


@pytest.mark.gpu
def test_the_tool_runs_at_a_tiny_size(built, tmp_path):
    r, table, rows = run_rate_tool("time_stats", ["--calls", "2", "--grids", "40x300"], tmp_path, limit=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [(x["grid"], x["planes"], x["groups"]) for x in rows] == \
        [("40x300", n, g) for n in (1, 2) for g in ("sum", "sum+squares", "extremes", "all")] + \
        [("512 x 64x128", 2, g) for g in ("sum", "sum+squares", "extremes", "all")]
    for x in rows:
        assert x["accumulate_device_ms"] > 0 and x["copy_ms"] > 0 and x["summary_device_ms"] > 0 and x["host_route_ms"] > 0
        assert x["bytes_per_cell_and_plane"] == {"sum": 20, "sum+squares": 36, "extremes": 20, "all": 68}[x["groups"]]
    assert table[0].startswith("| grid | planes | groups |") and len(table) == 2 + len(rows)
