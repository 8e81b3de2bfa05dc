"""tools/bundle_stats_rate.py run once at its smallest arguments: the header line and every row's keys, no timed value."""
import os
import sys

import pytest

from tests.children import ROOT, run_rate_tool


def test_configurations_and_traffic():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bundle_stats_rate as tool

    assert tool.parse_configs(tool.CONFIGS) == [(512, 64, 128, 8), (512, 64, 128, 32), (64, 256, 512, 8)]
    for bad in ("8x4x4", "8x4x4x3", "0x4x4x1", "8x4xax2"):
        with pytest.raises(ValueError):
            tool.parse_configs(bad)
    # every member's U and V read once; n planes per bundle and species written
    assert tool.traffic(512, 64, 128, 8, 2) == (2 * 4 * 512 * 8192, 2 * 4 * 2 * 64 * 8192)
    assert [len(names) for _, names in tool.RESULT_SETS] == [2, 5]


@pytest.mark.gpu
def test_the_tool_runs_at_a_tiny_size(built, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bundle_stats_rate as tool

    r, table, rows = run_rate_tool("bundle_stats", ["--calls", "1", "--configs", "4x5x7x2"], tmp_path, limit=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert table[:2] == tool.HEADER and len(table) == 2 + len(rows)
    assert [(x["config"], x["span"], x["results"]) for x in rows] == [("4 x 5x7", 2, "mean+variance"), ("4 x 5x7", 2, "all five")]
    for x in rows:
        assert sorted(x) == sorted(tool.KEYS)
