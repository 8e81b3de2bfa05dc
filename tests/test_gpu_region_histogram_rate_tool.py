"""tools/region_histogram_rate.py at a small size: it runs through, and its table has every column filled."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_region_histogram_rate_runs_and_fills_its_table(built, tmp_path):
    md, js = tmp_path / "rh.md", tmp_path / "rh.json"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "region_histogram_rate.py"), "--grids", "256x512", "--regions", "64x64",
           "--bins", "64", "--calls", "2", "--md", str(md), "--json", str(js)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = md.read_text().splitlines()
    columns = lines[0].count("|") - 1
    assert columns == 10 and lines[1] == "|" + "---|" * columns and len(lines) == 2 + 2          # the inputs `new` and `random`
    for line in lines[2:]:
        cells = [c.strip() for c in line.strip("|").split("|")]
        assert len(cells) == columns and all(cells) and "-" not in cells and "nan" not in line, line
        assert cells[:3] == ["256x512", "64x64", "64"] and all(float(x) > 0 for c in cells[4:] for x in c.split(" / ")), line
    rows = json.loads(js.read_text())
    assert [r["input"] for r in rows] == ["new", "random"]
    for row in rows:
        for key in ("region_hist_ms", "region_hist_reused_ms", "hist_ms", "region_summaries_ms", "host_ms", "region_hist_ratio",
                    "region_hist_reused_ratio"):
            assert row[key] > 0, (key, row)
