"""tools/region_change_rate.py at a small size: it runs through, its check of what it timed holds, and its table has every
column filled."""
import pytest

from tests.children import run_rate_tool

pytestmark = pytest.mark.gpu


def test_region_change_rate_runs_and_fills_its_table(built, tmp_path):
    r, lines, rows = run_rate_tool("region_change", ["--grids", "256x512", "--regions", "64x64,128x256", "--calls", "2"], tmp_path)
    assert r.returncode == 0, r.stderr
    columns = lines[0].count("|") - 1
    assert columns == 11 and lines[1] == "|" + "---|" * columns and len(lines) == 2 + 2
    for line, region in zip(lines[2:], ("64x64", "128x256")):
        cells = [c.strip() for c in line.strip("|").split("|")]
        assert len(cells) == columns and all(cells) and "nan" not in line, line
        assert cells[:2] == ["256x512", region] and all(float(x) > 0 for x in cells[2:]), line
    assert [(row["region"], row["regions"]) for row in rows] == [("64x64", 32), ("128x256", 4)]
    for row in rows:
        assert row["checked"] is True
        for key in ("change_records_ms", "change_wave_ms", "change_ms", "python_ms", "compare_ms", "region_summaries_ms",
                    "compare_ratio", "summaries_ratio", "host_ms"):
            assert row[key] > 0, (key, row)
