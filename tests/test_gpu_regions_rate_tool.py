"""tools/regions_rate.py at a small size: it runs through, and its table has every column filled."""
import pytest

from tests.children import run_rate_tool

pytestmark = pytest.mark.gpu


def test_regions_rate_runs_and_fills_its_table(built, tmp_path):
    r, lines, rows = run_rate_tool("regions", ["--grids", "256x512", "--regions", "64x64", "--calls", "2"], tmp_path)
    assert r.returncode == 0, r.stderr
    columns = lines[0].count("|") - 1
    assert columns == 13 and lines[1] == "|" + "---|" * columns and len(lines) == 2 + 2          # the inputs `new` and `random`
    for line in lines[2:]:
        cells = [c.strip() for c in line.strip("|").split("|")]
        assert len(cells) == columns and all(cells) and "-" not in cells and "nan" not in line, line
        assert cells[:2] == ["256x512", "64x64"] and all(float(c) > 0 for c in cells[3:]), line
    assert [r["input"] for r in rows] == ["new", "random"]
    for row in rows:
        for key in ("region_summary_ms", "summary_ms", "region_quads1_ms", "quads1_ms", "region_quads4_ms", "quads4_ms", "host_ms",
                    "summary_ratio", "quads1_ratio", "quads4_ratio"):
            assert row[key] > 0, (key, row)
