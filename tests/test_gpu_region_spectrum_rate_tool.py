"""tools/region_spectrum_rate.py at a small size: it runs through, and its table has every column filled."""
import pytest

from tests.children import run_rate_tool

pytestmark = pytest.mark.gpu


def test_region_spectrum_rate_runs_and_fills_its_table(built, tmp_path):
    r, lines, rows = run_rate_tool("region_spectrum", ["--grids", "256x512", "--regions", "64x64", "--tiles", "16", "--calls", "2"],
                                   tmp_path)
    assert r.returncode == 0, r.stderr
    columns = lines[0].count("|") - 1
    assert columns == 9 and lines[1] == "|" + "---|" * columns and len(lines) == 2 + 1
    for line in lines[2:]:
        cells = [c.strip() for c in line.strip("|").split("|")]
        assert len(cells) == columns and all(cells) and "-" not in cells and "nan" not in line, line
        assert cells[:3] == ["256x512", "64x64", "16"] and all(float(x) > 0 for c in cells[3:] for x in c.split(" / ")), line
    for row in rows:
        for key in ("region_spectrum_ms", "region_spectrum_reused_ms", "spectrum_ms", "region_summaries_ms", "host_ms",
                    "region_spectrum_ratio", "region_spectrum_reused_ratio"):
            assert row[key] > 0, (key, row)
