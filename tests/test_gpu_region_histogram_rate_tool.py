"""tools/region_histogram_rate.py at a small size: it runs through, and its table has every column filled."""
import pytest

from tests.children import run_rate_tool

pytestmark = pytest.mark.gpu


def test_region_histogram_rate_runs_and_fills_its_table(built, tmp_path):
    r, lines, rows = run_rate_tool("region_histogram", ["--grids", "256x512",
                                                        "--regions", "64x64", "--bins", "64", "--calls", "2"], tmp_path)
    assert r.returncode == 0, r.stderr
    columns = lines[0].count("|") - 1
    assert columns == 10 and lines[1] == "|" + "---|" * columns and len(lines) == 2 + 2          # the inputs `new` and `random`
    for line in lines[2:]:
        cells = [c.strip() for c in line.strip("|").split("|")]
        assert len(cells) == columns and all(cells) and "-" not in cells and "nan" not in line, line
        assert cells[:3] == ["256x512", "64x64", "64"] and all(float(x) > 0 for c in cells[4:] for x in c.split(" / ")), line
    assert [r["input"] for r in rows] == ["new", "random"]
    for row in rows:
        for key in ("region_hist_ms", "region_hist_reused_ms", "hist_ms", "region_summaries_ms", "host_ms", "region_hist_ratio",
                    "region_hist_reused_ratio"):
            assert row[key] > 0, (key, row)
