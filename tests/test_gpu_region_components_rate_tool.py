"""tools/region_components_rate.py at a small size: it runs through, and its table has every column filled (the host route
where scipy is present)."""
import pytest

from tests.children import run_rate_tool

pytestmark = pytest.mark.gpu


def test_region_components_rate_runs_and_fills_its_table(built, tmp_path):
    try:
        import scipy.ndimage  # noqa: F401
        host = True
    except ImportError:
        host = False
    r, lines, rows = run_rate_tool("region_components", ["--grids", "256x512", "--regions", "64x64", "--calls", "2"], tmp_path)
    assert r.returncode == 0, r.stderr
    columns = lines[0].count("|") - 1
    assert columns == 10 and lines[1] == "|" + "---|" * columns and len(lines) == 2 + 3          # the inputs `new`, `random`, `full`
    for line in lines[2:]:
        cells = [c.strip() for c in line.strip("|").split("|")]
        assert len(cells) == columns and all(cells) and "nan" not in line, line
        assert cells[:2] == ["256x512", "64x64"] and all(float(x) > 0 for x in cells[3:9]), line
        assert (float(cells[9]) > 0) if host else cells[9] == "-", line
    assert [r["input"] for r in rows] == ["new", "random", "full"]
    assert rows[2]["components"] == 4 * 8 and rows[0]["components"] >= 1 and rows[1]["components"] > 4 * 8
    for row in rows:
        for key in ("region_components8_ms", "region_components4_ms", "components8_ms", "region_morphology_ms",
                    "region_components8_ratio") + (("host_ms",) if host else ()):
            assert row[key] > 0, (key, row)
