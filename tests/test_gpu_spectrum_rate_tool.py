"""tools/spectrum_rate.py at a small size: it runs through, and its table has every column filled."""
import pytest

from tests.children import run_rate_tool

pytestmark = pytest.mark.gpu


def test_spectrum_rate_runs_and_fills_its_table(built, tmp_path):
    r, lines, rows = run_rate_tool("spectrum", ["--grids", "256x512", "--calls", "2"], tmp_path)
    assert r.returncode == 0, r.stderr
    columns = lines[0].count("|") - 1
    # the grid with tiles of 16, 64 and 128, the ensemble of 64 x 128 with 16 and 64; both windows each
    assert columns == 8 and lines[1] == "|" + "---|" * columns and len(lines) == 2 + 6 + 4
    for line in lines[2:]:
        cells = [c.strip() for c in line.strip("|").split("|")]
        assert len(cells) == columns and all(cells) and "-" not in cells and "nan" not in line, line
        assert cells[2] in ("hann", "none") and all(float(x) > 0 for x in cells[3:]), line
    assert [(x["tile"], x["window"]) for x in rows[:6]] == [(T, w) for T in (16, 64, 128) for w in ("hann", "none")]
    assert [x["tile"] for x in rows[6:]] == [16, 16, 64, 64]
    for row in rows:
        for key in ("spectrum_ms", "summary_ms", "ratio", "download_ms", "host_ms"):
            assert row[key] > 0, (key, row)
