"""The header the plane-scanning kernels share (grayscott_amd/csrc/gs_plane_scan.h), checked without a device."""
import pytest

from tests.children import build_program, run_program


@pytest.mark.parametrize("sanitize", [False, True])
def test_set_rule_grid_sizing_and_vector_verdict_on_the_host(tmp_path, sanitize):
    """tests/cpp/plane_scan.cpp: gs_is_set against the rule of include/gs_hip.h written out independently, gs_scan_groups by
    its properties and gs_plane_set's 16-byte verdict against a table -- a stand-alone program, also built with the address
    and undefined-behaviour sanitizers."""
    exe = build_program("plane_scan", tmp_path, library=False, sanitize=sanitize)
    r = run_program([str(exe)])
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]

