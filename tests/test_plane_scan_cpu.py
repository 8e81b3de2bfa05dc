"""The header the plane-scanning kernels share (grayscott_amd/csrc/gs_plane_scan.h), checked without a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True])
def test_set_rule_grid_sizing_and_vector_verdict_on_the_host(tmp_path, sanitize):
    """tests/cpp/plane_scan.cpp: gs_is_set against the rule of include/gs_hip.h written out independently, gs_scan_groups by
    its properties and gs_plane_set's 16-byte verdict against a table -- a stand-alone program, also built with the address
    and undefined-behaviour sanitizers."""
    exe = tmp_path / "plane_scan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd += [os.path.join(ROOT, "tests", "cpp", "plane_scan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]

