"""grayscott_amd/_build.py's list of translation units against the files under csrc/ (no library, no compiler)."""
import os

from grayscott_amd import _build


def test_every_source_is_built_and_every_unit_has_its_source():
    on_disk = {n for n in os.listdir(_build.CSRC) if n.endswith((".hip", ".cpp"))}
    listed = {src for src, _obj, _flags in _build.UNITS}
    assert listed - on_disk == set(), "UNITS names sources that do not exist"
    assert on_disk - listed == set(), "sources under csrc/ that no entry of UNITS compiles"
    objects = [obj for _src, obj, _flags in _build.UNITS]
    assert len(objects) == len(set(objects)), "two units write one object file"
