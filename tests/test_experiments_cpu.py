"""gs_experiments.h is the one place for build-time switches of the kernels: the sources, read as text (no library)."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grayscott_amd", "csrc")
HEADER = "gs_experiments.h"
# what _build.py sets per translation unit of the step kernels (gs_step_flavour.h): the build, not experiments
SELECTORS = {"GS_MATH_FUSED", "GS_SUFFIX"}


def _sources():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            out[name] = f.read()
    return out


def _defaulted(header):
    """NAME of every `#ifndef NAME` that the next line answers with `#define NAME`."""
    return set(re.findall(r"^[ \t]*#[ \t]*ifndef[ \t]+(\w+)[ \t]*\n[ \t]*#[ \t]*define[ \t]+\1\b", header, re.M))


def _documented(header):
    """NAME of every entry of part (1): a comment line that begins with the switch's name."""
    build_time = header.split("---- (2) run-time")[0]
    return set(re.findall(r"^// (GS_\w+)\s", build_time, re.M))


def test_every_default_is_used():
    src = _sources()
    names = _defaulted(src[HEADER])
    unused = sorted(n for n in names
                    if not any(re.search(r"\b%s\b" % n, text) for name, text in src.items() if name != HEADER))
    assert not unused, f"{HEADER} gives defaults to switches that no other file under csrc/ uses: {unused}"


def test_every_tested_switch_is_listed():
    src = _sources()
    known = _defaulted(src[HEADER]) | _documented(src[HEADER]) | SELECTORS
    assert {"GS_TB_TRACE", "GS_WIN_TRACE"} <= known  # (the entry format is still what _documented reads ...
    assert "GS_WIN_TAGGED" not in known              # ... and the paragraph of retired switches is no entry)
    strays = []
    for name, text in src.items():
        text = text.replace("\\\n", " ")  # a condition may continue on the next line
        for m in re.finditer(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", text, re.M):
            for macro in re.findall(r"\bGS_(?:TB|VS|WIN)_\w+", m.group(1).split("//")[0]):
                if macro not in known:
                    strays.append(f"{name}: {macro}")
    assert not strays, f"switches tested in an #if that {HEADER} neither defaults nor documents: {sorted(set(strays))}"


def test_no_macro_selects_a_translation_unit():
    """Every translation unit of the step kernels has a source file of its own: no `*_ONLY` macro anywhere under csrc/."""
    hits = sorted(f"{name}: {m}" for name, text in _sources().items() for m in set(re.findall(r"\b\w+_ONLY\b", text)))
    assert not hits, hits
