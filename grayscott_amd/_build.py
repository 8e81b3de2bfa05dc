"""In-tree build of ``libgs_hip.so`` with hipcc for gfx950 (no cmake, no JIT cache).

The step kernels are five sources (``gs_step_kernels.hip`` and ``gs_step_{op,map,mask,noise}.hip``), each compiled once
per arithmetic flavour (the ``.op`` unit: strict only), nine objects in all:

* strict: ``-DGS_MATH_FUSED=0`` with f32 denormal mode "flush results, keep inputs"
  (``-fdenormal-fp-math-f32=preserve-sign,ieee`` -> ``.amdhsa_float_denorm_mode_32 1``),
  the GPU equivalent of the reference's MXCSR.FTZ ``DenormalsFlusher``;
* fused:  ``-DGS_MATH_FUSED=1`` with hipcc's default (keep denormals).

Both with ``-ffp-contract=off``: parity with the reference's naive backend is bit for
bit, so the compiler must never contract ``a*b+c`` on its own.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
BUILD = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libgs_hip.so")
ARCH = "gfx950"

COMMON = ["--offload-arch=" + ARCH, "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off",
          "-fno-fast-math", "-Wall", "-Wno-unused-function"]
# Experiment hook (tools/sweep runs): extra hipcc flags for the kernel translation units.
EXTRA = os.environ.get("GS_HIP_EXTRA_FLAGS", "").split()

# The step kernels are built without the SLP vectoriser: v_pk_*_f32 has the lane throughput of the
# plain ops on gfx950 and the packing costs ~10 % extra v_mov (profiles/archive/r01_sweeps.md, runs 49-57).
KERNEL_FLAGS = ["-fno-slp-vectorize"]
STRICT = ["-DGS_MATH_FUSED=0", "-Xclang", "-fdenormal-fp-math-f32=preserve-sign,ieee"]

UNITS = [
    # (source, object, extra flags)
    ("gs_step_kernels.hip", "gs_step_strict.o", STRICT + KERNEL_FLAGS),
    # the parameter-specialised strict variants: their own translation unit, compiled in parallel
    ("gs_step_op.hip", "gs_step_strict_op.o", STRICT + KERNEL_FLAGS),
    ("gs_step_kernels.hip", "gs_step_fused.o", ["-DGS_MATH_FUSED=1"] + KERNEL_FLAGS),
    # the parameter map's forms of the marching kernel (gs_step_tb_mk), one translation unit per flavour
    ("gs_step_map.hip", "gs_step_strict_map.o", STRICT + KERNEL_FLAGS),
    ("gs_step_map.hip", "gs_step_fused_map.o", ["-DGS_MATH_FUSED=1"] + KERNEL_FLAGS),
    # the domain mask's forms of the marching kernel (gs_step_tb_wk), likewise
    ("gs_step_mask.hip", "gs_step_strict_mask.o", STRICT + KERNEL_FLAGS),
    ("gs_step_mask.hip", "gs_step_fused_mask.o", ["-DGS_MATH_FUSED=1"] + KERNEL_FLAGS),
    # the noise forms of the marching kernel (gs_step_tb_zk) and of the ensemble kernels, likewise
    ("gs_step_noise.hip", "gs_step_strict_noise.o", STRICT + KERNEL_FLAGS),
    ("gs_step_noise.hip", "gs_step_fused_noise.o", ["-DGS_MATH_FUSED=1"] + KERNEL_FLAGS),
    ("gs_util_kernels.hip", "gs_util.o", []),
    # summaries of planes (row records, the ensembles' fold): hipcc's default float mode, sub-normal cells kept
    ("gs_summary.hip", "gs_summary_k.o", []),
    # histograms of planes (counts in LDS, flushed to u64 counters): the same float mode, a sub-normal cell is binned as it is
    ("gs_histogram.hip", "gs_histogram_k.o", []),
    # bit-quad counts of thresholded planes (one pass for up to four thresholds): the same float mode, a sub-normal cell is
    # compared as it is
    ("gs_morphology.hip", "gs_morphology_k.o", []),
    # regional observables (summaries and bit-quad counts per region of one plane): the same float mode as their whole-grid
    # twins, sub-normal cells kept
    ("gs_regions.hip", "gs_regions_k.o", []),
    # two-point pair counts of thresholded planes (lags 0..64 along four directions, one pass for up to four thresholds):
    # the same float mode
    ("gs_correlation.hip", "gs_correlation_k.o", []),
    # regional two-point pair counts (a region's border is a wall for pairs): the same float mode
    ("gs_region_pairs.hip", "gs_region_pairs_k.o", []),
    # regional histograms (counts per tile of regions in LDS, flushed to the regions' u64 counters): the same float mode as
    # gs_histogram.hip, a sub-normal cell is binned as it is
    ("gs_region_hist.hip", "gs_region_hist_k.o", []),
    # connected components of thresholded planes (union-find over a u32 parent per cell; tile, border, flatten and tally
    # launches): the same float mode
    ("gs_components.hip", "gs_components_k.o", []),
    # regional connected components (the same labelling with the regions' borders as walls, a tally per region): the same
    # float mode
    ("gs_region_components.hip", "gs_region_components_k.o", []),
    # component lists: one record per component behind that labelling (count, scan, write, gather launches; integer atomics):
    # the same float mode
    ("gs_component_list.hip", "gs_component_list_k.o", []),
    # component matches: one overlap per piece that two labellings share (one launch behind the lists'; no atomics): the same
    # float mode
    ("gs_match.hip", "gs_match_k.o", []),
    # reduced result images (block averages in f64): the same float mode, a sub-normal pixel is kept
    ("gs_reduce.hip", "gs_reduce_k.o", []),
    # two planes compared (row records of |a - b| in f64, the ensembles' fold): the same float mode, sub-normal cells kept
    ("gs_change.hip", "gs_change_k.o", []),
    # regional state comparison (a wave per region, or row records and a fold): the same float mode as gs_change.hip
    ("gs_region_change.hip", "gs_region_change_k.o", []),
    # power spectra (f32 radix-2 transforms of tiles in LDS, f64 sums per segment of tiles and per band): the same float mode,
    # sub-normal values kept
    ("gs_spectrum.hip", "gs_spectrum_k.o", []),
    # regional power spectra (the same tile body from gs_spectrum_tile.h, segments and bands counted inside a region, the
    # fold per region): the same float mode as gs_spectrum.hip
    ("gs_region_spectrum.hip", "gs_region_spectrum_k.o", []),
    # time statistics (per-cell f64 sums, f32 extremes and u32 crossing counters read, updated and written back per sample):
    # the same float mode, a sub-normal sample counts as the value it is
    ("gs_time_stats.hip", "gs_time_stats_k.o", []),
    # bundle statistics (the same accumulators across the members of a bundle, kept in registers; only results are written):
    # the same float mode, a sub-normal value counts as the value it is
    ("gs_bundle_stats.hip", "gs_bundle_stats_k.o", []),
    # the host side (contexts and schedule, planes, kernel configuration, the window kernel's runtime, RCCL): only the
    # C ABI of include/gs_hip.h is visible outside the library
    ("gs_api.cpp", "gs_api.o", ["-x", "hip", "-fvisibility=hidden"]),
    ("gs_fields.cpp", "gs_fields.o", ["-x", "hip", "-fvisibility=hidden"]),
    ("gs_tuner.cpp", "gs_tuner.o", ["-x", "hip", "-fvisibility=hidden"]),
    ("gs_window.cpp", "gs_window.o", ["-x", "hip", "-fvisibility=hidden"]),
    ("gs_rccl.cpp", "gs_rccl.o", ["-x", "hip", "-fvisibility=hidden"]),
    ("gs_ensemble.cpp", "gs_ensemble.o", ["-x", "hip", "-fvisibility=hidden"]),
    ("gs_attached.cpp", "gs_attached.o", ["-x", "hip", "-fvisibility=hidden"]),
    ("gs_observe.cpp", "gs_observe.o", ["-x", "hip", "-fvisibility=hidden"]),
    ("gs_time_stats.cpp", "gs_time_stats.o", ["-x", "hip", "-fvisibility=hidden"]),
    ("gs_bundle_stats.cpp", "gs_bundle_stats.o", ["-x", "hip", "-fvisibility=hidden"]),
    # the opt-in table for more than 64 KB of dynamic LDS, shared by the step kernels' launchers
    ("gs_dyn_lds.cpp", "gs_dyn_lds.o", ["-x", "hip", "-fvisibility=hidden"]),
]


def hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: libgs_hip.so cannot be built")
    return exe


def _sources():
    out = [os.path.join(CSRC, n) for n in os.listdir(CSRC)]
    out.append(os.path.join(HERE, os.pardir, "include", "gs_hip.h"))
    out.append(os.path.abspath(__file__))
    return out


def up_to_date() -> bool:
    if not os.path.exists(LIB):
        return False
    t = os.path.getmtime(LIB)
    return all(os.path.getmtime(s) <= t for s in _sources())


def build(force: bool = False, verbose: bool = False, lib: str = LIB, build_dir: str = BUILD,
          extra_flags=()) -> str:
    """Compile every HIP translation unit and link ``libgs_hip.so``; returns its path.
    ``lib`` / ``build_dir`` / ``extra_flags`` build a variant next to it (tools/ab_build.py)."""
    if lib == LIB and not force and up_to_date():
        return LIB
    os.makedirs(build_dir, exist_ok=True)
    cc = hipcc()
    procs = []
    for src, obj, extra in UNITS:
        flags = list(COMMON) + ((EXTRA + list(extra_flags)) if src.endswith(".hip") else [])
        cmd = [cc] + flags + extra + ["-c", os.path.join(CSRC, src), "-o", os.path.join(build_dir, obj)]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed:\n%s\n%s" % (" ".join(cmd), out.decode(errors="replace")))
        if verbose and out:
            sys.stderr.write(out.decode(errors="replace"))
    objs = [os.path.join(build_dir, obj) for _, obj, _ in UNITS]
    cmd = [cc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib] + objs + ["-ldl"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n%s\n%s" % (" ".join(cmd), r.stdout.decode(errors="replace")))
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
