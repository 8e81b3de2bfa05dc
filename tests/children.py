"""The one place where tests start processes: compilers, compiled programs, tools, python children and the ranks of a
multi-process test.  Every child runs under a time limit of its own, and after a child that aborted, faulted or ran out of
time nothing more is started: ``died`` names that child, and every launcher here first asserts that it is empty.  The rule
matters on a GPU: a program that has faulted the card may have left it in a state in which the next one hangs.

What this module cannot do is stop the in-process GPU tests of a plain ``pytest -m gpu`` run after such a death: only a
``conftest.py`` could skip them (tools/gpu_run.sh runs pytest with ``-x``, which ends the run at the first failure).

A child that merely exits non-zero, or a rank that raises a Python exception, is a failing test and not a death.

This module imports neither the package nor torch at the top, so that CPU test files can use it cheaply."""
from __future__ import annotations

import contextlib
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grayscott_amd")

died = []  # the first child that aborted, faulted or ran out of time: nothing is started after it


def _deadly(returncode) -> bool:
    """Exit statuses that mean the process did not end itself: a signal, an abort (134) or a segmentation fault (139)."""
    return returncode < 0 or returncode in (134, 139)


def _may_start(what: str):
    assert not died, f"not started: {died[0]} died before"
    return what


def run_program(cmd, *, limit=120, **kw):
    """``subprocess.run`` of ``cmd`` with its output captured as text, under ``limit`` seconds; returns the
    ``CompletedProcess``, on which the caller asserts what it expects."""
    cmd = [str(c) for c in cmd]
    what = _may_start(" ".join(os.path.basename(c) for c in cmd[:3])[:80])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, **kw)   # (ends the child at the limit)
    except subprocess.TimeoutExpired:
        died.append(f"{what} (timeout)")
        pytest.fail(f"{what} did not end within {limit} s")
    if _deadly(r.returncode):
        died.append(f"{what} (exit status {r.returncode})")
    return r


def build_program(name, out_dir, *, library=True, sanitize=False, source=None) -> str:
    """Compile tests/cpp/NAME.cpp (or ``source``) into ``out_dir``/NAME, warnings being errors: against libgs_hip.so with
    ``library``, else a stand-alone program with debug information, which ``sanitize`` builds with the address and
    undefined-behaviour sanitizers.  Returns the program's path."""
    exe = os.path.join(str(out_dir), name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")]
    if not library:
        cmd += ["-g"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd += [str(source or os.path.join(ROOT, "tests", "cpp", f"{name}.cpp")), "-o", exe]
    if library:
        cmd += ["-L", LIBDIR, "-lgs_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"]
    r = run_program(cmd, limit=300)
    assert r.returncode == 0, r.stderr
    return exe


def build_shm_transport() -> str:
    """Compile the librccl test double (tests/cpp/shm_transport.cpp: the same eight nccl* entry points over shared-memory
    mailboxes; host code only, hipcc for the HIP runtime headers) unless it is up to date; returns its path."""
    from grayscott_amd import _build

    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    lib = os.path.join(out_dir, "libshm_transport.so")
    src = os.path.join(ROOT, "tests", "cpp", "shm_transport.cpp")
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        r = run_program([_build.hipcc(), "-O2", "-fPIC", "-shared", "-std=c++17", "-x", "hip", "--offload-arch=gfx950",
                         src, "-o", lib, "-lrt", "-lpthread"], limit=600)
        assert r.returncode == 0, r.stderr
    return lib


@pytest.fixture(scope="module")
def shm_transport(built):
    return build_shm_transport()


def join_ranks(rank, world, port, transport_lib, rows, local_slabs=1, own_device=False):
    """What every worker of a multi-process test does first: the torchrun environment of rank ``rank`` of ``world``
    (``transport_lib``, when given, takes librccl's place), the gloo bootstrap that carries the unique id, the ``HipArgs``
    of a process with ``local_slabs`` slabs -- on device 0, or with ``own_device`` on device ``rank`` where the box has a
    GPU per rank -- and this rank's rows [r0, r1) of a grid of ``rows`` rows.  Returns ``(args, (r0, r1))``."""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    if transport_lib:
        os.environ["GS_RCCL_LIBRARY"] = transport_lib
    from grayscott_amd import HipArgs, capi
    from grayscott_amd import dist as gsd

    info = gsd.bootstrap(backend="gloo", device="cpu")     # unique id travels over gloo
    device = rank if own_device and capi.device_count() >= world else 0
    args = HipArgs(devices=[device] * local_slabs, rank=info.rank, world=info.world, unique_id=info.unique_id)
    slabs = world * local_slabs
    r0 = gsd.slab_range(rows, slabs, rank * local_slabs)[0]
    r1 = gsd.slab_range(rows, slabs, (rank + 1) * local_slabs - 1)[1]
    return args, (r0, r1)


@contextlib.contextmanager
def rank_session(rank, world, port, transport_lib, rows, local_slabs=1, *, params=None, own_device=False):
    """The frame of a worker: ``join_ranks``, a ``Simulation`` of ``params`` (the defaults when None) and, after the body,
    the barrier that keeps every rank until all are done, then the teardown.  Yields ``(sim, (r0, r1))``.  A body that
    raises skips the barrier: the exception ends the rank, and with it the test."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from grayscott_amd import Parameters, Simulation

    args, own_rows = join_ranks(rank, world, port, transport_lib, rows, local_slabs, own_device)
    sim = Simulation.new(params or Parameters(), args)
    yield sim, own_rows
    dist.barrier()
    sim.context.close()
    dist.destroy_process_group()


def spawn_ranks(worker, args, world, *, limit=120):
    """``worker(rank, *args)`` in ``world`` spawned processes, under one time limit.  A failing rank makes the join raise,
    as ``mp.spawn(..., join=True)`` does; at the limit every rank still alive is ended and the test fails."""
    import torch.multiprocessing as mp

    what = _may_start(f"the ranks of {getattr(worker, '__module__', '?')}.{getattr(worker, '__name__', worker)}")
    ctx = mp.spawn(worker, args=tuple(args), nprocs=world, join=False)
    end = time.monotonic() + limit
    try:
        while not ctx.join(timeout=1.0):
            if time.monotonic() > end:
                died.append(f"{what} (timeout)")
                pytest.fail(f"the ranks did not end within {limit} s")
    except mp.ProcessExitedException as e:
        if _deadly(e.exit_code):
            died.append(f"{what} (rank {e.error_index}: exit status {e.exit_code})")
        raise
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
        for p in ctx.processes:
            p.join(5.0)


def run_rate_tool(name, args, tmp_path, *, limit=120):
    """tools/NAME_rate.py with ``args`` and its two report files under ``tmp_path``.  Returns ``(completed, md_lines,
    json_rows)``: the lines of the markdown table and the rows of the JSON file, a list or one object per line (both
    empty where the tool failed: the caller's assertion on the exit status then speaks first)."""
    out_json, out_md = tmp_path / "out" / "rows.json", tmp_path / "table.md"
    r = run_program([sys.executable, os.path.join(ROOT, "tools", f"{name}_rate.py")] + [str(a) for a in args]
                    + ["--json", str(out_json), "--md", str(out_md)], limit=limit, cwd=ROOT)
    if r.returncode != 0:
        return r, [], []
    md, text = out_md.read_text().splitlines(), out_json.read_text()
    rows = json.loads(text) if text.lstrip().startswith("[") else [json.loads(line) for line in text.splitlines()]
    return r, md, rows


_handed_out = set()


def free_port() -> int:
    """A port nobody listens on and that this test process has not handed out before: the kernel gives a closed
    ephemeral port out again at once, and the rendezvous store of the previous test may still hold it (EADDRINUSE in
    the next test's TCPStore, seen once on the GPU box)."""
    import random
    import socket

    rng = random.Random(os.getpid() * 7919 + len(_handed_out))
    for _ in range(200):
        port = rng.randrange(20000, 45000)
        if port in _handed_out:
            continue
        with socket.socket() as s:
            try:
                s.bind(("127.0.0.1", port))
            except OSError:
                continue
        _handed_out.add(port)
        return port
    raise RuntimeError("no free port found")
