"""Regional state comparison in a multi-process context: gs_fields_region_compare is collective and gives every rank every
region's bits, equal to the definition, under both routes and the library's choice; a rank seam that is no multiple of the
region height is refused on every rank alike.  All ranks share device 0 through the shared-memory transport double
(tests/cpp/shm_transport.cpp, built as tests/test_gpu_multiprocess.py builds it)."""
import os

import numpy as np
import pytest

from tests.children import rank_session, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
ROWS, COLS, WORLD = 96, 300, 2
ALIGNED = [(16, 64), (48, 256)]                # region shapes whose rows the rank seam (row 48) is a multiple of
UNALIGNED = (32, 64)                           # ... and one that it is not
ROUTES = ("records", "wave", "")               # "": the library's choice
FIELDS = ("sum_abs", "sum_sq", "max_abs", "differing", "nonfinite")


def _planes():
    from tests import change_ref

    ua, ub = change_ref.order_sensitive((ROWS, COLS), 31)
    va, vb = change_ref.order_sensitive((ROWS, COLS), 32)
    ua[47:49, ::3], vb[63:65, ::5] = np.float32(np.nan), np.float32(np.inf)
    va[40:56, 100:200] = vb[40:56, 100:200]    # a block across the rank seam that has not moved
    return ua, va, ub, vb


def _results(species, snap, region):
    out = {}
    for route in ROUTES:
        os.environ["GS_HIP_REGION_CHANGE_ROUTE"] = route
        for name, c in zip("uv", species.region_changes_since(snap, region)):
            for f in FIELDS:
                out[f"{route or 'choice'}_{name}_{f}"] = getattr(c, f)
    os.environ.pop("GS_HIP_REGION_CHANGE_ROUTE")
    return out


def _worker(rank, world, port, out_dir, transport_lib):
    from grayscott_amd import capi
    from tests.helpers import species_from_arrays

    with rank_session(rank, world, port, transport_lib, ROWS) as (sim, (r0, r1)):
        ua, va, ub, vb = _planes()
        species = species_from_arrays(sim, ub[r0:r1], vb[r0:r1], shape=(ROWS, COLS))
        snap = species.snapshot()
        species.in_out()[0].upload(sim.context, ua[r0:r1])
        species.in_out()[1].upload(sim.context, va[r0:r1])
        before = sim.context.stats()
        got = {}
        for k, region in enumerate(ALIGNED):
            for key, a in _results(species, snap, region).items():
                got[f"r{k}_{key}"] = a
        try:
            species.region_changes_since(snap, UNALIGNED)
            refused = 0
        except capi.GsError as e:
            refused = e.code
        for key, a in _results(species, snap, ALIGNED[0]).items():             # the context goes on working
            assert a.tobytes() == got[f"r0_{key}"].tobytes(), key
        assert sim.context.stats() == before
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), refused=np.array(refused), **got)
        snap.close()


def test_every_rank_gets_every_region(tmp_path, built, shm_transport):
    from grayscott_amd import capi
    from tests import region_change_ref
    from tests.helpers import free_port

    spawn_ranks(_worker, (WORLD, free_port(), str(tmp_path), shm_transport), WORLD)
    ua, va, ub, vb = _planes()
    for k, region in enumerate(ALIGNED):
        want = {"u": region_change_ref.changes(ua, ub, region), "v": region_change_ref.changes(va, vb, region)}
        for rank in range(WORLD):
            z = np.load(tmp_path / f"rank{rank}.npz")
            assert int(z["refused"]) == capi.GS_ERR_UNSUPPORTED, (rank, z["refused"])
            for route in ROUTES:
                for name in "uv":
                    for f in FIELDS:
                        got = z[f"r{k}_{route or 'choice'}_{name}_{f}"]
                        assert got.dtype == want[name][f].dtype and got.tobytes() == want[name][f].tobytes(), (rank, region, route, name, f)
