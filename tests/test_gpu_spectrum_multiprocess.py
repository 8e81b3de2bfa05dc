"""Power spectra in a multi-process context: gs_fields_spectrum is collective and gives every rank the global result, bit for
bit the single-process one; a rank seam that is no multiple of the tile size is refused on every rank alike.  Both ranks
share device 0 through the shared-memory transport double (tests/cpp/shm_transport.cpp, built as
tests/test_gpu_multiprocess.py builds it)."""
import os

import numpy as np
import pytest

from tests.children import rank_session, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
ROWS, COLS = 96, 300
ALIGNED = ((16, "hann"), (16, "none"))                                    # the seam at row 48 is a multiple of 16 ...
UNALIGNED = 32                                                            # ... and not of 32


def _planes():
    from tests.helpers import stress_fields

    u, v = stress_fields((ROWS, COLS), 23)
    u = (u - np.float32(0.5)) * np.float32(3.0)
    v[70, 40] = np.float32(np.nan)                                        # a skipped tile in the second rank's rows
    return u, v


def _results(species, tile, window):
    out = {}
    for name, s in zip("uv", species.spectrum(tile, window)):
        out[f"{name}_power"] = s.raw
        out[f"{name}_tiles"] = np.array([s.tiles_used, s.tiles_skipped], np.uint64)
    return out


def _worker(rank, world, port, out_dir, transport_lib):
    from grayscott_amd import capi
    from tests.helpers import species_from_arrays

    with rank_session(rank, world, port, transport_lib, ROWS) as (sim, (r0, r1)):
        u0, v0 = _planes()
        species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(ROWS, COLS))
        before = sim.context.stats()
        got = {}
        for k, (tile, window) in enumerate(ALIGNED):
            for name, a in _results(species, tile, window).items():
                got[f"c{k}_{name}"] = a
        try:
            species.spectrum(UNALIGNED, "hann")
            refused = 0
        except capi.GsError as e:
            refused = e.code
        for name, a in _results(species, *ALIGNED[0]).items():                 # the context goes on working
            assert a.tobytes() == got[f"c0_{name}"].tobytes()
        assert sim.context.stats() == before
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), refused=np.array(refused), **got)


def test_every_rank_gets_the_global_spectrum(tmp_path, built, shm_transport):
    from grayscott_amd import HipArgs, Parameters, Simulation, capi
    from grayscott_amd.simulation import spectrum_tables
    from tests import spectrum_ref as ref
    from tests.helpers import free_port, species_from_arrays

    world = 2
    spawn_ranks(_worker, (world, free_port(), str(tmp_path), shm_transport), world)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = _planes()
    species = species_from_arrays(sim, u0, v0)
    for k, (tile, window) in enumerate(ALIGNED):
        want = _results(species, tile, window)
        h, w = spectrum_tables(tile)
        power, tiles = ref.spectrum(v0, tile, 1 if window == "hann" else 0, h, w)
        assert want["v_power"].tobytes() == power.tobytes() and tuple(want["v_tiles"]) == tuple(tiles) and tiles[1] == 1
        for rank in range(world):
            z = np.load(tmp_path / f"rank{rank}.npz")
            assert int(z["refused"]) == capi.GS_ERR_UNSUPPORTED, (rank, z["refused"])
            for name, a in want.items():
                assert z[f"c{k}_{name}"].dtype == a.dtype and z[f"c{k}_{name}"].tobytes() == a.tobytes(), (rank, tile, window, name)
    sim.context.close()
