"""Regional power spectra in a multi-process context: gs_fields_region_spectrum is collective and gives every rank every
region, bit for bit the single-process result; a rank seam that is no multiple of the region height is refused on every rank
alike.  All ranks share device 0 through the shared-memory transport double (tests/cpp/shm_transport.cpp, built as
tests/test_gpu_multiprocess.py builds it)."""
import os

import numpy as np
import pytest

from tests.children import rank_session, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
ROWS, COLS, WORLD = 96, 300, 2
ALIGNED = [((16, 64), 16), ((48, 132), 32), ((24, 300), 16)]         # (region, tile): the seam at row 48 is a multiple of rh
UNALIGNED = ((32, 64), 16)                                           # ... and one of which it is not


def _planes():
    from tests.helpers import stress_fields

    u, v = stress_fields((ROWS, COLS), 14)
    v[47:49, 10] = np.float32(np.inf)
    u[63, ::3] = np.float32(np.nan)
    return u, v


def _results(species, region, tile):
    out = []
    for s in species.region_spectrum(region, tile, "hann"):
        out += [s.raw, s.tiles_used, s.tiles_skipped]
    return out


def _worker(rank, world, port, out_dir, transport_lib):
    from grayscott_amd import capi
    from tests.helpers import species_from_arrays

    with rank_session(rank, world, port, transport_lib, ROWS) as (sim, (r0, r1)):
        u0, v0 = _planes()
        species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(ROWS, COLS))
        before = sim.context.stats()
        got = {}
        for k, (region, tile) in enumerate(ALIGNED):
            for i, a in enumerate(_results(species, region, tile)):
                got[f"r{k}_{i}"] = a
        try:
            species.region_spectrum(UNALIGNED[0], UNALIGNED[1], "hann")
            refused = 0
        except capi.GsError as e:
            refused = e.code
        for i, a in enumerate(_results(species, *ALIGNED[0])):                 # the context goes on working
            assert a.tobytes() == got[f"r0_{i}"].tobytes()
        assert sim.context.stats() == before
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), refused=np.array(refused), **got)


def test_every_rank_gets_every_region(tmp_path, built, shm_transport):
    from grayscott_amd import HipArgs, Parameters, Simulation, capi
    from grayscott_amd.simulation import spectrum_tables
    from tests import region_spectrum_ref
    from tests.helpers import free_port, species_from_arrays

    spawn_ranks(_worker, (WORLD, free_port(), str(tmp_path), shm_transport), WORLD)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    u0, v0 = _planes()
    species = species_from_arrays(sim, u0, v0)
    for k, (region, tile) in enumerate(ALIGNED):
        want = _results(species, region, tile)
        h, w = spectrum_tables(tile)
        for p, plane in enumerate((u0, v0)):
            power, tiles = region_spectrum_ref.by_crop(plane, region, tile, 1, h, w)
            assert want[3 * p].tobytes() == power.tobytes() and np.array_equal(want[3 * p + 2], tiles[..., 1]), (region, p)
        for rank in range(WORLD):
            z = np.load(tmp_path / f"rank{rank}.npz")
            assert int(z["refused"]) == capi.GS_ERR_UNSUPPORTED, (rank, z["refused"])
            for i, a in enumerate(want):
                assert z[f"r{k}_{i}"].dtype == a.dtype and z[f"r{k}_{i}"].tobytes() == a.tobytes(), (rank, region, i)
    sim.context.close()
