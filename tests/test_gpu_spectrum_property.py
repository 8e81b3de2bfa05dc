"""Randomised parity of the on-device power spectra (gs_fields_spectrum, gs_members_spectrum) with their restatement
(tests/spectrum_ref.py), in the manner of tests/test_gpu_float_observe_property.py: a case draws the shape -- around the
seams of the fold: one tile, ragged sides, 16 / 17 / 33 tiles per band, no tile --, the tile size, the window, the values
(normal, uniform, scaled per tile into sub-normals and large numbers) salted with non-finite cells, the call form (one
field, a field list, ensemble members) and the slab count.  Checked: ``power`` as f64 bit patterns and ``tiles``; and, on
planes of at most 20 000 cells, sum |power - P| <= B(T) sum P against numpy's f64 transform of the same tiles (the bound of
tests/test_spectrum_cpu.py, summed over the tiles used).  The bound rests on fl(a op b) = (a op b)(1 + d), |d| <= u, which
holds only while no result falls into the sub-normal range: the ``scaled`` values, whose tiles of 1e-42 and 1e-30 have
powers far below the smallest f32, are held to the bits alone.

GS_PROPERTY_EXAMPLES_SPECTRUM sets the number of drawn cases (default 6)."""
import os

import numpy as np
import pytest
from hypothesis import HealthCheck, example, given, settings, strategies as st

from grayscott_amd import HipArgs, HipConcentration, Parameters, Simulation, capi
from grayscott_amd.simulation import spectrum_fields, spectrum_tables
from tests import spectrum_ref as ref

pytestmark = pytest.mark.gpu

WINDOWS = ("none", "hann")
EXACT_CELLS = 20000


@st.composite
def cases(draw):
    T = draw(st.sampled_from(ref.TILES))
    bands = draw(st.sampled_from([0, 1, 1, 2, 3] if T <= 32 else [0, 1, 1, 2]))
    per_band = draw(st.sampled_from([0, 1, 2, 15, 16, 17, 33] if T == 16 else ([0, 1, 2, 5, 17] if T == 32 else [0, 1, 2, 3])))
    rows = bands * T + draw(st.sampled_from([0, 0, 1, T - 1]))
    cols = per_band * T + draw(st.sampled_from([0, 0, 3, T - 1]))
    form = draw(st.sampled_from(["field", "fields", "members"]))
    slabs = draw(st.sampled_from([1, 1, 2, 4])) if form != "members" else 1
    if rows < 16 * slabs:                                                 # (a slab chain wants rows to share out)
        slabs = 1
    return dict(T=T, rows=max(rows, 1), cols=max(cols, 1), window=draw(st.sampled_from(WINDOWS)), form=form, slabs=slabs,
                values=draw(st.sampled_from(["normal", "uniform", "scaled"])), salt=draw(st.integers(0, 3)),
                seed=draw(st.integers(0, 2 ** 16)))


def planes_of(c, n):
    rng = np.random.default_rng(c["seed"])
    shape, T = (n, c["rows"], c["cols"]), c["T"]
    if c["values"] == "uniform":
        x = rng.random(shape, dtype=np.float32)
    else:
        x = rng.standard_normal(shape).astype(np.float32)
    if c["values"] == "scaled":
        for k, (b, j) in enumerate(np.ndindex(c["rows"] // T + 1, c["cols"] // T + 1)):
            x[:, b * T:(b + 1) * T, j * T:(j + 1) * T] *= np.float32((1e-42, 1e-30, 1.0, 1e12, 3e-39)[(k + c["seed"]) % 5])
    for _ in range(c["salt"]):
        at = tuple(int(rng.integers(0, s)) for s in shape)
        x[at] = (np.nan, np.inf, -np.inf)[int(rng.integers(0, 3))]
    return x


def refused(c):
    """A grid that has tiles on a slab chain with a seam off the tiles' rows: GS_ERR_UNSUPPORTED."""
    fit = all((k * c["rows"] // c["slabs"]) % c["T"] == 0 for k in range(1, c["slabs"]))
    return not fit and c["rows"] >= c["T"] and c["cols"] >= c["T"]


def run_case(c):
    T, window = c["T"], c["window"]
    n = {"field": 1, "fields": 3, "members": 2 * 3}[c["form"]]
    planes = planes_of(c, n)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * c["slabs"]))
    try:
        if c["form"] == "members":
            ens = sim.make_ensemble((c["rows"], c["cols"]), [Parameters()] * 3)
            ens.upload(planes[0::2], planes[1::2])
            power, tiles = ens.spectra(tile=T, window=window)
            got = [(power[m, s], tiles[m, s]) for m in range(3) for s in range(2)]
            ens.destroy()
        else:
            fields = []
            for p in planes:
                f = HipConcentration(sim.context, p.shape)
                f.upload(sim.context, p)
                fields.append(f)
            if refused(c):
                with pytest.raises(capi.GsError) as e:
                    spectrum_fields(sim.context, fields, T, window)
                assert e.value.code == capi.GS_ERR_UNSUPPORTED, c
                return
            got = [(s.raw, np.array([s.tiles_used, s.tiles_skipped], np.uint64)) for s in spectrum_fields(sim.context, fields, T, window)]
    finally:
        sim.context.close()
    h, w = spectrum_tables(T)
    for k, (power, tiles) in enumerate(got):
        want_power, want_tiles = ref.spectrum(planes[k], T, WINDOWS.index(window), h, w)
        assert tuple(int(x) for x in tiles) == tuple(int(x) for x in want_tiles), (c, k)
        assert power.tobytes() == want_power.tobytes(), (c, k, int((power.view(np.uint64) != want_power.view(np.uint64)).sum()))
        if planes[k].size <= EXACT_CELLS and int(tiles[0]) and c["values"] != "scaled":
            flat = ref.tiles_of(planes[k], T).reshape(-1, T, T)
            used = flat[np.isfinite(flat).all(axis=(1, 2))]
            P = ref.exact_power(used, h, WINDOWS.index(window)).sum(axis=0)
            err, total = np.abs(power - P).sum(), P.sum()
            print(f"T {T} {window} {c['values']}: sum |power - P| / sum P = {err / total if total else 0.0:.3e}, B = {ref.bound(T):.3e}")
            assert err <= ref.bound(T) * total, (c, k, err, total)


PINNED = [dict(T=16, rows=33, cols=273, window="hann", form="fields", slabs=2, values="scaled", salt=2, seed=1),
          dict(T=16, rows=48, cols=528, window="none", form="field", slabs=1, values="normal", salt=0, seed=2),
          dict(T=64, rows=131, cols=130, window="hann", form="members", slabs=1, values="uniform", salt=1, seed=3),
          dict(T=128, rows=128, cols=131, window="none", form="field", slabs=1, values="normal", salt=0, seed=4),
          dict(T=32, rows=15, cols=100, window="hann", form="field", slabs=1, values="normal", salt=0, seed=5),
          dict(T=32, rows=128, cols=70, window="hann", form="fields", slabs=4, values="uniform", salt=1, seed=6),
          dict(T=64, rows=128, cols=70, window="none", form="field", slabs=4, values="normal", salt=0, seed=7)]


def _with_examples(test):
    for case in reversed(PINNED):
        test = example(case)(test)
    return test


@settings(max_examples=int(os.environ.get("GS_PROPERTY_EXAMPLES_SPECTRUM", "6")), deadline=None,
          suppress_health_check=list(HealthCheck))
@given(cases())
@_with_examples
def test_any_spectrum_matches_the_reference(built, case):
    run_case(case)
