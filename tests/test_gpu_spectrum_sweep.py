"""The sweep's ``--spectrum-every``: a 2 x 2 sweep of 64 x 128 records the members' power spectra into
``<stem>.spectrum.npz`` with the stated shapes, the last sample equal to ``Ensemble.spectra`` at the end state, and leaves
the fields as they are."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_sweep_records_spectra_without_changing_the_fields(built, tmp_path):
    from grayscott_amd import HipArgs, Parameters, Simulation, Spectrum, hdf5_min, sweep

    T = 64
    base = ["--feed", "0.02:0.05:2", "--kill", "0.05:0.062:2", "-r", "64", "-c", "128", "-s", "64"]
    sweep.main(base + ["-o", str(tmp_path / "plain.h5")])
    sweep.main(base + ["--spectrum-every", "32", "--spectrum-tile", str(T), "-o", str(tmp_path / "spec.h5")])
    assert (tmp_path / "plain.h5").read_bytes() == (tmp_path / "spec.h5").read_bytes()
    assert not (tmp_path / "plain.spectrum.npz").exists()
    z = np.load(tmp_path / "spec.spectrum.npz")
    assert list(z["steps"]) == [32, 64] and int(z["tile"]) == T and str(z["window"]) == "hann"
    assert z["power"].shape == (2, 4, 2, T, T // 2 + 1) and z["power"].dtype == np.float64
    assert z["tiles"].shape == (2, 4, 2, 2) and z["tiles"].dtype == np.uint64
    assert z["wavelength"].shape == (2, 4, 2) and z["wavelength"].dtype == np.float64
    assert np.all(z["tiles"][..., 0] == 2) and not z["tiles"][..., 1].any()
    # the end state again, member by member with its own parameters: the same bits
    args = sweep.parse(base)
    params = sweep.member_params(args)
    sim = Simulation.new(params[0], HipArgs(devices=[0]))
    ens = sim.make_ensemble((64, 128), params)
    ens.perform_steps(64)
    assert ens.result_views().tobytes() == hdf5_min.read(str(tmp_path / "spec.h5")).tobytes()
    power, tiles = ens.spectra(tile=T, window="hann")
    assert z["power"][-1].tobytes() == power.tobytes() and z["tiles"][-1].tobytes() == tiles.tobytes()
    for m in range(4):
        for s in range(2):
            want = Spectrum.from_raw(power[m, s], T, "hann", tiles[m, s]).wavelength()
            got = z["wavelength"][-1, m, s]
            assert (np.isnan(got) and want is None) or got == want, (m, s)
    ens.destroy()
    sim.context.close()
