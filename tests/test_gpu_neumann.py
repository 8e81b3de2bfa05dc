"""The zero-flux (Neumann) boundary rule on the MI355X: every kernel that kernel = AUTO or a pin reaches, bit for bit
against the pad-and-crop reference (tests/neumann_ref.py) in strict math and under the existing contract in fused math;
slab chains, row bands and several processes (only the global edges change); conservation of U + V with F = k = 0
(which the other rules do not have, so a site that falls back to one of them fails it); ensembles against lone Species;
the refusals; and the simulate and sweep drivers end to end."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

import oracle
from grayscott_amd import GsError, HipArgs, Parameters, Simulation, capi, hdf5_min

from . import neumann_ref
from .helpers import assert_bits_equal, gpu_run, oracle_params, species_from_arrays, stress_fields
from .test_gpu_property import tb_cols_per_wave
from tests.children import ROOT, run_program, shm_transport, spawn_ranks  # noqa: F401

pytestmark = pytest.mark.gpu
N = capi.GS_BOUNDARY_NEUMANN


def args(**kw):
    kw.setdefault("devices", [0])
    kw.setdefault("boundary", N)
    return HipArgs(**kw)


def fields(shape, seed):
    """seed < 0: Species::new's pattern; else the stress fields."""
    return oracle.init_species(*shape) if seed < 0 else stress_fields(shape, seed)


def is_neumann(name):
    return name.split("@")[0].endswith("/neumann")


# ---- AUTO: every path by shape; calls of 1, 2, 4, 26 and 67 steps = 1, 3, 7, 33 and 100 steps in all ----------------
AUTO_SHAPES = [(1, 1), (1, 9), (7, 1), (2, 2), (3, 5), (40, 37),   # the LDS-resident kernel
               (256, 512), (1000, 1003),                           # LDS-resident windows
               (1080, 1920), (777, 2049), (1500, 1503)]            # the marching kernel
CALLS = (1, 2, 4, 26, 67)


@pytest.mark.parametrize("shape", AUTO_SHAPES)
@pytest.mark.parametrize("seed", [-1, 5])
def test_auto_matches_the_reference(shape, seed):
    u0, v0 = fields(shape, seed)
    sim = Simulation.new(Parameters(), args())
    species = species_from_arrays(sim, u0, v0)
    ref_u, ref_v, done = u0, v0, 0
    names = []
    try:
        for n in CALLS:
            sim.perform_steps(species, n)
            ref_u, ref_v = neumann_ref.run(ref_u, ref_v, n)
            done += n
            name = sim.context.info()[0]
            names.append(name)
            assert is_neumann(name), name
            iu, iv, _, _ = species.in_out()
            assert_bits_equal(iu.make_scalar_view(sim.context), ref_u, f"U {shape} after {done} ({name})")
            assert_bits_equal(iv.make_scalar_view(sim.context), ref_v, f"V {shape} after {done} ({name})")
    finally:
        sim.context.close()
    cells = shape[0] * shape[1]
    want = "resident-lds" if cells <= 1536 else ("tile" if cells < 1_500_000 else "tb-")
    assert names[-1].startswith(want), (shape, names)


# ---- pinned kernels --------------------------------------------------------------------------------------------------
PIN_SHAPES = [(1, 1), (1, 9), (7, 1), (2, 2), (3, 5), (40, 37), (129, 250), (300, 701)]


@pytest.mark.parametrize("kernel", [capi.GS_KERNEL_SIMPLE, capi.GS_KERNEL_STREAM])
@pytest.mark.parametrize("shape", PIN_SHAPES + [(9, 257), (33, 255), (64, 1024)])
def test_single_step_kernels(shape, kernel):
    u0, v0 = stress_fields(shape, 11)
    ref_u, ref_v = neumann_ref.run(u0, v0, 7)
    got_u, got_v, info = gpu_run(u0, v0, 7, args=args(kernel=kernel), stepwise=True)
    assert info[0].endswith("/neumann"), info
    assert_bits_equal(got_u, ref_u, f"U {shape} {info[0]}")
    assert_bits_equal(got_v, ref_v, f"V {shape} {info[0]}")


TB_CONFIGS = ([dict(cols_per_lane=c, fuse_steps=k) for c in (1, 2, 4) for k in (1, 2, 3, 4)]
              + [dict(cols_per_lane=2, fuse_steps=k, share_taps=s) for s in (0, 1, 2, 3) for k in (2, 3, 4)]
              + [dict(cols_per_lane=c, fuse_steps=4, general_kernels=1) for c in (1, 2, 4)]
              + [dict(cols_per_lane=2, fuse_steps=4, use_graph=1), dict(fuse_steps=4, use_graph=1, rows_per_block=8)])


def edge_shapes(cfg):
    """Grids whose last strip of the marching kernel is 1 or K columns wide after a full one (cols = W + 1, W + K with
    W = tb_cols_per_wave(K, CPL), every CPL where the configuration leaves it to the library): the wrap or clamp of
    the last strip reaches past the strip before it."""
    k = cfg["fuse_steps"]
    return [s for c in ([cfg["cols_per_lane"]] if "cols_per_lane" in cfg else [1, 2, 4])
            for s in ((19, tb_cols_per_wave(k, c) + 1), (37, tb_cols_per_wave(k, c) + k))]


# every configuration in both flavours (the fused ones: the fused build's own marching kernels, its .op-less forms)
@pytest.mark.parametrize("cfg", TB_CONFIGS + [dict(c, math=capi.GS_MATH_FUSED) for c in TB_CONFIGS],
                         ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_marching_kernel_pinned(cfg):
    for shape in PIN_SHAPES + [(1000, 1003)] + edge_shapes(cfg):
        u0, v0 = stress_fields(shape, 3)
        steps = 37 if cfg.get("use_graph") else 11  # (a graph batch is 16 passes)
        ref_u, ref_v = neumann_ref.run(u0, v0, steps)
        got_u, got_v, info = gpu_run(u0, v0, steps, args=args(kernel=capi.GS_KERNEL_TB, no_tune=1, **cfg))
        assert info[0].startswith("tb-") and is_neumann(info[0]), info
        assert ("/fused" in info[0]) == (cfg.get("math") == capi.GS_MATH_FUSED), info
        assert_bits_equal(got_u, ref_u, f"U {shape} {cfg} {info[0]}")
        assert_bits_equal(got_v, ref_v, f"V {shape} {cfg} {info[0]}")


@pytest.mark.parametrize("cpl", [1, 2])
def test_fair_progress_form(cpl, monkeypatch):
    """GS_HIP_FAIR = 1: the 16-wave workgroups of one-round launches, in a fresh process (the switch is read once)."""
    code = (f"import sys; sys.path.insert(0, {ROOT!r})\n"
            "from tests import neumann_ref\nfrom tests.helpers import gpu_run, stress_fields\n"
            "from grayscott_amd import HipArgs, capi\n"
            "u0, v0 = stress_fields((1000, 1003), 6)\n"
            f"gu, gv, info = gpu_run(u0, v0, 12, args=HipArgs(devices=[0], boundary=3, kernel=capi.GS_KERNEL_TB, no_tune=1, "
            f"fuse_steps=4, cols_per_lane={cpl}))\n"
            "ru, rv = neumann_ref.run(u0, v0, 12)\n"
            "assert 'f/' in info[0] and info[0].split('@')[0].endswith('/neumann'), info\n"
            "assert gu.tobytes() == ru.tobytes() and gv.tobytes() == rv.tobytes(), info\n")
    env = dict(os.environ, GS_HIP_FAIR="1")
    r = run_program([sys.executable, "-c", code], cwd=ROOT, env=env, limit=300)
    assert r.returncode == 0, r.stdout + r.stderr


def tile_edge_shapes(tile_shape, fuse):
    """Grids one row and one column past a whole window's output, at the steps per launch the pinned form runs
    (gs_run: fuse_steps, else 8, or 4 for 16-row windows; 2K below the window's rows)."""
    rows = {1: 32, 2: 16, 3: 64}[tile_shape]
    k = min(fuse or (4 if rows == 16 else 8), rows // 2 - 1)
    return [(rows - 2 * k + 1, 64 - 2 * k + 1), (2 * (rows - 2 * k) + k, 2 * (64 - 2 * k) + k)]


@pytest.mark.parametrize("tile_shape", [1, 2, 3])
@pytest.mark.parametrize("fuse", [0, 1, 3, 8])
def test_tile_kernel_pinned(tile_shape, fuse):
    for shape, math in ([(s, capi.GS_MATH_STRICT) for s in PIN_SHAPES + [(1000, 1003)]]
                        + [(s, m) for s in tile_edge_shapes(tile_shape, fuse) for m in (capi.GS_MATH_STRICT, capi.GS_MATH_FUSED)]
                        + [(s, capi.GS_MATH_FUSED) for s in PIN_SHAPES + [(1000, 1003)]]):
        u0, v0 = stress_fields(shape, 4)
        ref_u, ref_v = neumann_ref.run(u0, v0, 19)
        try:
            got_u, got_v, info = gpu_run(u0, v0, 19, args=args(kernel=capi.GS_KERNEL_TILE, tile_shape=tile_shape, fuse_steps=fuse,
                                                                math=math))
        except GsError as e:  # (K = 8 does not fit the 16-row windows: refused for every rule)
            assert fuse == 8 and tile_shape == 2 and e.code == capi.GS_ERR_INVALID, e
            return
        assert info[0].startswith("tile") and info[0].endswith("/neumann"), info
        assert ("/fused" in info[0]) == (math == capi.GS_MATH_FUSED), info
        assert_bits_equal(got_u, ref_u, f"U {shape} {info[0]}")
        assert_bits_equal(got_v, ref_v, f"V {shape} {info[0]}")


SKEW = ((0.1, 0.3, 0.2), (0.6, 0.0, 0.4), (0.05, 0.25, 0.15))


@pytest.mark.parametrize("kernel", [capi.GS_KERNEL_AUTO, capi.GS_KERNEL_TB, capi.GS_KERNEL_STREAM])
def test_general_kernels_with_a_skew_stencil(kernel):
    """general_kernels = 1 and a stencil that is not symmetric: a site that mirrors the edge wrongly shows up."""
    p = Parameters(weights=SKEW, feed_rate=0.03, kill_rate=0.06, time_step=0.5)
    for shape in [(3, 5), (40, 37), (256, 512), (1080, 1920)]:
        u0, v0 = stress_fields(shape, 8)
        ref_u, ref_v = neumann_ref.run(u0, v0, 9, params=oracle_params(p))
        got_u, got_v, info = gpu_run(u0, v0, 9, params=p, args=args(kernel=kernel, general_kernels=1))
        assert ".op" not in info[0] and is_neumann(info[0]), info
        assert_bits_equal(got_u, ref_u, f"U {shape} {info[0]}")
        assert_bits_equal(got_v, ref_v, f"V {shape} {info[0]}")


# ---- fused math: bit for bit where no intermediate is sub-normal, within 1e-37 where one is ---------------------------
@pytest.mark.parametrize("shape", [(3, 5), (40, 37), (250, 130), (1080, 1920)])
def test_fused_flavour(shape):
    u0, v0 = stress_fields(shape, 1)
    ref_u, ref_v = neumann_ref.run(u0, v0, 20)
    got_u, got_v, info = gpu_run(u0, v0, 20, args=args(math=capi.GS_MATH_FUSED))
    assert "fused" in info[0] and is_neumann(info[0]), info
    assert_bits_equal(got_u, ref_u, f"fused U {shape}")
    assert_bits_equal(got_v, ref_v, f"fused V {shape}")
    u0, v0 = oracle.init_species(64, 128)
    ref_u, ref_v = neumann_ref.run(u0, v0, 100)
    got_u, got_v, _ = gpu_run(u0, v0, 100, args=args(math=capi.GS_MATH_FUSED))
    assert_bits_equal(got_u, ref_u, "fused U with a sub-normal V front")
    assert np.max(np.abs(got_v.astype(np.float64) - ref_v.astype(np.float64))) <= 1e-37


# ---- slab chains, row bands, processes -------------------------------------------------------------------------------
@pytest.mark.parametrize("devices,shape", [([0, 0], (300, 701)), ([0, 0], (7, 1003)), ([0, 0, 0], (9, 257)),
                                           ([0, 0, 0], (600, 1003)), ([0, 0, 0], (11, 40))])
@pytest.mark.parametrize("kernel", [capi.GS_KERNEL_AUTO, capi.GS_KERNEL_SIMPLE, capi.GS_KERNEL_STREAM])
def test_slab_chains(devices, shape, kernel):
    """Slabs of 2 to 300 rows: only the global edges clamp, seams read their ghost rows."""
    u0, v0 = stress_fields(shape, 12)
    for steps in (11, 1):
        ref_u, ref_v = neumann_ref.run(u0, v0, steps)
        got_u, got_v, info = gpu_run(u0, v0, steps, args=args(devices=devices, kernel=kernel))
        assert is_neumann(info[0]), info
        assert_bits_equal(got_u, ref_u, f"U {shape} {devices} {info[0]}")
        assert_bits_equal(got_v, ref_v, f"V {shape} {devices} {info[0]}")


@pytest.mark.parametrize("shape", [(300, 701), (1000, 1003)])
def test_row_bands(shape):
    u0, v0 = stress_fields(shape, 13)
    ref_u, ref_v = neumann_ref.run(u0, v0, 13)
    got_u, got_v, info = gpu_run(u0, v0, 13, args=args(split=2))
    assert is_neumann(info[0]), info
    assert_bits_equal(got_u, ref_u, f"U {shape} split 2 {info[0]}")
    assert_bits_equal(got_v, ref_v, f"V {shape} split 2 {info[0]}")


def _worker(rank, world, port, rows, cols, steps, out_dir, transport_lib, local_slabs):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", GS_RCCL_LIBRARY=transport_lib)
    import torch.distributed as dist

    from grayscott_amd import HipArgs, Parameters, Simulation
    from grayscott_amd import dist as gsd
    from tests.helpers import species_from_arrays, stress_fields

    info = gsd.bootstrap(backend="gloo", device="cpu")
    sim = Simulation.new(Parameters(), HipArgs(devices=[0] * local_slabs, rank=info.rank, world=info.world,
                                               unique_id=info.unique_id, boundary=3))
    r0 = gsd.slab_range(rows, world * local_slabs, rank * local_slabs)[0]
    r1 = gsd.slab_range(rows, world * local_slabs, (rank + 1) * local_slabs - 1)[1]
    u0, v0 = stress_fields((rows, cols), 21)
    species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(rows, cols))
    sim.perform_steps(species, steps)
    for _ in range(3):
        sim.perform_step(species)
    in_u, in_v, _, _ = species.in_out()
    u = gsd.gather_rows(in_u.make_scalar_view(sim.context), rank, world)
    v = gsd.gather_rows(in_v.make_scalar_view(sim.context), rank, world)
    if rank == 0:
        np.save(os.path.join(out_dir, "u.npy"), u)
        np.save(os.path.join(out_dir, "v.npy"), v)
        open(os.path.join(out_dir, "name"), "w").write(sim.context.info()[0])
    dist.barrier()
    sim.context.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,local_slabs,rows,cols,steps", [(2, 1, 300, 517, 14), (3, 1, 70, 260, 9),
                                                                (2, 2, 200, 300, 10), (3, 2, 60, 129, 7)])
def test_processes_over_the_shm_transport(tmp_path, built, shm_transport, world, local_slabs, rows, cols, steps):  # noqa: F811
    from tests.helpers import free_port

    spawn_ranks(_worker, (world, free_port(), rows, cols, steps, str(tmp_path), shm_transport, local_slabs), world)
    u0, v0 = stress_fields((rows, cols), 21)
    ref_u, ref_v = neumann_ref.run(u0, v0, steps + 3)
    assert is_neumann(open(tmp_path / "name").read())
    assert_bits_equal(np.load(tmp_path / "u.npy"), ref_u, f"U, {world} processes x {local_slabs} slabs")
    assert_bits_equal(np.load(tmp_path / "v.npy"), ref_v, f"V, {world} processes x {local_slabs} slabs")


# ---- conservation: the property of the rule, which every other rule breaks -------------------------------------------
@pytest.mark.parametrize("shape,kw", [((40, 37), {}), ((256, 512), {}), ((1080, 1920), {}), ((300, 701), dict(devices=[0, 0])),
                                      ((300, 701), dict(kernel=capi.GS_KERNEL_TB, cols_per_lane=2, fuse_steps=4))])
def test_u_plus_v_is_conserved_without_reaction(shape, kw):
    p = Parameters(feed_rate=0.0, kill_rate=0.0)
    u0, v0 = stress_fields(shape, 14)
    total = float(u0.astype(np.float64).sum() + v0.astype(np.float64).sum())

    def drift(boundary):
        gu, gv, info = gpu_run(u0, v0, 200, params=p, args=args(boundary=boundary, **kw))
        return abs(float(gu.astype(np.float64).sum() + gv.astype(np.float64).sum()) - total) / total, info[0]

    d, name = drift(N)
    assert d < 1e-6 and is_neumann(name), (d, name)
    for rule in (capi.GS_BOUNDARY_CLIPPED, capi.GS_BOUNDARY_ZERO_HALO):
        assert drift(rule)[0] > 20 * d, (rule, d)  # (edge losses shrink with the edge's share of the cells)


# ---- ensembles -------------------------------------------------------------------------------------------------------
PARAMS = [Parameters(),
          Parameters(feed_rate=0.030, kill_rate=0.060),
          Parameters(feed_rate=0.022, kill_rate=0.051, diffusion_rate_u=0.12, diffusion_rate_v=0.06),
          Parameters(feed_rate=0.018, kill_rate=0.049, diffusion_rate_v=0.03, time_step=2.0)]


@pytest.mark.parametrize("math", [capi.GS_MATH_STRICT, capi.GS_MATH_FUSED])
@pytest.mark.parametrize("shape,steps,form", [((16, 32), 37, "ensemble-resident"), ((1, 5), 9, "ensemble-resident"),
                                              ((37, 53), 37, "ensemble-tile"), ((100, 300), 21, "ensemble-tile")])
def test_ensemble_members_are_lone_species(shape, steps, form, math):
    pairs = [stress_fields(shape, 100 + i) for i in range(len(PARAMS))]
    u0, v0 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    sim = Simulation.new(PARAMS[0], args(math=math))
    ens = sim.make_ensemble(shape, PARAMS, seed=False)
    ens.upload(u0, v0)
    for n in (steps // 3, steps - steps // 3):
        ens.prepare_steps(n)
    u, v = ens.u_views(), ens.result_views()
    name = sim.context.info()[0]
    ens.destroy()
    sim.context.close()
    assert name.startswith(form) and name.endswith("/neumann"), name
    for i, p in enumerate(PARAMS):
        lu, lv, info = gpu_run(u0[i], v0[i], steps, params=p, args=args(math=math))
        assert_bits_equal(u[i], lu, f"U of member {i} ({name}) against a lone Species ({info[0]})")
        assert_bits_equal(v[i], lv, f"V of member {i} ({name}) against a lone Species ({info[0]})")
        if math == capi.GS_MATH_STRICT:
            ref_u, ref_v = neumann_ref.run(u0[i], v0[i], steps, params=oracle_params(p))
            assert_bits_equal(u[i], ref_u, f"U of member {i} ({name})")
            assert_bits_equal(v[i], ref_v, f"V of member {i} ({name})")


def test_resident_ensemble_takes_8192_cells():
    """The resident form's capacity is the zero-halo rule's: 8 cells per thread."""
    shape, members = (64, 120), 256
    rng = np.random.default_rng(9)
    u0 = rng.random((members,) + shape, dtype=np.float32)
    v0 = (rng.random((members,) + shape, dtype=np.float32) * np.float32(0.5)).astype(np.float32)
    sim = Simulation.new(Parameters(), args())
    ens = sim.make_ensemble(shape, [Parameters()] * members, seed=False)
    ens.upload(u0, v0)
    ens.prepare_steps(6)
    u, v = ens.u_views(), ens.result_views()
    name = sim.context.info()[0]
    ens.destroy()
    sim.context.close()
    assert name.startswith("ensemble-resident") and name.endswith("/neumann"), name
    for i in (0, 77, members - 1):
        ref_u, ref_v = neumann_ref.run(u0[i], v0[i], 6)
        assert_bits_equal(u[i], ref_u, f"U of member {i}")
        assert_bits_equal(v[i], ref_v, f"V of member {i}")


# ---- refusals and AUTO's choice where the window kernel would run ----------------------------------------------------
@pytest.mark.parametrize("kw,what", [(dict(kernel=capi.GS_KERNEL_WINDOW), "window"), (dict(kernel=capi.GS_KERNEL_LDS), "LDS-staged")])
def test_refusals(kw, what):
    with pytest.raises(GsError) as e:
        Simulation.new(Parameters(), args(**kw))
    assert e.value.code == capi.GS_ERR_UNSUPPORTED
    assert "Neumann" in str(e.value) and what in str(e.value), str(e.value)


def test_auto_takes_the_marching_kernel_where_the_window_kernel_would_run():
    u0, v0 = oracle.init_species(1080, 1920)
    sim = Simulation.new(Parameters(), args())
    species = species_from_arrays(sim, u0, v0)
    for _ in range(3):
        sim.perform_steps(species, 64)
    name = sim.context.info()[0]
    iu, iv, _, _ = species.in_out()
    got_v = iv.make_scalar_view(sim.context)
    sim.context.close()
    assert name.startswith("tb-") and is_neumann(name), name
    assert_bits_equal(got_v, neumann_ref.run(u0, v0, 192)[1], "V after 3 x 64 steps")


# ---- the drivers end to end ------------------------------------------------------------------------------------------
def test_simulate_end_to_end(tmp_path):
    out = tmp_path / "p.h5"
    r = run_program([sys.executable, "-m", "grayscott_amd.simulate", "--hip-boundary", "3", "-r", "64", "-c", "128",
                     "-n", "3", "-e", "32", "-o", str(out)], cwd=ROOT, limit=300)
    assert r.returncode == 0, r.stdout + r.stderr
    data = hdf5_min.read(str(out))
    assert data.shape == (3, 64, 128)
    u, v = oracle.init_species(64, 128)
    for i in range(3):
        u, v = neumann_ref.run(u, v, 32)
        assert_bits_equal(np.asarray(data[i]), v, f"image {i} (after {32 * (i + 1)} steps)")


def test_sweep_end_to_end(tmp_path):
    out = tmp_path / "s.h5"
    r = run_program([sys.executable, "-m", "grayscott_amd.sweep", "--feed", "0.02:0.03:2", "--kill", "0.05:0.06:2",
                     "-r", "24", "-c", "40", "-s", "30", "--hip-boundary", "3", "-o", str(out)],
                    cwd=ROOT, limit=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "/neumann" in r.stderr, r.stderr
    data = hdf5_min.read(str(out))
    assert data.shape == (4, 24, 40)
    u, v = oracle.init_species(24, 40)
    for i, (feed, kill) in enumerate([(0.02, 0.05), (0.03, 0.05), (0.02, 0.06), (0.03, 0.06)]):  # kill-major
        ref_v = neumann_ref.run(u, v, 30, params=oracle_params(Parameters(feed_rate=feed, kill_rate=kill)))[1]
        assert_bits_equal(np.asarray(data[i]), ref_v, f"member {i} (feed {feed}, kill {kill})")
