"""Component matches on the device (gs_fields_match, gs_members_match) against the scipy restatement of their rule
(tests/match_ref.py) on the same planes: both lists equal to tests/component_list_ref.py's, record for record, and every
overlap equal, in the same order, everywhere.  Exact equality throughout."""
import os
import re

import numpy as np
import pytest

from grayscott_amd import ComponentMatch, HipArgs, HipConcentration, Parameters, Simulation, capi
from tests import component_list_ref
from tests import components_ref
from tests import match_ref as ref
from tests.children import ROOT, build_program, rank_session, run_program, shm_transport, spawn_ranks  # noqa: F401
from tests.helpers import species_from_arrays, stress_fields
from tests.observe_cases import seam_rows

pytestmark = pytest.mark.gpu

T = components_ref.TILE_ROWS  # the labelling's tile height (kCompTileRows)
EVENT_NAMES = ("continued", "split", "merged", "born", "died")


def assert_match(got: ComponentMatch, want, what: str):
    """``want``: (before's records, after's records, overlaps) of ``ref.match``."""
    rb, ra, ov = want
    print(f"{what}: {got.before.count} / {got.after.count} records, {got.overlaps.shape[0]} overlaps; wanted {rb.shape[0]} / "
          f"{ra.shape[0]}, {ov.shape[0]}")
    assert got.before.records.dtype == got.after.records.dtype == component_list_ref.DTYPE and got.overlaps.dtype == ref.OVERLAP
    assert np.array_equal(got.before.records, rb), f"{what}: before {got.before.records[:4]} ..., not {rb[:4]} ..."
    assert np.array_equal(got.after.records, ra), f"{what}: after {got.after.records[:4]} ..., not {ra[:4]} ..."
    assert np.array_equal(got.overlaps, ov), f"{what}: overlaps {got.overlaps[:6]} ..., not {ov[:6]} ..."
    assert got.counts() == ref.events(rb, ra, ov), what


def same_match(a: ComponentMatch, b: ComponentMatch) -> bool:
    return (np.array_equal(a.before.records, b.before.records) and np.array_equal(a.after.records, b.after.records) and
            np.array_equal(a.overlaps, b.overlaps))


def upload_pair(ctx, shape, before, after):
    fb, fa = HipConcentration(ctx, shape), HipConcentration(ctx, shape)
    fb.upload(ctx, before)
    fa.upload(ctx, after)
    return fb, fa


# ---- planted pairs of planes -------------------------------------------------------------------------------------------------

COLUMN_SHAPES = [(1, 1), (2, 3), (5, 253), (3, 255), (4, 256), (3, 257), (2, 1023), (6, 1025)]
ROW_SHAPES = [(T - 1, 300), (T, 300), (T + 1, 300), (2 * T + 1, 300)]


@pytest.mark.parametrize("shape", COLUMN_SHAPES + ROW_SHAPES)
def test_pairs_of_planes(built, shape):
    """Every kind of tests/match_ref.py's generator (tests/test_match_cpu.py shows that the kinds hold every event, and pairs
    made of two pieces, over these shapes), both connectivities, min_size 1 and 3."""
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    fb, fa = HipConcentration(sim.context, shape), HipConcentration(sim.context, shape)
    for kind in ref.KINDS:
        before, after = ref.pair_of_planes(shape, 1, kind)
        fb.upload(sim.context, before)
        fa.upload(sim.context, after)
        for conn in (4, 8):
            for min_size in (1, 3):
                got = fa.match(sim.context, fb, ref.THRESHOLD, True, conn, min_size)
                assert (got.after.rows, got.after.cols, got.after.connectivity, got.after.min_size) == shape + (conn, min_size)
                assert_match(got, ref.match(before, after, ref.THRESHOLD, True, conn, min_size), f"{kind}, {conn}, min_size {min_size}")
                if min_size == 1:
                    both = (before > np.float32(ref.THRESHOLD)) & (after > np.float32(ref.THRESHOLD))
                    assert int(got.overlaps["cells"].sum()) == int(both.sum())
        below = fa.match(sim.context, fb, ref.THRESHOLD, False, 8, 1)   # the other sense: NaN, -inf and the threshold itself
        assert_match(below, ref.match(before, after, ref.THRESHOLD, False, 8, 1), f"{kind}, below")
    sim.context.close()


def test_special_planes(built):
    shape = rows, cols = (2 * T + 1, 513)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ctx = sim.context
    ones, zeros = np.ones(shape, np.float32), np.zeros(shape, np.float32)
    noise, _ = ref.pair_of_planes(shape, 3, "noise")
    full, other = upload_pair(ctx, shape, ones, ones)
    for conn in (4, 8):
        m = other.match(ctx, full, 0.5, True, conn)             # one component against one: a piece over many tiles
        assert_match(m, ref.match(ones, ones, 0.5, True, conn), "all set")
        assert [tuple(int(x) for x in o) for o in m.overlaps] == [(0, 0, rows * cols)]
        assert m.counts() == {"continued": 1, "split": 0, "merged": 0, "born": 0, "died": 0}
        assert np.array_equal(m.displacements(), [[0.0, 0.0]])
        assert m.before.count == 1 and int(m.before.sizes[0]) == rows * cols
    other.upload(ctx, noise)
    for conn in (4, 8):
        for min_size in (1, 3):
            want = ref.match(ones, noise, 0.5, True, conn, min_size)
            m = other.match(ctx, full, 0.5, True, conn, min_size)   # everything the full plane's one component overlaps
            assert_match(m, want, "all set against noise")
            assert m.counts()["split"] == 1 and list(m.children(0)) == list(range(m.after.count))
            assert_match(full.match(ctx, other, 0.5, True, conn, min_size), ref.match(noise, ones, 0.5, True, conn, min_size),
                         "noise against all set")
            same = other.match(ctx, other, 0.5, True, conn, min_size)   # the same handle twice: (i, i, size_i)
            assert_match(same, ref.match(noise, noise, 0.5, True, conn, min_size), "the same handle")
            n = same.before.count
            assert n > 1 and np.array_equal(same.overlaps["before"], np.arange(n)) and np.array_equal(same.overlaps["after"], np.arange(n))
            assert np.array_equal(same.overlaps["cells"], same.before.sizes)
    full.upload(ctx, zeros)
    for conn in (4, 8):
        m = other.match(ctx, full, 0.5, True, conn)             # empty against anything
        assert_match(m, ref.match(zeros, noise, 0.5, True, conn), "empty against noise")
        assert m.before.count == 0 and m.overlaps.shape == (0,) and m.counts()["born"] == m.after.count > 0
        m = full.match(ctx, other, 0.5, True, conn)
        assert m.after.count == 0 and m.overlaps.shape == (0,) and m.counts()["died"] == m.before.count > 0
        m = full.match(ctx, full, 0.5, True, conn)
        assert m.before.count == m.after.count == 0 and m.overlaps.shape == (0,) and m.overlaps.dtype == ref.OVERLAP
    for empty_shape in ((0, 16), (7, 0)):
        a, b = HipConcentration(ctx, empty_shape), HipConcentration(ctx, empty_shape)
        m = a.match(ctx, b, 0.1)
        assert m.before.count == m.after.count == 0 and m.overlaps.shape == (0,)
        assert m.counts() == dict.fromkeys(EVENT_NAMES, 0)
    ctx.close()


# ---- slab layouts ----------------------------------------------------------------------------------------------------------------

def layout_pairs(shape):
    """Pairs of planes for chains of two and of three slabs (the seams of both): generated kinds with busy seam rows; a U against two bars through its
    arms on both sides of every seam -- pieces cut by the seam --; the U against a Z that meets one arm above the seam and
    the other below it -- ONE overlap whose two pieces lie in different slabs --; a column against itself -- one piece cut by
    every seam, each slab's part smaller than min_size = rows --; and the column against the U."""
    rows, cols = shape
    rng = np.random.default_rng(13)
    seams = sorted(set(seam_rows(rows, 2)) | set(seam_rows(rows, 3)))
    out = {}
    for kind in ("noise", "flip"):
        before, after = ref.pair_of_planes(shape, 5, kind)
        for seam in seams:
            for r in (seam - 1, seam):
                before[r] = np.where(rng.random(cols) < 0.6, np.float32(0.9), np.float32(0.1))
                after[r] = np.where(rng.random(cols) < 0.6, np.float32(0.9), np.float32(0.1))
        out[kind] = (before, after)
    column = components_ref.column(shape)
    out["column"] = (column, column)
    for seam in seams:
        u = components_ref.u_shape(shape, seam)
        bars = np.zeros(shape, np.float32)
        bars[seam - 1] = bars[seam] = 1
        bars[seam - 1, cols // 2] = bars[seam, cols // 2] = 0    # (two bars, left and right: each meets one arm, across the seam)
        z = np.zeros(shape, np.float32)                          # one component: it meets one arm above the seam, one below
        z[seam - 1, : cols // 2 + 1] = z[seam, cols // 2:] = 1
        out[f"u against bars at {seam}"] = (u, bars)
        out[f"u against z at {seam}"] = (u, z)
        out[f"column against u at {seam}"] = (column, u)
    return out


@pytest.mark.parametrize("shape", [(5, 300), (7, 257), (2 * T + 1, 300), (50, 513)])
def test_matches_do_not_depend_on_the_slab_layout(built, shape):
    rows, cols = shape
    wanted, alone = {}, {}
    for slabs in (1, 2, 3):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0] * slabs))
        fb, fa = HipConcentration(sim.context, shape), HipConcentration(sim.context, shape)
        stats = sim.context.stats()
        for what, (before, after) in layout_pairs(shape).items():
            fb.upload(sim.context, before)
            fa.upload(sim.context, after)
            for conn in (4, 8):
                for min_size in (1, 3, rows):
                    key = (what, conn, min_size)
                    if key not in wanted:
                        wanted[key] = ref.match(before, after, 0.5, True, conn, min_size)
                    got = fa.match(sim.context, fb, 0.5, True, conn, min_size)
                    assert_match(got, wanted[key], f"{what}, {slabs} slabs, connectivity {conn}, min_size {min_size}")
                    if slabs == 1:
                        alone[key] = got
                    assert same_match(got, alone[key]), key
                    if what == "column":                      # every slab's part is below min_size = rows, the whole is not
                        assert [tuple(int(x) for x in o) for o in got.overlaps] == [(0, 0, rows)], key
        assert sim.context.stats() == stats
        sim.context.close()
    for what, (b, a) in layout_pairs(shape).items():
        if what.startswith("u against z"):
            assert [int(n) for n in ref.pieces(b, a, 0.5, True, 4)] == [2], "one overlap, a piece on either side of the seam"


# ---- ensembles -------------------------------------------------------------------------------------------------------------------

def member_planes(members, shape, seed):
    """[members, rows, cols] before and after: every kind in turn; member i's last row and member i + 1's first row fully set in
    both -- they stay separate components --; member 3 has nothing set afterwards."""
    before = np.zeros((members,) + shape, np.float32)
    after = np.zeros((members,) + shape, np.float32)
    for i in range(members):
        before[i], after[i] = ref.pair_of_planes(shape, seed + i, ref.KINDS[i % len(ref.KINDS)])
        for j, r in ((i, shape[0] - 1), (i + 1, 0)):
            if j < members:
                before[j, r] = after[j, r] = np.float32(0.75)
    if members > 3:
        after[3] = np.float32(0.125)
    return before, after


@pytest.mark.parametrize("members,shape", [(1, (16, 32)), (5, (16, 32)), (5, (64, 128))])
def test_ensemble_members_equal_lone_pairs_of_fields(built, members, shape):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ens = sim.make_ensemble(shape, Parameters(), members=members)
    before, after = member_planes(members, shape, 20)
    ens.upload(None, before)
    snap = ens.snapshot()
    ens.upload(None, after)
    fb, fa = HipConcentration(sim.context, shape), HipConcentration(sim.context, shape)
    for conn, min_size in ((8, 1), (4, 1), (8, 3)):
        got = ens.matches_since(snap, threshold=0.5, connectivity=conn, min_size=min_size)
        assert len(got) == members
        for i in range(members):
            assert_match(got[i], ref.match(before[i], after[i], 0.5, True, conn, min_size), f"member {i}")
            fb.upload(sim.context, before[i])
            fa.upload(sim.context, after[i])
            assert same_match(fa.match(sim.context, fb, 0.5, True, conn, min_size), got[i]), f"member {i} as a pair of fields"
            if i == 3:
                assert got[i].after.count == 0 and got[i].overlaps.shape == (0,)
        lists = ens.component_lists(threshold=0.5, connectivity=conn, min_size=min_size)
        for i in range(members):
            assert np.array_equal(lists[i].records, got[i].after.records)
        if members > 2:                                     # a range that does not start at 0, across the empty member
            part = ens.matches_since(snap, 2, members - 2, threshold=0.5, connectivity=conn, min_size=min_size)
            assert len(part) == members - 2
            for i, m in enumerate(part):
                assert same_match(m, got[2 + i]), f"member {2 + i} of a range"
        same = ens.matches_since(ens, threshold=0.5, connectivity=conn, min_size=min_size)   # the same ensemble twice
        for i in range(members):
            assert_match(same[i], ref.match(after[i], after[i], 0.5, True, conn, min_size), f"member {i} against itself")
    below = ens.matches_since(snap, species="u", threshold=0.5, above=False)   # U: as seeded, the same in both
    u = ens.u_views()
    for i in range(members):
        assert_match(below[i], ref.match(u[i], u[i], 0.5, False, 8, 1), f"member {i} U")
    snap.destroy()
    ens.destroy()
    sim.context.close()


def test_first_and_last_member_of_a_batch_with_an_empty_list(built):
    """Three members of (16, 32) in one batch: member 0 has nothing set before, member 2 nothing set afterwards, so the batch's
    first plane has no before-record and its last no after-record, and the records and pieces of the planes between must
    still land in their own planes.  Ranges of one such member are batches whose before-list (after-list) is empty as a
    whole: nothing is listed and no record memory is asked for.  All against the three lone pairs of fields."""
    members, shape = 3, (16, 32)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ens = sim.make_ensemble(shape, Parameters(), members=members)
    before, after = member_planes(members, shape, 40)
    before[0] = np.float32(0.125)
    after[2] = np.float32(0.125)
    ens.upload(None, before)
    snap = ens.snapshot()
    ens.upload(None, after)
    fb, fa = HipConcentration(sim.context, shape), HipConcentration(sim.context, shape)
    for conn, min_size in ((8, 1), (4, 3)):
        got = ens.matches_since(snap, threshold=0.5, connectivity=conn, min_size=min_size)
        assert len(got) == members
        assert got[0].before.count == 0 and got[0].after.count > 0 and got[0].overlaps.shape == (0,)
        assert got[2].after.count == 0 and got[2].before.count > 0 and got[2].overlaps.shape == (0,)
        assert got[1].overlaps.shape[0] > 0
        for i in range(members):
            assert_match(got[i], ref.match(before[i], after[i], 0.5, True, conn, min_size), f"member {i}")
            fb.upload(sim.context, before[i])
            fa.upload(sim.context, after[i])
            lone = fa.match(sim.context, fb, 0.5, True, conn, min_size)
            assert same_match(lone, got[i]), f"member {i} as a pair of fields"
            one = ens.matches_since(snap, i, 1, threshold=0.5, connectivity=conn, min_size=min_size)
            assert len(one) == 1 and same_match(one[0], lone), f"member {i} as a batch of its own"
    snap.destroy()
    ens.destroy()
    sim.context.close()


def test_more_members_than_one_batch(built):
    """One member more than fit GS_COMPONENTS_BATCH_BYTES of label memory (8 bytes per cell and labelling): the last member is
    a batch of its own, and the offsets of the lists and of the overlaps run through."""
    header = open(os.path.join(ROOT, "include", "gs_hip.h")).read()
    m = re.search(r"#define GS_COMPONENTS_BATCH_BYTES \((\d+)u << (\d+)\)", header)
    shape = (64, 128)
    batch = (int(m.group(1)) << int(m.group(2))) // 8 // (shape[0] * shape[1])
    members = batch + 1
    assert members * shape[0] * shape[1] * 16 < 2 ** 30, "four planes of an ensemble: a second's worth of memory traffic"
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ens = sim.make_ensemble(shape, Parameters(), members=members)
    rng = np.random.default_rng(5)
    before = (rng.random((members,) + shape, dtype=np.float32) < np.float32(0.3)).astype(np.float32)
    after = before.copy()
    flip = rng.random((members,) + shape, dtype=np.float32) < np.float32(0.05)
    after[flip] = np.float32(1) - after[flip]
    before[7] = 0                                             # an empty member inside the first batch
    after[9] = 0
    ens.upload(None, before)
    snap = ens.snapshot()
    ens.upload(None, after)
    got = ens.matches_since(snap, threshold=0.5, min_size=4)
    assert len(got) == members and got[7].before.count == 0 and got[9].after.count == 0
    assert got[7].overlaps.shape == got[9].overlaps.shape == (0,)
    for i in (0, 7, 8, 9, batch - 1, batch):
        assert_match(got[i], ref.match(before[i], after[i], 0.5, True, 8, 4), f"member {i} of {members}")
    assert got[batch].overlaps.shape[0] > 0 and got[batch - 1].overlaps.shape[0] > 0
    tail = ens.matches_since(snap, batch - 1, 2, threshold=0.5, min_size=4)
    assert same_match(tail[0], got[batch - 1]) and same_match(tail[1], got[batch])
    snap.destroy()
    ens.destroy()
    sim.context.close()


def test_a_retired_member_is_matched_in_its_held_state(built):
    members, shape = 5, (45, 61)
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    ens = sim.make_ensemble(shape, Parameters(), members=members)
    rng = np.random.default_rng(3)
    ens.upload(rng.random((members,) + shape, dtype=np.float32),
               (rng.random((members,) + shape, dtype=np.float32) * np.float32(0.5)).astype(np.float32))
    ens.perform_steps(7)
    snap = ens.snapshot()
    v0 = ens.result_views()
    ens.retire([1, 3])
    for steps in (3, 4):                     # an odd and an even number of further runs' steps: both slots are in play
        ens.perform_steps(steps)
        got = ens.matches_since(snap, threshold=0.1)
        v = ens.result_views()
        for i in range(members):
            assert_match(got[i], ref.match(v0[i], v[i], 0.1, True, 8), f"member {i} after {steps} more steps")
        for i in (1, 3):                     # held: every component continues as itself
            n = got[i].before.count
            assert v[i].tobytes() == v0[i].tobytes() and n > 0
            assert np.array_equal(got[i].overlaps["before"], np.arange(n)) and np.array_equal(got[i].overlaps["cells"], got[i].before.sizes)
    snap.destroy()
    ens.destroy()
    sim.context.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------

def test_match_since_after_real_kernels_and_without_side_effects(built):
    """A snapshot, 200 steps, a match -- under the default kernel and under GS_KERNEL_SIMPLE: the same match, equal to the
    reference on the downloaded planes -- and then 50 more steps, bit for bit those of a run that never looked."""
    shape = (200, 333)
    u0, v0 = stress_fields(shape, 9)
    matches, ends = [], []
    for look, kernel in ((True, capi.GS_KERNEL_AUTO), (True, capi.GS_KERNEL_SIMPLE), (False, capi.GS_KERNEL_AUTO)):
        sim = Simulation.new(Parameters(), HipArgs(devices=[0], kernel=kernel))
        species = species_from_arrays(sim, u0, v0)
        snap = species.snapshot() if look else None
        before = v0
        sim.perform_steps(species, 200)
        if look:
            after = species.make_result_view()
            t = float(np.median(after))
            sim.context.sync()
            state = (sim.context.stats(), sim.context.info())
            for conn, min_size in ((8, 1), (4, 2)):
                got = species.match_since(snap, t, "v", True, conn, min_size)
                want = ref.match(before, after, t, True, conn, min_size)
                assert_match(got, want, f"kernel {kernel} ({sim.context.info()[0]}), connectivity {conn}, min_size {min_size}")
                assert want[2].shape[0] >= 1 and 0 < int(want[1]["size"].sum()) < after.size, "a pattern, not a full or empty plane"
                matches.append(got)
            u_match = species.match_since(snap, 0.5, "u", False)
            in_u = species.in_out()[0].make_scalar_view(sim.context)
            assert np.array_equal(u_match.after.records, component_list_ref.records(in_u, 0.5, False, 8))
            assert (sim.context.stats(), sim.context.info()) == state
        sim.perform_steps(species, 50)
        in_u, in_v, _, _ = species.in_out()
        ends.append((in_u.make_scalar_view(sim.context), in_v.make_scalar_view(sim.context)))
        sim.context.close()
    assert same_match(matches[0], matches[2]) and same_match(matches[1], matches[3])      # default against simple
    for k in (1, 2):
        assert ends[0][0].tobytes() == ends[k][0].tobytes() and ends[0][1].tobytes() == ends[k][1].tobytes(), k


# ---- refusals that need handles ---------------------------------------------------------------------------------------------------

def test_refusals_that_need_handles(built):
    sim = Simulation.new(Parameters(), HipArgs(devices=[0]))
    other = Simulation.new(Parameters(), HipArgs(devices=[0]))
    a, b = HipConcentration(sim.context, (8, 16)), HipConcentration(sim.context, (8, 16))
    foreign, wide = HipConcentration(other.context, (8, 16)), HipConcentration(sim.context, (8, 17))
    for before, after in ((foreign, a), (a, foreign), (wide, a), (a, wide)):
        with pytest.raises(capi.GsError) as e:
            after.match(sim.context, before, 0.5)
        assert e.value.code == capi.GS_ERR_INVALID
    for kwargs in ({"threshold": float("nan")}, {"threshold": 0.5, "connectivity": 6}, {"threshold": 0.5, "min_size": 0}):
        with pytest.raises(capi.GsError) as e:
            a.match(sim.context, b, **kwargs)
        assert e.value.code == capi.GS_ERR_INVALID, kwargs
    ens = sim.make_ensemble((8, 16), Parameters(), members=3)
    snap = ens.snapshot()
    for first, count in ((3, 1), (2, 2), (0, 4)):
        with pytest.raises(capi.GsError) as e:
            ens.matches_since(snap, first, count)
        assert e.value.code == capi.GS_ERR_INVALID, (first, count)
    for theirs in (other.make_ensemble((8, 16), Parameters(), members=3), sim.make_ensemble((8, 16), Parameters(), members=4),
                   sim.make_ensemble((8, 17), Parameters(), members=3)):
        for pair in ((theirs, ens), (ens, theirs)):
            h = capi.ctypes.c_void_p()
            assert sim.context._lib.gs_members_match(sim.context.handle, pair[0].handle, pair[1].handle, 0, 1, 1, 0.5, 1, 8, 1,
                                                     capi.ctypes.byref(h)) == capi.GS_ERR_INVALID and not h
    with pytest.raises(ValueError):
        ens.matches_since(snap, species="w")
    assert len(ens.matches_since(snap)) == 3                  # the context goes on working
    for s in (sim, other):
        s.context.close()


# ---- the sweep driver --------------------------------------------------------------------------------------------------------------

def test_sweep_records_tracks_without_changing_the_fields(built, tmp_path):
    from grayscott_amd import hdf5_min, sweep

    base = ["--feed", "0.02:0.05:3", "--kill", "0.05:0.062:2", "-r", "48", "-c", "72", "-s", "30"]
    track = ["--track-threshold-v", "0.1", "--track-min-size", "2", "--track-connectivity", "4"]
    spots = ["--spots-every", "10", "--spot-threshold-v", "0.1", "--spot-min-size", "2", "--spot-connectivity", "4"]
    sweep.main(base + ["-o", str(tmp_path / "plain.h5")])
    sweep.main(base + ["--track-every", "10"] + track + spots + ["-o", str(tmp_path / "tracks.h5")])
    assert (tmp_path / "plain.h5").read_bytes() == (tmp_path / "tracks.h5").read_bytes()
    assert not (tmp_path / "plain.tracks.npz").exists()
    z, s = np.load(tmp_path / "tracks.tracks.npz"), np.load(tmp_path / "tracks.spots.npz")
    assert list(z["steps"]) == [10, 20, 30] and int(z["connectivity"]) == 4 and int(z["min_size"]) == 2
    assert float(z["threshold"]) == float(np.float32(0.1))
    assert z["offsets"].shape == (3 * 6 + 1,) and z["overlaps"].dtype == ref.OVERLAP and int(z["offsets"][-1]) == z["overlaps"].shape[0]
    for name in EVENT_NAMES:
        assert z[name].shape == (3, 6) and z[name].dtype == np.int64
    assert z["displacement_offsets"].shape == (19,) and z["displacements"].shape == (int(z["displacement_offsets"][-1]), 2)
    # sample 2 against sample 1: the overlaps index the spot lists taken at the same steps with the same rule
    found = 0
    for i in range(6):
        rec_b = s["records"][s["offsets"][6 + i]:s["offsets"][6 + i + 1]]
        rec_a = s["records"][s["offsets"][12 + i]:s["offsets"][12 + i + 1]]
        ov = z["overlaps"][z["offsets"][12 + i]:z["offsets"][12 + i + 1]]
        assert ref.events(rec_b, rec_a, ov) == {name: int(z[name][2, i]) for name in EVENT_NAMES}, i
        assert np.all(ov["before"] < max(len(rec_b), 1)) and np.all(ov["after"] < max(len(rec_a), 1))
        found += ov.shape[0]
    assert found > 0, "a sweep with nothing to match checks nothing"
    v = hdf5_min.read(str(tmp_path / "tracks.h5"))
    for i in range(6):
        rec_a = s["records"][s["offsets"][12 + i]:s["offsets"][12 + i + 1]]
        assert np.array_equal(rec_a, component_list_ref.records(v[i], 0.1, True, 4, 2)), i


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------------

def test_cpp_mirror_matches(built, tmp_path):
    exe = build_program("match_mirror", tmp_path)
    members, rows, cols = 4, 72, 200
    out = tmp_path / "o.bin"
    r = run_program([str(exe), str(members), str(rows), str(cols), "300", str(out)])
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    matches, at = [], 0
    for _ in range(2 + members):
        nb, na, no = (int(x) for x in np.frombuffer(raw, np.uint64, 3, at))
        at += 24
        rb = np.frombuffer(raw, component_list_ref.DTYPE, nb, at)
        ra = np.frombuffer(raw, component_list_ref.DTYPE, na, at + 48 * nb)
        ov = np.frombuffer(raw, ref.OVERLAP, no, at + 48 * (nb + na))
        at += 48 * (nb + na) + 16 * no
        matches.append((rb, ra, ov))
    planes = np.frombuffer(raw[at:], np.float32).reshape(2, rows, cols)
    for got, want in ((matches[0], ref.match(planes[0], planes[1], 0.25, True, 8)),
                      (matches[1], ref.match(planes[0], planes[1], 0.1, True, 4, 3))):
        for k in range(3):
            assert np.array_equal(got[k], want[k]), k
    assert matches[1][2].shape[0] > 0
    for i in range(members):
        for k in range(3):
            assert np.array_equal(matches[2 + i][k], matches[0][k]), (i, k)


# ---- a multi-process context -----------------------------------------------------------------------------------------------------------

def _worker(rank, world, port, rows, cols, out_dir, transport_lib):
    from grayscott_amd import capi
    from tests.helpers import species_from_arrays

    with rank_session(rank, world, port, transport_lib, rows) as (sim, (r0, r1)):
        u0, v0 = stress_fields((rows, cols), 4)
        species = species_from_arrays(sim, u0[r0:r1], v0[r0:r1], shape=(rows, cols))
        snap = species.snapshot()
        codes = []
        for call in (lambda: species.match_since(snap, 0.25), lambda: species.in_out()[0].match(sim.context, snap.u, 0.5, False, 4, 2)):
            try:
                call()
                codes.append(0)
            except capi.GsError as e:
                codes.append(e.code)
        sim.perform_steps(species, 3)                               # the context goes on working, on every rank
        np.save(os.path.join(out_dir, f"refused{rank}.npy"), np.array(codes))


def test_a_two_process_context_is_refused_on_both_ranks(tmp_path, built, shm_transport):
    from tests.helpers import free_port

    spawn_ranks(_worker, (2, free_port(), 50, 333, str(tmp_path), shm_transport), 2)
    for rank in range(2):
        codes = list(np.load(tmp_path / f"refused{rank}.npy"))
        assert codes == [capi.GS_ERR_UNSUPPORTED] * 2, (rank, codes)
