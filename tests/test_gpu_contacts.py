"""Device-side contact lifetime correlations (include/vvhip.h: vvhip_contacts_*) on the GPU.  The ground truth needs no second trajectory:
the same context also runs the frame recorder (float64) at the same interval, and the expected table is tests/contacts_reference.py over
those frames, each with its own box.  Every comparison is np.array_equal on int64 words.  Groups hold a few hundred sites and a case takes
about a dozen samples, so the NumPy reference stays well within a second per case."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contacts_reference as CR      # noqa: E402
import test_gpu_rdf as TR            # noqa: E402  (the small systems and the helpers)

pkg = importlib.import_module("openmm-velocityverlet_amd")
S, I = pkg.systems, pkg.integrator
H = I.H

pytestmark = pytest.mark.gpu

spec_for, integrator_for, make, two_groups, state, same_bits, eq = TR.spec_for, TR.integrator_for, TR.make, TR.two_groups, TR.state, TR.same_bits, TR.eq
CLASSES = [(0, 1), (0, 0), (1, 0)]


def expected(frames, which, groups, classes, r_cut, num_lags, every, mol_id=None, continuous=True, max_samples=1 << 62):
    """(table, samples, dropped, invalid) of the reference over the frames `which` as samples 0, 1, ..., each with the box its step ran with."""
    which = list(which)
    assert frames.positions.dtype == np.float64 and eq(frames.particles, np.arange(len(frames.particles), dtype=np.int32))
    return CR.contacts_reference(frames.positions[which], frames.box[which], groups, classes, r_cut, num_lags, every, mol_id, continuous, max_samples)


def assert_equal(con, want, what=None):
    table, samples, dropped, invalid = want
    assert con.words.dtype == np.int64 and con.words.shape == table.shape and np.array_equal(con.words, table), what
    assert (con.samples, con.invalid) == (samples, invalid), what


def cutoff_from(frames, groups, ceiling=0.6):
    """A cutoff in the middle of the largest separation gained between the first and the last frame by a (0, 1) pair that ends below
    `ceiling`: that pair is a contact at the first origin and none at the last sample."""
    ia, ib = CR.sites(groups, len(groups), 0), CR.sites(groups, len(groups), 1)
    r0 = np.sqrt(CR.r2_matrix(frames.positions[0][ia], frames.positions[0][ib], frames.box[0]))
    r1 = np.sqrt(CR.r2_matrix(frames.positions[-1][ia], frames.positions[-1][ib], frames.box[-1]))
    gain = np.where(r1 < ceiling, r1 - r0, -np.inf)
    i, j = np.unravel_index(int(np.argmax(gain)), gain.shape)
    assert gain[i, j] > 0
    return float(0.5 * (r0[i, j] + r1[i, j]))


# ------------------------------------------------------------------------------------------ 1. the table equals the reference over the frames
CASES = [("C3", "mixed", True), ("C3", "single", True), ("C3", "double", True), ("C3", "mixed", False)]


@pytest.mark.parametrize("cfg,precision,middle", CASES, ids=[f"{c}-{p}-{'middle' if m else 'classic'}" for c, p, m in CASES])
def test_table_equals_the_reference_over_the_frames(cfg, precision, middle):
    """A scout context records 8 frames; the cutoff is taken from them; the recording context runs the same steps (the same trajectory bit
    for bit) with the recorder and frames of its own, and its table is held to the reference over THOSE frames -- 6 lags, every other sample
    an origin, three classes, with and without the exclusion; a context without a recorder runs the same steps."""
    spec = spec_for(cfg)
    groups, mol = two_groups(spec.num_atoms, most=300), np.asarray(spec.mol_id)
    (_, scout), (_, rec), (_, plain) = make(cfg, spec, precision, middle), make(cfg, spec, precision, middle), make(cfg, spec, precision, middle)
    try:
        scout.frames_start(10, capacity=8, float64=True)
        scout.run_graph(80, 40)
        cut = cutoff_from(scout.frames_read(), groups)
        cuts = [cut, cut, 0.9 * cut]
        rec.frames_start(10, capacity=16, float64=True)
        for k, exclude in enumerate([False, True]):
            rec.contacts_start(10, 6, CLASSES, cuts, origin_every=2, groups=groups, exclude_same_molecule=exclude, max_samples=100)
            lay = rec.contacts_info()
            n0, n1 = int(np.count_nonzero(groups == 0)), int(np.count_nonzero(groups == 1))
            assert (lay.active, lay.num_classes, lay.num_origins, lay.words, lay.start_step) == (1, 3, 3, 3 * 6 * 4, 80 * k)
            assert list(lay.rows[:3]) == [n0, n0, n1] and list(lay.cols[:3]) == [n1, n0, n0]
            rec.run_graph(80, 40)
            con, f = rec.contacts_read(), rec.frames_read()
            assert list(f.step[8 * k:]) == list(range(80 * k + 10, 80 * k + 81, 10))
            want = expected(f, range(8 * k, 8 * k + 8), groups, CLASSES, cuts, 6, 2, mol if exclude else None)
            # a table of zeros must not pass: the reference has contacts at the origins, and some of them are gone at a later sample
            assert want[0][0, 0, 1] > 0 and np.any(want[0][:, :, 2] < want[0][:, :, 1]), want[0][0]
            assert (con.samples, con.dropped, con.invalid) == (8, 0, 0)
            assert_equal(con, want, exclude)
            assert list(con.origins) == [4, 4, 3, 3, 2, 2] and con.mean_contacts(0) > 0
            assert np.all(con.words[..., 3] <= con.words[..., 2]) and np.all(con.words[..., 2] <= con.words[..., 1])
        plain.run_graph(160, 40)
        assert same_bits(state(rec), state(plain))                    # the recorder changes nothing of the run
    finally:
        for c in (scout, rec, plain):
            c.close()


# ------------------------------------------------------------------------------------------ 2. a hand-made sequence
def test_hand_made_sequence():
    """Three pairs of class (0, 1), cutoff 0.5 nm, far from each other: one breaks and re-forms (the intermittent correlation recovers,
    the continuous one does not), one sits exactly AT the cutoff (no contact), one sits 0.25 nm apart across three periodic images."""
    spec = spec_for("C1")
    n = spec.num_atoms
    it, ctx = make("C1", spec, precision="double")
    try:
        box = np.array([4.0, 5.0, 6.0])
        ctx.setPeriodicBoxSize(*box)
        posq = ctx.getPosq()
        assert posq.dtype == np.float64
        groups = np.full(n, -1, dtype=np.int8)
        groups[:6] = np.arange(6) % 2
        hand = posq.copy()
        for k in range(3):
            hand[2 * k, :3] = hand[2 * k + 1, :3] = [1.0, 1.0, 0.5 + 2.0 * k]
        hand[3, 0] += 0.5                                              # exactly at the cutoff: 1.5 - 1.0 and 0.5 * 0.5 are exact
        hand[5, :3] += [0.25 + 3 * 4.0, -2 * 5.0, 6.0]                 # 0.25 apart, three images away
        ctx.contacts_start(1000, 3, [(0, 1)], [0.5], groups=groups)
        frames = []
        for gap in (0.3, 0.7, 0.3):
            hand[1, 0] = 1.0 + gap
            ctx.posq.upload(hand)
            ctx.contacts_sample()
            frames.append(hand[:, :3].copy())
        con = ctx.contacts_read()
        want = np.array([[[3, 5, 5, 5], [2, 3, 2, 2], [1, 2, 2, 1]]], dtype=np.int64)
        assert (con.samples, con.dropped, con.invalid) == (3, 0, 0) and np.array_equal(con.words, want)
        assert np.array_equal(CR.contacts_reference(frames, [box] * 3, groups, [(0, 1)], [0.5], 3, 1)[0], want)
        assert con.intermittent(0)[2] == 1.0 and con.continuous(0)[2] == 0.5
        # one ulp above the cutoff the pair at 0.5 nm is a contact; a NaN site is none and counts once per pair it is in
        hand[4, 0] = np.nan
        ctx.posq.upload(hand)
        ctx.contacts_start(1000, 1, [(0, 1), (1, 0)], [np.nextafter(0.5, 1.0), 0.5], groups=groups)
        ctx.contacts_sample()
        con = ctx.contacts_read()
        assert (con.samples, con.invalid) == (1, 6) and list(con.words[0, 0]) == [1, 2, 2, 2] and list(con.words[1, 0]) == [1, 1, 1, 1]
        assert CR.contacts_reference([hand[:, :3]], [box], groups, [(0, 1), (1, 0)], [np.nextafter(0.5, 1.0), 0.5], 1, 1)[3] == 6
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 3. edge shapes under every hook
TUNES = [None, {"contacts_rows_per_tile": 64}, {"contacts_rows_per_tile": 256}, {"contacts_words_per_item": 1}, {"contacts_words_per_item": 64},
         {"contacts_skip_zero": 0}, {"grid_cap_a": 1}]


@pytest.mark.parametrize("tune", TUNES, ids=["default", "rows_per_tile-64", "rows_per_tile-256", "words_per_item-1", "words_per_item-64", "skip_zero-0", "grid_cap_a-1"])
def test_edge_shapes(tune):
    """Column counts of 1, 63, 64, 65, 129 and row counts of 1, 64, 65, tile, tile + 1, a class of one group with itself, and a group
    without sites on either side; three samples of uploaded configurations, 3 lags, with and without the exclusion and the continuous ring."""
    spec = spec_for("C1")
    n = spec.num_atoms
    it, ctx = make("C1", spec, tune=tune)
    try:
        ctx.contacts_start(1, 1, [(0, 0)], [0.3])
        tile = int(ctx.contacts_info().rows_per_tile)
        assert tile == (tune or {}).get("contacts_rows_per_tile", 128)
        sizes = [1, 63, 64, 65, 129, tile, tile + 1]
        assert sum(sizes) + 3 * 8 <= n
        groups, at = np.full(n, -1, dtype=np.int8), 2
        for g, size in enumerate(sizes):                                # runs of the index, three particles without a site between them
            groups[at:at + size] = g
            at += size + 3
        classes = [(0, 4), (2, 1), (3, 2), (5, 3), (6, 0), (6, 6), (7, 2), (2, 7)]
        cuts = [1.5, 0.6, 0.6, 0.6, 0.9, 0.5, 0.6, 0.6]
        rng = np.random.default_rng(3)
        x0 = ctx.getPositions()
        configs = [x0, x0 + rng.normal(0, 0.08, x0.shape), x0 + rng.normal(0, 0.08, x0.shape)]
        mol = np.asarray(spec.mol_id)
        for exclude, continuous in [(False, True), (True, False)]:
            ctx.contacts_start(1000, 3, classes, cuts, groups=groups, exclude_same_molecule=exclude, continuous=continuous)
            lay = ctx.contacts_info()
            assert list(lay.num_sites[:8]) == sizes + [0] and list(lay.rows[:8]) == [1, 64, 65, tile, tile + 1, tile + 1, 0, 64]
            assert list(lay.cols[:8]) == [129, 63, 64, 65, 1, tile + 1, 64, 0]
            frames = []
            for x in configs:
                posq = ctx.getPosq()
                posq[:, :3] = x.astype(posq.dtype)                       # (the correction of the mixed precision stays as it is)
                ctx.posq.upload(posq)
                ctx.contacts_sample()
                frames.append(ctx.getPositions())                        # as the device holds them
            con = ctx.contacts_read()
            want = CR.contacts_reference(frames, [spec.box] * 3, groups, classes, cuts, 3, 1, mol if exclude else None, continuous)
            assert (con.samples, con.dropped) == (3, 0)
            assert_equal(con, want, (exclude, continuous))
            assert np.all(want[0][:5 if exclude else 6, 0, 1] > 0) and np.any(want[0][:, 1:, 2] < want[0][:, 1:, 1]) and not want[0][6:, :, 1:].any()
            assert list(con.words[7, :, 0]) == [3, 2, 1]                 # a class without sites still counts its visits
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 4. the ring, the schedule and the counts
def test_ring_wrap_schedule_and_counts():
    spec = spec_for("C3")
    groups = two_groups(spec.num_atoms, most=300)
    box = np.asarray(spec.box, dtype=np.float64)
    cuts = [0.45, 0.45, 0.4]
    it, ctx = make("C3", spec)
    try:
        it.step(3)                                                      # an unaligned start, host-driven
        ctx.frames_start(10, capacity=32, float64=True)
        ctx.contacts_start(10, 3, CLASSES, cuts, groups=groups, max_samples=12)
        lay = ctx.contacts_info()
        assert (lay.start_step, lay.num_origins) == (3, 3)
        ctx.run_graph(137, 10)                                          # steps 4 .. 140: 12 samples after 10 .. 120, 130 and 140 dropped
        con, f = ctx.contacts_read(reset=True), ctx.frames_read()
        assert list(f.step) == list(range(10, 141, 10)) and (con.samples, con.dropped, con.invalid) == (12, 2, 0)
        want = expected(f, range(12), groups, CLASSES, cuts, 3, 1)
        assert_equal(con, want)
        assert list(con.origins) == [12, 11, 10] and want[0][0, 0, 1] > 0      # every slot was overwritten three times
        z = ctx.contacts_read()
        assert (z.samples, z.dropped, z.invalid) == (0, 0, 0) and not z.words.any()
        # the schedule continues without gap or repeat, and no slot survived the reset
        ctx.run_graph(20, 10)
        con, f = ctx.contacts_read(), ctx.frames_read()
        assert list(f.step[14:]) == [150, 160] and (con.samples, con.dropped) == (2, 0)
        two = expected(f, [14, 15], groups, CLASSES, cuts, 3, 1)
        assert_equal(con, two)
        assert list(con.origins) == [2, 1, 0]
        # a box that no longer holds the largest cutoff: the due samples are dropped; back in range they count again
        ctx.setPeriodicBoxSize(*(box * (2 * 0.45 / box.min() * 0.99)))
        ctx.contacts_sample()
        ctx.setPeriodicBoxSize(*box)
        ctx.run_eager(10)
        con, f = ctx.contacts_read(), ctx.frames_read()
        assert list(f.step[16:]) == [170] and (con.samples, con.dropped) == (3, 1)
        assert_equal(con, expected(f, [14, 15, 16], groups, CLASSES, cuts, 3, 1))
        ctx.contacts_stop()
        assert ctx.contacts_info().active == 0 and ctx.contacts_info().words == 0
        for call in (ctx.contacts_read, ctx.contacts_sample):
            with pytest.raises(H.VVHipError) as e:
                call()
            assert e.value.code == H.ERR_INVALID and "none started" in str(e.value)
    finally:
        ctx.close()


def test_graph_replay_equals_eager_steps():
    spec = spec_for("C3")
    groups = two_groups(spec.num_atoms, most=300)
    (_, graph), (_, eager) = make("C3", spec), make("C3", spec)
    try:
        for c in (graph, eager):
            c.contacts_start(7, 5, CLASSES, [0.45, 0.45, 0.4], origin_every=2, groups=groups, exclude_same_molecule=True)
        graph.run_graph(60, 20)
        graph.run_eager(3)
        graph.run_graph(21, 20)
        eager.run_eager(84)
        g, e = graph.contacts_read(), eager.contacts_read()
        assert (g.samples, g.dropped, g.invalid) == (e.samples, e.dropped, e.invalid) == (12, 0, 0)
        assert np.array_equal(g.words, e.words) and g.words[:, :, 1].min() > 0
        assert same_bits(state(graph), state(eager))
    finally:
        graph.close()
        eager.close()


def test_steady_state_replays_capture_nothing():
    spec = spec_for("C3")
    groups = two_groups(spec.num_atoms, most=300)
    it, ctx = make("C3", spec)
    try:
        ctx.contacts_start(50, 4, CLASSES, [0.45, 0.45, 0.4], groups=groups)
        ctx.run_graph(400, 50)
        before = ctx.series_info().graph_captures
        ctx.run_graph(300, 50)
        assert ctx.series_info().graph_captures == before
        assert ctx.contacts_read().samples == 14
    finally:
        ctx.close()


def test_nine_riders_with_windows_that_shift_between_replays():
    """Series every 7, removals every 5, frames every 3, profile every 11, MSD every 13, RDF every 17, currents every 9, density modes
    every 6, contacts every 12, graphs of 20 steps, against one step at a time with all nine riders on in both; the contact table also
    against the reference over the context's own frames."""
    spec = spec_for("C3")
    groups, w = two_groups(spec.num_atoms, most=300), I.current_weights(spec)
    drude = np.ones(spec.num_atoms, dtype=np.int8)
    drude[np.asarray(spec.drude_pairs)[:, 0]] = 0
    cuts = [0.45, 0.45, 0.4]
    modes = I.modes_in_shells((1.0, 1.0, 1.0), 2 * np.pi * 1.5)[:8]
    (it1, graph), (it2, single) = make("C3", spec), make("C3", spec)
    try:
        for c in (graph, single):
            c.series_start(7, capacity=32)
            c.remove_cm_motion_every(5)
            c.frames_start(3, capacity=64, float64=True)
            c.profile_start(11, 64, groups=drude, max_samples=100, charge=True, mass=True)
            c.msd_start(13, 8, 3, groups=drude, max_samples=100)
            c.rdf_start(17, TR.short_r(spec), 32, [(0, 1), (1, 1)], groups=groups, max_samples=100)
            c.current_start(9, 8, 3, groups=drude, max_samples=100)
            c.modes_start(6, modes, num_lags=7, origin_every=2, weights=w, groups=drude, max_samples=100)
            c.contacts_start(12, 5, CLASSES, cuts, origin_every=2, groups=groups, max_samples=100)
        graph.run_graph(70, 20)
        graph.run_eager(3)
        graph.run_graph(47, 20)
        for _ in range(120):
            it2.step(1)
        kg, ks = graph.contacts_read(), single.contacts_read()
        assert (kg.samples, kg.dropped, kg.invalid) == (ks.samples, ks.dropped, ks.invalid) == (10, 0, 0)
        assert np.array_equal(kg.words, ks.words)
        fg, fs = graph.frames_read(), single.frames_read()
        assert list(fg.step) == list(fs.step) == list(range(3, 121, 3)) and eq(fg.positions, fs.positions)
        want = expected(fg, range(3, 40, 4), groups, CLASSES, cuts, 5, 2)
        assert_equal(kg, want)
        assert want[0][0, 0, 1] > 0
        dg, ds = graph.modes_read(), single.modes_read()
        assert dg.samples == ds.samples == 20 and np.array_equal(dg.words, ds.words)
        cg, cs = graph.current_read(), single.current_read()
        assert cg.samples == cs.samples == 13 and np.array_equal(cg.words, cs.words)
        mg, ms = graph.msd_read(), single.msd_read()
        assert mg.samples == ms.samples == 9 and np.array_equal(mg.words, ms.words)
        rg, rs = graph.rdf_read(), single.rdf_read()
        assert rg.samples == rs.samples == 7 and np.array_equal(rg.counts, rs.counts)
        pg, ps = graph.profile_read(), single.profile_read()
        assert pg.samples == ps.samples == 10 and np.array_equal(pg.words, ps.words)
        rows = [c.series_read() for c in (graph, single)]
        assert all(list(r.step) == list(range(7, 121, 7)) for r in rows)
        assert [c.cm_motion_record().removals for c in (graph, single)] == [24, 24]
        assert same_bits(state(graph), state(single))
    finally:
        graph.close()
        single.close()


# ------------------------------------------------------------------------------------------ 5. repair, restart, the barostat, a sharded plan
def test_a_repair_puts_table_and_rings_back_with_the_step_counter():
    """vvhip_debug_recover repairs on request, without anything having failed: the snapshot of the run call goes back -- the recorder's
    whole allocation, both rings included, with the step counter -- and the call is repeated.  origin_every = 1 and num_lags = 2 make rings
    of two slots, each overwritten five times inside the repeated window of 100 steps: the repeat's first sample measures against the
    origin and the surviving contacts of the sample before the window, which the window's last samples overwrote.  Rings that did not go
    back show as a different table, samples added twice as 23 samples."""
    spec = spec_for("C3")
    groups = two_groups(spec.num_atoms, most=300)
    (it1, rec), (it2, calm) = make("C3", spec), make("C3", spec)
    try:
        for c in (rec, calm):
            c.run_graph(50, 50)
            c.contacts_start(10, 2, CLASSES, [0.45, 0.45, 0.4], groups=groups, max_samples=100)
            c.run_graph(30, 10)                                     # three samples before the snapshot
            c.synchronize()
        assert rec.contacts_info().num_origins == 2
        assert rec.fused_status()[0] and rec.recovery_count() == 0
        rec.run_graph(100, 50)
        calm.run_graph(100, 50)
        H.check(H.lib.vvhip_debug_recover(rec.plan), rec.plan)
        assert rec.recovery_count() == 1 and not rec.fused_status()[0] and rec.status_words() == [0, 0, 0, 0]
        r, q = rec.contacts_read(), calm.contacts_read()
        assert (r.samples, r.dropped, r.invalid) == (q.samples, q.dropped, q.invalid) == (13, 0, 0)
        assert np.array_equal(r.words, q.words) and r.words[:, :, 1].min() > 0
        assert same_bits(state(rec), state(calm))
        assert rec.series_info().steps == calm.series_info().steps == 180
    finally:
        rec.close()
        calm.close()


def test_start_over_a_running_recorder_equals_stop_then_start():
    """25 steps in graphs of 5 with 4 lags (steps 10 and 20 are due), then 6 lags -- plan A without a stop, nothing read or synchronised in
    between, plan B after a stop -- and 20 steps more (steps 30 and 40 are due)."""
    spec = spec_for("C3")
    groups = two_groups(spec.num_atoms, most=300)
    (_, a), (_, b) = make("C3", spec), make("C3", spec)
    try:
        for c in (a, b):
            c.contacts_start(10, 4, CLASSES, [0.45, 0.45, 0.4], groups=groups)
            c.run_graph(25, 5)
        b.contacts_stop()
        assert not b.contacts_info().active
        for c in (a, b):
            c.contacts_start(10, 6, CLASSES, [0.45, 0.45, 0.4], groups=groups)
            lay = c.contacts_info()
            assert lay.active and lay.num_lags == 6 and lay.start_step == c.series_info().steps == 25
            c.run_graph(20, 5)
        ra, rb = a.contacts_read(), b.contacts_read()
        assert (ra.samples, ra.dropped) == (rb.samples, rb.dropped) == (2, 0)
        assert ra.words.shape == (3, 6, 4) and np.array_equal(ra.words, rb.words) and ra.words.any()
    finally:
        a.close()
        b.close()


def test_a_barostat_move_between_samples_keeps_the_origins():
    """An accepted and a rejected scale_box between samples: every sample is built with the box it was enqueued under, which is the box its
    frame carries, and the origins stored before a move are still measured against afterwards -- the reference knows no origin floor."""
    spec = spec_for("C3")
    groups = two_groups(spec.num_atoms, most=300)
    cuts = [0.45, 0.45, 0.4]
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(10, capacity=16, float64=True)
        ctx.contacts_start(10, 6, CLASSES, cuts, groups=groups)
        ctx.run_graph(20, 10)
        ctx.scale_box((1.01, 0.99, 1.02))                             # accepted
        ctx.run_graph(20, 10)
        ctx.scale_box((0.97, 0.97, 0.97))
        ctx.restore_box()                                             # rejected
        ctx.run_graph(20, 10)
        con, f = ctx.contacts_read(), ctx.frames_read()
        assert list(f.step) == list(range(10, 61, 10)) and (con.samples, con.dropped, con.invalid) == (6, 0, 0)
        assert eq(f.box[0], f.box[1]) and not eq(f.box[1], f.box[2]) and eq(f.box[2], f.box[5])
        want = expected(f, range(6), groups, CLASSES, cuts, 6, 1)
        assert_equal(con, want)
        assert list(con.origins) == [6, 5, 4, 3, 2, 1] and want[0][0, 5, 1] > 0      # the first origin is measured against across both moves
    finally:
        ctx.close()


def test_a_sharded_plan_is_refused_and_allocates_nothing():
    spec = spec_for("C3")
    n = spec.num_atoms
    mol = np.asarray(spec.mol_id)
    cut = int(np.nonzero(mol == mol[n // 2])[0].min())
    it = integrator_for("C3", spec)
    it.setUseCOMTempGroup(False)
    ctx = I.Context(spec, it, precision="mixed", force_provider="tether", shard=(0, cut))
    try:
        def live():
            count, size = C.c_int64(), C.c_int64()
            assert H.lib.vvhip_debug_live_buffers(C.byref(count), C.byref(size)) == H.OK
            return count.value, size.value
        before = live()
        with pytest.raises(H.VVHipError) as e:
            ctx.contacts_start(10, 4, CLASSES, [0.45, 0.45, 0.4], groups=two_groups(n))
        assert e.value.code == H.ERR_UNSUPPORTED and "shard" in str(e.value)
        assert live() == before and ctx.contacts_info().active == 0
    finally:
        ctx.close()
