"""Device-side spatial distribution functions (include/vvhip.h: vvhip_sdf_*) on the GPU.  The ground truth needs no second trajectory:
the same context also runs the frame recorder (float64) at the same interval, and the expected table is tests/sdf_reference.py over
those frames, each with its own box.  Every comparison is np.array_equal on int64.  A case has at most ~500 frames, ~1 000 sites and 6
samples, so the NumPy reference stays within a second or two per case.  The molecular frames come from each molecule's first three
particles that have mass and are no Drude particle: with the Drude particles left in, C3's first triplet has |p|^2 = 0 at the start."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdf_reference as SR       # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S, I = pkg.systems, pkg.integrator
H = I.H

pytestmark = pytest.mark.gpu

NH_FIELDS = ("eta", "eta_dot", "eta_dotdot", "ke2", "vscale", "v_bias")
SCALE = {"C1": 1.0, "C3": 0.1, "C5": 0.25}
NUM_FRAMES = {"C1": 166, "C3": 500, "C5": 256}
_SPECS, _FRAMES = {}, {}
CLASSES = [(0, 0), (0, 1), (1, 1), (1, 0)]
# Not sparse at n = 16, h = 0.5: a kernel that bins nothing, or into a few voxels, cannot pass.  A sample has about F S 8 h^3 / V pairs in
# range: on the start configurations (the reference alone) 3 590, 9 089 and 3 431 of them in 1 919, 3 171 and 2 045 of the 4 096 voxels
# for C1, C3, C5 -- C3 has 500 frames, the other two 166 and 256 -- so more than half the voxels for C3 and more
# than a quarter for the others, with room for the pairs the exclusion takes out
DENSE = {"C1": 4096 // 4, "C3": 4096 // 2, "C5": 4096 // 4}


def spec_for(cfg):
    if cfg not in _SPECS:
        _SPECS[cfg] = S.make_config(cfg, scale=SCALE[cfg])
    return _SPECS[cfg]


def frames_for(cfg):
    """The molecules' frames (shared, never written to) and their groups: even and odd frames."""
    if cfg not in _FRAMES:
        spec = spec_for(cfg)
        fr = SR.frames_of_molecules(spec.mol_id, spec.masses, spec.drude_pairs[:, 0], most=500)
        assert len(fr) == NUM_FRAMES[cfg]
        fr.setflags(write=False)
        _FRAMES[cfg] = fr
    fr = _FRAMES[cfg]
    return fr, (np.arange(len(fr)) % 2).astype(np.int8)


def integrator_for(cfg, spec, middle=True, dt=0.001):
    it = I.VVIntegrator(333.0, 10.0, 1.0, 40.0, dt, 3, 1)
    if cfg != "C1":
        it.setMaxDrudeDistance(0.02)
    if cfg == "C5":
        lz = float(spec.box[2])
        it.setMirrorLocation(lz / 2)
        it.setElectricField(2.0 / lz * 2 * 1.602176634e-22)
    it.setUseMiddleScheme(middle)
    return it


def make(cfg, spec, precision="mixed", middle=True, dt=0.001, **kw):
    it = integrator_for(cfg, spec, middle, dt)
    return it, I.Context(spec, it, precision=precision, force_provider="tether", **kw)


def two_groups(n, most=500):
    """Site groups by particle index: every k-th particle in group 0, its successor in group 1, the rest no site; at most `most` sites
    each.  Neighbours in index share a molecule, so the exclusion has sites to leave out."""
    k = max(2, -(-n // most))
    g = np.full(n, -1, dtype=np.int8)
    g[np.arange(n) % k == 0] = 0
    g[np.arange(n) % k == 1] = 1
    return g


def largest_extent(box):
    return float(min(box)) / 2 / np.sqrt(3.0)


def state(ctx):
    st = ctx.getNHState()
    return [ctx.getPosq(), ctx.getPosqCorrection(), ctx.getVelm()] + [np.array(getattr(st, f)) for f in NH_FIELDS]


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def eq(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def expected(frames, which, fr, classes, extent, nbins, fg=None, sg=None, mol_id=None):
    """(table, invalid, bad_frames, frame_visits) of the reference over the recorded frames `which`, each with the box its step ran with."""
    assert eq(frames.particles, np.arange(len(frames.particles), dtype=np.int32))
    table, invalid, bad, visits = np.zeros((len(classes), nbins, nbins, nbins), dtype=np.int64), 0, 0, np.zeros(16, dtype=np.int64)
    for j in which:
        t, i, b, v = SR.sdf_reference(frames.positions[j], frames.box[j], fr, classes, extent, nbins, fg, sg, mol_id)
        table += t
        invalid += i
        bad += b
        visits += v
    return table, invalid, bad, visits


def agrees(r, want):
    """The device's table and counts against expected()'s tuple."""
    table, invalid, bad, visits = want
    return (r.counts.dtype == np.int64 and np.array_equal(r.counts, table) and (r.invalid, r.bad_frames) == (invalid, bad)
            and np.array_equal(r.frame_visits, visits[:len(r.frame_visits)]))


# ------------------------------------------------------------------------------------------ 1. the table equals the reference over the frames
CASES = [("C1", "mixed", True), ("C3", "mixed", True), ("C5", "mixed", True), ("C3", "single", True), ("C3", "double", True), ("C3", "mixed", False)]


@pytest.mark.parametrize("cfg,precision,middle", CASES, ids=[f"{c}-{p}-{'middle' if m else 'classic'}" for c, p, m in CASES])
def test_table_equals_the_reference_over_the_frames(cfg, precision, middle):
    """Every description -- (n, h, exclusion) of (1, 0.45 min(L) / sqrt 3, off), (16, 0.5, on), (128, 0.7 or 0.4 min(L) / sqrt 3, off, one
    class) -- takes the next 20 steps of one context with a sample every 10, which records its own frames beside it; a second context
    takes the same samples through eager steps (frames of its own beside it), a third runs the same steps without a recorder."""
    spec = spec_for(cfg)
    fr, fg = frames_for(cfg)
    sg, mol = two_groups(spec.num_atoms), np.asarray(spec.mol_id)
    most = largest_extent(spec.box)
    (_, rec), (_, eager), (_, plain) = make(cfg, spec, precision, middle), make(cfg, spec, precision, middle), make(cfg, spec, precision, middle)
    try:
        for c in (rec, eager):
            c.frames_start(10, capacity=8, float64=True)
        descriptions = [(1, 0.45 * 2 * most, False, CLASSES), (16, 0.5, True, CLASSES), (128, min(0.7, 0.4 * 2 * most), False, [(0, 1)])]
        for k, (n, h, exclude, classes) in enumerate(descriptions):
            for c in (rec, eager):
                c.sdf_start(10, h, n, fr, classes, frame_groups=fg, site_groups=sg, exclude_same_molecule=exclude, max_samples=100)
            lay = rec.sdf_info()
            assert (lay.active, lay.nbins, lay.num_classes, lay.words, lay.start_step) == (1, n, len(classes), len(classes) * n ** 3, 20 * k)
            assert list(lay.pairs_per_sample[:len(classes)]) == list(SR.pairs_per_sample(fg, sg, classes, len(fr), spec.num_atoms))
            rec.run_graph(20, 10)
            eager.run_eager(20)
            r, e, f, fe = rec.sdf_read(), eager.sdf_read(), rec.frames_read(), eager.frames_read()
            assert list(f.step[2 * k:]) == [20 * k + 10, 20 * k + 20]
            args = (fr, classes, h, n, fg, sg, mol if exclude else None)
            want = expected(f, range(2 * k, 2 * k + 2), *args)
            print(cfg, precision, (n, h, exclude), "in range", int(want[0].sum()), "voxels hit", int(np.count_nonzero(want[0].sum(axis=0))), "of", n ** 3)
            assert (r.samples, r.dropped) == (2, 0) and want[1:3] == (0, 0) and want[3][:2].sum() == 2 * len(fr)
            assert agrees(r, want), (n, h, exclude)
            assert want[0].sum() > 0
            if n == 16:
                assert np.count_nonzero(want[0].sum(axis=0)) > DENSE[cfg]
            # the eager steps: the same table bit for bit wherever they are the same trajectory bit for bit (all but C5, whose Langevin
            # particles draw other numbers in a captured graph, which begins with a refill of the random buffer); there the eager table
            # is held to the reference over the eager context's own frames
            same_trajectory = eq(fe.positions[2 * k:], f.positions[2 * k:])
            assert same_trajectory == (cfg != "C5")
            assert (e.samples, e.dropped) == (2, 0)
            assert agrees(e, want if same_trajectory else expected(fe, range(2 * k, 2 * k + 2), *args))
            assert eq(np.float64(r.inv_volume_sum), np.float64(SR.inv_volume_sum(f.box[2 * k:2 * k + 2]))) and eq(np.float64(e.inv_volume_sum), np.float64(r.inv_volume_sum))
        plain.run_graph(60, 10)
        assert same_bits(state(rec), state(plain))
    finally:
        for c in (rec, eager, plain):
            c.close()


# ------------------------------------------------------------------------------------------ 2. tile edges
@pytest.mark.parametrize("tune", [None, {"sdf_items_target": 2}], ids=["default", "sdf_items_target-2"])
def test_tile_edges(tune):
    """Frame and site counts of 1, 63, 64, 65 and 257 = tile + 1, and a group without members on either side of a class.  One sample of
    the configuration as it stands (sdf_sample).  The tune makes blocks take several j-tiles: the same table."""
    spec = spec_for("C3")
    n = spec.num_atoms
    fr, _ = frames_for("C3")
    it, ctx = make("C3", spec, tune=tune)
    try:
        ctx.sdf_start(1, 0.5, 2, fr, [(0, 0)])
        tile = int(ctx.sdf_info().tile)
        assert tile == 256
        sizes = [1, 63, 64, 65, tile + 1]
        assert sum(sizes) <= len(fr) and sum(sizes) + 6 * 3 <= n
        fg = np.full(len(fr), -1, dtype=np.int8)
        sg, at_f, at_s = np.full(n, -1, dtype=np.int8), 0, 5
        for g, size in enumerate(sizes):                                # runs of the index; three particles without a site between the runs
            fg[at_f:at_f + size] = g
            sg[at_s:at_s + size] = g
            at_f, at_s = at_f + size, at_s + size + 3
        classes = [(g, g) for g in range(5)] + [(0, 4), (4, 0), (1, 3), (3, 1), (2, 4), (4, 2), (5, 2), (2, 5), (5, 5), (4, 3), (3, 4)]
        mol = np.asarray(spec.mol_id)
        for nbins, h, exclude in [(16, 0.5, False), (5, 0.6, True)]:
            ctx.sdf_start(1000, h, nbins, fr, classes, frame_groups=fg, site_groups=sg, exclude_same_molecule=exclude)
            lay = ctx.sdf_info()
            assert list(lay.num_frames[:6]) == sizes + [0] and list(lay.num_sites[:6]) == sizes + [0]
            assert list(lay.pairs_per_sample[:16]) == [sizes[a] * sizes[b] if max(a, b) < 5 else 0 for a, b in classes]
            if tune is None:
                assert lay.num_items == sum(-(-sizes[a] // tile) * -(-sizes[b] // 64) for a, b in classes if max(a, b) < 5)
            else:
                assert lay.num_items < 40                               # runs of several tiles: (4, 4) is two i-tiles of one run each
            ctx.sdf_sample()
            r = ctx.sdf_read()
            want = SR.sdf_reference(ctx.getPositions(), spec.box, fr, classes, h, nbins, fg, sg, mol if exclude else None)
            assert (r.samples, r.dropped) == (1, 0) and want[1:3] == (0, 0)
            assert agrees(r, want), (nbins, h, exclude)
            assert not r.counts[[11, 12, 13]].any() and want[0][4].sum() > 0 and want[0][9].sum() > 0 and want[0][5].sum() + want[0][6].sum() > 0
            assert list(r.frame_visits[:6]) == sizes + [0]
        # a sample of a single class without work still counts
        ctx.sdf_start(1000, 0.5, 8, fr, [(5, 5)], frame_groups=fg, site_groups=sg)
        ctx.sdf_sample()
        ctx.sdf_sample()
        r = ctx.sdf_read()
        assert (r.samples, r.dropped) == (2, 0) and not r.counts.any() and ctx.sdf_info().num_items == 0
        assert list(r.frame_visits[:5]) == [2 * s for s in sizes]
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 3. voxel edges, images and bad frames
def test_voxel_edges_images_and_bad_frames_with_hand_made_positions():
    spec = spec_for("C1")
    n = spec.num_atoms
    mols, _ = frames_for("C1")
    it, ctx = make("C1", spec, precision="double")
    try:
        box = np.array([4.0, 5.0, 6.0])
        ctx.setPeriodicBoxSize(*box)
        posq = ctx.getPosq()
        assert posq.dtype == np.float64
        hand = posq.copy()
        base = np.array([1.0, 1.0, 1.0])
        ex, ey = np.array([0.25, 0.0, 0.0]), np.array([0.0, 0.25, 0.0])

        def place(triplet, o, a, b):
            for i, x in zip(triplet, (o, a, b)):
                hand[i, :3] = x
        place(mols[0], base, base + ex, base + ey)                      # frame 0: along the box axes
        place(mols[1], base, base + ex, base - ey)                      # frame 1: b mirrored through the e1 axis
        place(mols[2], base, base + ex, [np.nan, 1.0, 1.0])             # a NaN in a frame atom
        place(mols[3], base, base, base + ey)                           # a on top of o
        place(mols[4], base, base + ex, base + 3 * ex)                  # o, a, b collinear
        frames = np.array(mols[:5])
        fg = np.array([0, 2, 1, 1, 1], dtype=np.int8)
        free = [int(i) for i in mols[10:40].reshape(-1)]                # particles of other molecules
        sites = {free[0]: base - [1.0, 0.0, 0.0],                       # xi1 = -h exactly: voxel 0
                 free[1]: base + [1.0, 0.0, 0.0],                       # xi1 = +h exactly: out
                 free[2]: base,                                         # xi = 0: voxel n / 2 on every axis
                 free[3]: base + [0.25, 0.0, 0.0],                      # on the edge between voxels 4 and 5: 5
                 free[4]: base + [-1.0 + 3 * 4.0, -2 * 5.0, 6.0],       # the first again, three images away
                 free[5]: base + [0.25 + 3 * 4.0, -2 * 5.0, 6.0],       # the edge again
                 free[6]: [1.0, np.nan, 1.0]}                           # NaN: invalid, no voxel
        sg = np.full(n, -1, dtype=np.int8)
        for i, x in sites.items():
            hand[i, :3] = x
            sg[i] = 0
        rng = np.random.default_rng(12)
        generic = free[10:70]                                           # off the voxel faces (with probability 1)
        hand[generic, :3] = base + rng.uniform(-0.95, 0.95, size=(len(generic), 3))
        sg[generic] = 1
        o, E, good = SR.frame_axes(hand[:, :3], frames)
        assert list(good) == [True, True, False, False, False]
        assert np.array_equal(E[0], np.eye(3)) and np.array_equal(E[1], np.diag([1.0, -1.0, -1.0]))      # the premise of the exact edges
        classes = [(0, 0), (0, 1), (2, 1), (1, 0), (1, 1)]
        ctx.posq.upload(hand)
        ctx.sdf_start(1000, 1.0, 8, frames, classes, frame_groups=fg, site_groups=sg)
        ctx.sdf_sample()
        r = ctx.sdf_read()
        want = np.zeros((8, 8, 8), dtype=np.int64)
        want[0, 4, 4], want[4, 4, 4], want[5, 4, 4] = 2, 1, 2
        assert (r.samples, r.invalid, r.bad_frames) == (1, 1, 3) and list(r.frame_visits) == [1, 0, 1]
        assert np.array_equal(r.counts[0], want)
        assert r.counts[1].sum() > 30 and np.array_equal(r.counts[2], r.counts[1][:, ::-1, ::-1]) and not np.array_equal(r.counts[2], r.counts[1])
        assert not r.counts[3:].any()                                   # a bad frame takes part in no pair, not in `invalid` either
        ref = SR.sdf_reference(hand[:, :3], box, frames, classes, 1.0, 8, fg, sg)
        assert ref[1:3] == (1, 3) and agrees(r, ref)
        assert np.array_equal(r.edges, np.linspace(-1.0, 1.0, 9)) and r.voxel == 0.25
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 4. schedule and counts
def test_schedule_and_counts():
    spec = spec_for("C3")
    fr, fg = frames_for("C3")
    sg = two_groups(spec.num_atoms)
    box = np.asarray(spec.box, dtype=np.float64)
    h, n = 0.995 * largest_extent(box), 12
    args = (fr, CLASSES, h, n, fg, sg)
    it, ctx = make("C3", spec)
    try:
        it.step(3)                                                      # an unaligned start, host-driven
        ctx.frames_start(10, capacity=16, float64=True)
        ctx.sdf_start(10, h, n, fr, CLASSES, frame_groups=fg, site_groups=sg, max_samples=3)
        assert ctx.sdf_info().start_step == 3
        ctx.run_graph(47, 10)                                           # steps 4 .. 50: samples after 10, 20, 30; 40 and 50 dropped
        r = ctx.sdf_read(reset=True)
        f = ctx.frames_read()
        assert list(f.step) == [10, 20, 30, 40, 50] and (r.samples, r.dropped) == (3, 2)
        assert agrees(r, expected(f, range(3), *args)) and r.counts.sum() > 0 and r.frame_visits.sum() == 3 * len(fr)
        assert eq(np.float64(r.inv_volume_sum), np.float64(SR.inv_volume_sum([box] * 3)))
        z = ctx.sdf_read()
        assert (z.samples, z.dropped, z.invalid, z.bad_frames, z.inv_volume_sum) == (0, 0, 0, 0, 0.0) and not z.counts.any() and not z.frame_visits.any()
        # the schedule continues without gap or repeat
        ctx.run_graph(20, 10)
        r, f = ctx.sdf_read(), ctx.frames_read()
        assert list(f.step[5:]) == [60, 70] and (r.samples, r.dropped) == (2, 0)
        two = expected(f, range(5, 7), *args)
        assert agrees(r, two)
        # a box that no longer holds the cube: the due samples are dropped, table and visits stay; back in range they count again
        ctx.setPeriodicBoxSize(*(box * 0.99))
        ctx.run_graph(20, 10)
        ctx.sdf_sample()
        r = ctx.sdf_read()
        assert (r.samples, r.dropped) == (2, 3) and agrees(r, two)
        ctx.setPeriodicBoxSize(*box)
        ctx.run_eager(10)
        r, f = ctx.sdf_read(), ctx.frames_read()
        assert list(f.step[7:]) == [80, 90, 100] and (r.samples, r.dropped) == (3, 3)
        third = expected(f, [9], *args)
        assert agrees(r, (two[0] + third[0], 0, 0, two[3] + third[3]))
        assert eq(np.float64(r.inv_volume_sum), np.float64(SR.inv_volume_sum([box] * 3)))
        # stop: no recorder, no sample
        ctx.sdf_stop()
        assert ctx.sdf_info().active == 0 and ctx.sdf_info().words == 0
        for call in (ctx.sdf_read, ctx.sdf_sample):
            with pytest.raises(H.VVHipError) as e:
                call()
            assert e.value.code == H.ERR_INVALID and "none started" in str(e.value)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 5. steady-state replays
def test_steady_state_replays_capture_nothing():
    spec = spec_for("C3")
    fr, fg = frames_for("C3")
    it, ctx = make("C3", spec)
    try:
        ctx.sdf_start(50, 0.5, 16, fr, CLASSES, frame_groups=fg, site_groups=two_groups(spec.num_atoms))
        ctx.run_graph(400, 50)
        before = ctx.series_info().graph_captures
        ctx.run_graph(300, 50)
        assert ctx.series_info().graph_captures == before
        assert ctx.sdf_read().samples == 14
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 6. riders together
def test_riders_together():
    """Frames every 5, profile every 11, MSD every 7, RDF every 15, SDF every 10 on one context, graphs of 20 steps: beside a context
    without the SDF every other recorder gives what it gives there, and the SDF the reference over the frames."""
    spec = spec_for("C3")
    fr, fg = frames_for("C3")
    sg = two_groups(spec.num_atoms)
    (it1, five), (it2, four) = make("C3", spec), make("C3", spec)
    try:
        for c in (five, four):
            c.frames_start(5, capacity=32, float64=True)
            c.profile_start(11, 64, groups=sg, max_samples=100, charge=True, mass=True)
            c.msd_start(7, 4, 2, groups=sg, max_samples=100)
            c.rdf_start(15, 0.6, 100, [(0, 1), (0, 0)], groups=sg, exclude_same_molecule=True)
        five.sdf_start(10, 0.5, 16, fr, CLASSES, frame_groups=fg, site_groups=sg, exclude_same_molecule=True)
        for c in (five, four):
            c.run_graph(40, 20)
            c.run_eager(3)
            c.run_graph(17, 20)
        f5, f4 = five.frames_read(), four.frames_read()
        assert list(f5.step) == list(range(5, 61, 5)) and eq(f5.positions, f4.positions)
        p5, p4 = five.profile_read(), four.profile_read()
        assert p5.samples == p4.samples == 5 and np.array_equal(p5.words, p4.words)
        m5, m4 = five.msd_read(), four.msd_read()
        assert m5.samples == m4.samples == 8 and np.array_equal(m5.words, m4.words) and m5.pairs.sum() > 0
        g5, g4 = five.rdf_read(), four.rdf_read()
        assert g5.samples == g4.samples == 4 and np.array_equal(g5.counts, g4.counts) and g5.counts.sum() > 0
        r = five.sdf_read()
        want = expected(f5, [1, 3, 5, 7, 9, 11], fr, CLASSES, 0.5, 16, fg, sg, np.asarray(spec.mol_id))
        assert (r.samples, r.dropped) == (6, 0) and agrees(r, want) and want[0].sum() > 0
        assert same_bits(state(five), state(four))
    finally:
        five.close()
        four.close()


# ------------------------------------------------------------------------------------------ 7. recovery
def test_a_repair_puts_head_and_table_back_with_the_step_counter():
    """vvhip_debug_recover repairs on request, without anything having failed: the snapshot of the run call goes back -- the recorder's
    counts and table with the step counter -- and the call is repeated.  A table that did not go back shows as samples added twice."""
    spec = spec_for("C3")
    fr, fg = frames_for("C3")
    sg = two_groups(spec.num_atoms)
    (it1, rec), (it2, calm) = make("C3", spec), make("C3", spec)
    try:
        for c in (rec, calm):
            c.run_graph(50, 50)
            c.sdf_start(10, 0.5, 16, fr, CLASSES, frame_groups=fg, site_groups=sg)
            c.run_graph(30, 10)                                     # three samples before the snapshot
            c.synchronize()
        assert rec.fused_status()[0] and rec.recovery_count() == 0
        rec.run_graph(100, 50)
        calm.run_graph(100, 50)
        H.check(H.lib.vvhip_debug_recover(rec.plan), rec.plan)
        assert rec.recovery_count() == 1 and not rec.fused_status()[0] and rec.status_words() == [0, 0, 0, 0]
        r, q = rec.sdf_read(), calm.sdf_read()
        assert (r.samples, r.dropped, r.invalid, r.bad_frames) == (q.samples, q.dropped, q.invalid, q.bad_frames) == (13, 0, 0, 0)
        assert np.array_equal(r.counts, q.counts) and r.counts.sum() > 0 and eq(np.float64(r.inv_volume_sum), np.float64(q.inv_volume_sum))
        assert np.array_equal(r.frame_visits, q.frame_visits) and r.frame_visits.sum() == 13 * len(fr)
        assert same_bits(state(rec), state(calm))
        assert rec.series_info().steps == calm.series_info().steps == 180
    finally:
        rec.close()
        calm.close()


# ------------------------------------------------------------------------------------------ 8. the barostat
def test_barostat_moves_between_samples():
    """An accepted and a rejected scale_box between samples: every sample is binned with the box it was enqueued under, which is the box
    its frame carries."""
    spec = spec_for("C3")
    fr, fg = frames_for("C3")
    sg = two_groups(spec.num_atoms)
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(10, capacity=16, float64=True)
        ctx.sdf_start(10, 0.5, 16, fr, CLASSES, frame_groups=fg, site_groups=sg)
        ctx.run_graph(20, 10)
        ctx.scale_box((1.01, 0.99, 1.02))                             # accepted
        ctx.run_graph(20, 10)
        ctx.scale_box((0.97, 0.97, 0.97))
        ctx.restore_box()                                             # rejected
        ctx.run_graph(20, 10)
        r, f = ctx.sdf_read(), ctx.frames_read()
        assert list(f.step) == list(range(10, 61, 10)) and (r.samples, r.dropped) == (6, 0)
        assert eq(f.box[0], f.box[1]) and not eq(f.box[1], f.box[2]) and eq(f.box[2], f.box[5])
        want = expected(f, range(6), fr, CLASSES, 0.5, 16, fg, sg)
        assert agrees(r, want) and want[0].sum() > 0
        assert eq(np.float64(r.inv_volume_sum), np.float64(SR.inv_volume_sum(f.box)))
        g = r.g(1)
        assert g.shape == (16, 16, 16) and np.all(np.isfinite(g))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 9. a sharded plan
def test_a_sharded_plan_is_refused_and_allocates_nothing():
    spec = spec_for("C3")
    n = spec.num_atoms
    fr, fg = frames_for("C3")
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
            ctx.sdf_start(10, 0.5, 16, fr, CLASSES, frame_groups=fg, site_groups=two_groups(n))
        assert e.value.code == H.ERR_UNSUPPORTED and "shard" in str(e.value)
        assert live() == before and ctx.sdf_info().active == 0
    finally:
        ctx.close()
