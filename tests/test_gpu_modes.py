"""Device-side density modes, S(k) and F(k, t) (include/vvhip.h: vvhip_modes_*) on the GPU.  The ground truth needs no second trajectory:
the same context also runs the frame recorder (float64 positions) at the same interval, and the expected table is
tests/modes_reference.py over those frames, each with its own box.  Every comparison is np.array_equal on int64 words: the table, the
counts and the bits of box_sum."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import checkpoint_cases as K        # noqa: E402
import modes_reference as MR        # noqa: E402
import test_gpu_current as TC       # noqa: E402  (the reduced boxes and the helpers)
import test_modes as TM             # noqa: E402  (the lattice and the wrap list)

pkg = importlib.import_module("openmm-velocityverlet_amd")
S, I = pkg.systems, pkg.integrator
H = I.H

pytestmark = pytest.mark.gpu

spec_for, integrator_for, make, groups_for, state, same_bits, eq = TC.spec_for, TC.integrator_for, TC.make, TC.groups_for, TC.state, TC.same_bits, TC.eq

# about 40 modes: (0,0,0), a +-pair, a duplicate, the largest components, then the low shells
MODES = np.array([(0, 0, 0), (1, 2, 3), (-1, -2, -3), (4095, -4095, 1), (-4095, 4095, 4095), (1, 2, 3)] +
                 [tuple(m) for m in I.modes_in_shells((1.0, 1.0, 1.0), 2 * np.pi * 2.5)[:34]], dtype=np.int32)
assert len(MODES) == 40


def expected(frames, weights, groups, lay, modes, which=None, floor=0):
    """The reference over the frames `which` (all) as samples 0, 1, ... for the layout `lay`."""
    which = list(range(len(frames.step)) if which is None else which)
    assert frames.positions.dtype == np.float64 and frames.box.dtype == np.float64
    assert eq(frames.particles, np.arange(len(weights), dtype=np.int32))
    return MR.modes_reference(frames.positions[which], frames.box[which], weights, groups, lay.num_groups, modes, lay.num_lags, lay.origin_every,
                              lay.frac_bits, lay.limit_position, floor)


def assert_equal(dm, want, what=None):
    assert dm.words.dtype == np.int64 and np.array_equal(dm.words, want["words"]), what
    assert (dm.out_of_range, dm.invalid_samples) == (want["out_of_range"], want["invalid_samples"]), what
    assert eq(np.asarray(dm.box_sum, dtype=np.float64), np.asarray(want["box_sum"], dtype=np.float64)), what


# ------------------------------------------------------------------------------------------ 1. the table equals the reference over the frames
CASES = [("C3", "mixed", True), ("C3", "single", True), ("C3", "double", True), ("C3", "mixed", False), ("C5", "mixed", True)]


@pytest.mark.parametrize("cfg,precision,middle", CASES, ids=[f"{c}-{p}-{'middle' if m else 'classic'}" for c, p, m in CASES])
def test_table_equals_the_reference_over_the_frames(cfg, precision, middle):
    """Two groups, the charges as weights, 40 modes, 12 samples, 5 lags with every other sample an origin; a context without a recorder
    runs the same steps."""
    spec = spec_for(cfg)
    groups, w = groups_for(cfg, spec), np.asarray(spec.charges, dtype=np.float64)
    (_, rec), (_, plain) = make(cfg, spec, precision, middle), make(cfg, spec, precision, middle)
    try:
        rec.frames_start(10, capacity=16, float64=True)
        rec.modes_start(10, MODES, num_lags=5, origin_every=2, weights=w, groups=groups, max_samples=1000)
        lay = rec.modes_info()
        sites = [int(np.count_nonzero(groups == g)) for g in range(2)]
        assert (lay.active, lay.num_groups, lay.num_modes, lay.num_origins, lay.row_words) == (1, 2, 40, 3, MR.row_words(2, 40))
        assert lay.words == 6 * MR.row_words(2, 40) and lay.start_step == 0 and list(lay.group_sites)[:2] == sites
        assert lay.weight_bound == MR.weight_bound(w, groups) and lay.frac_bits == MR.frac_bits(lay.weight_bound) and lay.limit_position == 64.0
        rec.run_graph(120, 40)
        dm, f = rec.modes_read(), rec.frames_read()
        assert list(f.step) == list(range(10, 121, 10))
        want = expected(f, w, groups, lay, MODES)
        assert (dm.samples, dm.dropped, dm.out_of_range, dm.invalid_samples, dm.origin_floor) == (12, 0, 0, 0, 0)
        assert_equal(dm, want)
        assert np.array_equal(dm.count, MR.lag_counts(12, 2, 5)) and dm.count[1:].sum() > 0
        # what the table must show whatever the trajectory: mode (0,0,0) is the squared total weight; a mode and its negative agree in
        # the real part; a duplicate is the same bits; S_gg > 0
        q0 = w[groups == 0].sum()
        assert np.allclose(dm.S(0, 0)[0] * sites[0], q0 * q0, rtol=1e-6, atol=1e-6)
        assert np.array_equal(dm.F(0, 0)[:, 1], dm.F(0, 0)[:, 5]) and np.isclose(dm.F(0, 1)[0, 1], dm.F(0, 1)[0, 2], rtol=1e-12, atol=1e-9)
        assert np.all(dm.S(1, 1)[6:] > 0)
        plain.run_graph(120, 40)
        assert same_bits(state(rec), state(plain))                    # the recorder changes nothing of the run
    finally:
        rec.close()
        plain.close()


# ------------------------------------------------------------------------------------------ 2. the smallest shapes and the launch shapes
def _selections(n):
    def run(first, count, G=1):
        g = np.full(n, -1, dtype=np.int8)
        g[first:first + count] = np.arange(count) % G
        return g
    three = (np.arange(n) % 2 * 2).astype(np.int8)                    # groups 0 and 2: group 1 has no site
    # K: a number of modes; run: the number of modes is the shape's mode run plus this
    return [dict(groups=run(0, 0), K=3, num_lags=2, every=1), dict(groups=run(n - 1, 1), K=1, num_lags=0, every=1),
            dict(groups=run(5, 63), run=-1, num_lags=3, every=2), dict(groups=run(3, 64), run=0, num_lags=4, every=4),
            dict(groups=run(7, 65, G=2), run=+1, num_lags=2, every=1), dict(groups=three, K=5, num_lags=3, every=1)]


TUNES = [None, {"modes_sites_per_thread": 1}, {"modes_sites_per_thread": 8}, {"modes_k_tile": 1}, {"modes_k_tile": 7}, {"modes_block_threads": 64},
         {"modes_block_threads": 192}, {"grid_cap_a": 1}]
_FIRST = []


@pytest.mark.parametrize("tune", TUNES, ids=["default", "P-1", "P-8", "k_tile-1", "k_tile-7", "block-64", "block-192", "grid_cap_a-1"])
def test_smallest_shapes_and_launch_shapes(tune):
    """C1 (1 992 particles).  0, 1, 63, 64 and 65 recorded sites, the 65 in two groups whose seam lies inside what would be one wave, a
    group without a site; K = 1 and K one below, at and one above the mode run of the shape in force.  Every description takes the next
    20 steps of one context with a sample behind every other step."""
    spec = spec_for("C1")
    n = spec.num_atoms
    w = np.asarray(spec.charges, dtype=np.float64)
    it, ctx = make("C1", spec, tune=tune)
    try:
        sel = _selections(n)
        ctx.frames_start(2, capacity=10 * len(sel), float64=True)
        for k, d in enumerate(sel):
            nk = d.get("K")
            if nk is None:
                ctx.modes_start(2, MODES, groups=d["groups"], weights=w)      # what mode run does this shape get?
                kt = ctx.modes_info().k_tile
                assert 1 <= kt < len(MODES)
                nk = max(kt + d["run"], 1)
            modes = MODES[:nk]
            ctx.modes_start(2, modes, num_lags=d["num_lags"], origin_every=d["every"], weights=w, groups=d["groups"], max_samples=100)
            lay = ctx.modes_info()
            assert lay.start_step == 20 * k and lay.num_particles == np.count_nonzero(d["groups"] >= 0) and lay.num_modes == nk
            if "run" in d:
                assert lay.k_tile == kt
            if tune and "grid_cap_a" not in tune:
                key, value = next(iter(tune.items()))
                assert getattr(lay, key[len("modes_"):]) == value
            ctx.run_graph(20, 10)
            dm, f = ctx.modes_read(), ctx.frames_read()
            want = expected(f, w, d["groups"], lay, modes, which=range(10 * k, 10 * k + 10))
            assert (dm.samples, dm.dropped, dm.out_of_range, dm.invalid_samples) == (10, 0, 0, 0), k
            assert_equal(dm, want, k)
            assert np.array_equal(dm.count, MR.lag_counts(10, d["every"], d["num_lags"]))
            if k == 0:
                assert not dm.words[:, 1:].any()                      # no site: every cell is +0.0
            if k == 5:
                assert not dm._cells(1, 1).any() and dm._cells(0, 2).any()
                _FIRST.append((f.positions[10 * k:].copy(), dm.words))
        # ... and for the last description equal to each other across the tunes wherever the trajectories are the same bits
        for x, words in _FIRST:
            if eq(x, _FIRST[0][0]):
                assert np.array_equal(words, _FIRST[0][1])
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 3. uploaded adversarial positions
def test_uploaded_lattice_and_wrap_positions_give_the_exact_sums():
    """The 8 x 8 x 8 lattice and the wrap list of tests/test_modes.py, uploaded into a double-precision C1 context whose particles are at
    rest on their tether sites: the step leaves them where they are -- asserted from the frame, not assumed -- so the device's sums are
    those of the exact cases: (512 2^30, 0) at the Bragg modes and (0, 0) elsewhere, and the wrap list's turns as Python integers form them."""
    spec = spec_for("C1")
    n = spec.num_atoms
    it, ctx = make("C1", spec, precision="double")
    try:
        for box, X, modes in [(TM.LATTICE_BOX, TM.lattice_positions(), TM.LATTICE_MODES), (TM.WRAP_BOX, TM.wrap_positions(), TM.WRAP_MODES)]:
            posq, velm = ctx.getPosq(), ctx.getVelm()
            posq[:len(X), :3] = X
            velm[:, :3] = 0.0
            ctx.posq.upload(posq)
            ctx.site.upload(posq)
            ctx.velm.upload(velm)
            ctx.forces_valid = False
            ctx.setPeriodicBoxSize(*box)
            groups = np.full(n, -1, dtype=np.int8)
            groups[:len(X)] = 0
            ctx.frames_start(1, capacity=4, float64=True)
            ctx.modes_start(1, modes, groups=groups)
            lay = ctx.modes_info()
            assert (lay.weight_bound, lay.frac_bits) == (2.0, 29)      # (weights of 1: W is the power of two ABOVE them)
            ctx.run_eager(1)
            dm, f = ctx.modes_read(), ctx.frames_read()
            assert dm.samples == 1 and dm.invalid_samples == 0
            # (by value: the step's x + v dt turns an uploaded -0.0 into +0.0, which is the same turn)
            assert np.array_equal(f.positions[-1][:len(X)], X), "the premise: the particles are where they were uploaded"
            A, B, bad = MR.sample_sums(X, np.array(box), np.ones(len(X)), None, 1, modes, lay.frac_bits)
            a, b = A[0].astype(np.float64) * 2.0 ** -lay.frac_bits, B[0].astype(np.float64) * 2.0 ** -lay.frac_bits
            assert np.array_equal(dm._cells(0, 0)[0], a * a + b * b)
            if box is TM.LATTICE_BOX:
                bragg = np.all(np.asarray(modes) % 8 == 0, axis=1)
                assert np.array_equal(dm._cells(0, 0)[0], np.where(bragg, 512.0 * 512.0, 0.0))
            assert eq(dm.box_sum, np.array(box, dtype=np.float64))
            ctx.modes_stop()
            ctx.frames_stop()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 4. eager against graph, all eight riders
@pytest.mark.parametrize("cfg", ["C3", "C5"])
def test_eager_steps_and_shifting_windows_give_the_same_bits(cfg):
    """Samples every 7 steps in graphs of 50: the replays' windows differ."""
    spec = spec_for(cfg)
    groups, w = groups_for(cfg, spec), np.asarray(spec.charges, dtype=np.float64)
    (it1, graph), (it2, eager), (it3, single) = make(cfg, spec), make(cfg, spec), make(cfg, spec)
    try:
        for c in (graph, eager, single):
            c.frames_start(7, capacity=32, float64=True)
            c.modes_start(7, MODES[:12], num_lags=6, origin_every=3, weights=w, groups=groups, max_samples=100)
        lay = graph.modes_info()
        graph.run_graph(140, 50)
        eager.run_eager(140)
        it3.step(140)
        dg, de, ds = graph.modes_read(), eager.modes_read(), single.modes_read()
        fg, fe, fs = graph.frames_read(), eager.frames_read(), single.frames_read()
        assert dg.samples == de.samples == ds.samples == 20 and list(fg.step) == list(range(7, 141, 7))
        assert_equal(dg, expected(fg, w, groups, lay, MODES[:12]))
        same_trajectory = eq(fe.positions, fg.positions)              # (C5's Langevin particles: tests/test_gpu_current.py says why not)
        assert same_trajectory == (cfg != "C5")
        assert np.array_equal(de.words, dg.words) if same_trajectory else True
        assert_equal(de, expected(fe, w, groups, lay, MODES[:12]))
        assert_equal(ds, expected(fs, w, groups, lay, MODES[:12]))
    finally:
        for c in (graph, eager, single):
            c.close()


def test_eight_riders_with_windows_that_shift_between_replays():
    """Series every 7, removals every 5, frames every 3, profile every 11, MSD every 13, RDF every 17, currents every 9, density modes
    every 6, graphs of 20 steps.  `graph` against `single` (one step at a time), all eight riders on in both; `truth` has the series and
    the removals on too (the removal changes the trajectory: like with like) and its frames at the mode recorder's steps."""
    spec = spec_for("C3")
    groups, w = groups_for("C3", spec), I.current_weights(spec)
    r_max = min(0.7, 0.3 * float(min(spec.box)))
    (it1, graph), (it2, single), (it3, truth) = make("C3", spec), make("C3", spec), make("C3", spec)
    try:
        for c in (graph, single, truth):
            c.series_start(7, capacity=32)
            c.remove_cm_motion_every(5)
        for c in (graph, single):
            c.frames_start(3, capacity=64, velocities=True, float64=True)
            c.profile_start(11, 64, groups=groups, max_samples=100, charge=True, mass=True, momentum=True, kinetic=True)
            c.msd_start(13, 8, 3, groups=groups, max_samples=100)
            c.rdf_start(17, r_max, 32, [(0, 1), (1, 1)], groups=groups, max_samples=100)
            c.current_start(9, 8, 3, groups=groups, max_samples=100)
            c.modes_start(6, MODES[:10], num_lags=7, origin_every=2, weights=w, groups=groups, max_samples=100)
        truth.frames_start(6, capacity=32, float64=True)
        lay = graph.modes_info()
        graph.run_graph(130, 20)
        graph.run_eager(3)
        graph.run_graph(47, 20)
        for _ in range(180):
            it2.step(1)
        truth.run_graph(180, 20)
        dg, ds = graph.modes_read(), single.modes_read()
        assert (dg.samples, dg.dropped, dg.out_of_range, dg.invalid_samples) == (ds.samples, ds.dropped, ds.out_of_range, ds.invalid_samples) == (30, 0, 0, 0)
        assert np.array_equal(dg.words, ds.words) and eq(dg.box_sum, ds.box_sum)
        ft = truth.frames_read()
        assert list(ft.step) == list(range(6, 181, 6))
        assert_equal(dg, expected(ft, w, groups, lay, MODES[:10]))
        assert dg.count[1:].sum() > 0
        cg, cs = graph.current_read(), single.current_read()
        assert cg.samples == cs.samples == 20 and np.array_equal(cg.words, cs.words)
        mg, ms = graph.msd_read(), single.msd_read()
        assert mg.samples == ms.samples == 13 and np.array_equal(mg.words, ms.words)
        rg, rs = graph.rdf_read(), single.rdf_read()
        assert rg.samples == rs.samples == 10 and np.array_equal(rg.counts, rs.counts) and rg.counts.sum() > 0
        pg, ps = graph.profile_read(), single.profile_read()
        assert pg.samples == ps.samples == 16 and np.array_equal(pg.words, ps.words)
        fg, fs = graph.frames_read(), single.frames_read()
        assert list(fg.step) == list(fs.step) == list(range(3, 181, 3)) and eq(fg.positions, fs.positions) and eq(fg.velocities, fs.velocities)
        rows = [c.series_read() for c in (graph, single, truth)]
        for r in rows:
            assert list(r.step) == list(range(7, 181, 7)) and r.dropped == 0
        recs = [c.cm_motion_record() for c in (graph, single, truth)]
        assert [r.removals for r in recs] == [36, 36, 36]
        K.assert_same(K.state(graph), K.state(single), "replays against single steps")
    finally:
        for c in (graph, single, truth):
            c.close()


# ------------------------------------------------------------------------------------------ 5. max_samples, reset, num_lags = 0
def test_max_samples_reset_and_the_static_table():
    spec = spec_for("C3")
    groups, w = groups_for("C3", spec), np.asarray(spec.charges, dtype=np.float64)
    (it1, ctx), (it2, static) = make("C3", spec), make("C3", spec)
    try:
        ctx.frames_start(10, capacity=16, float64=True)
        ctx.modes_start(10, MODES[:9], num_lags=4, origin_every=2, weights=w, groups=groups, max_samples=5)
        lay = ctx.modes_info()
        static.modes_start(10, MODES[:9], num_lags=0, weights=w, groups=groups, max_samples=5)
        sl = static.modes_info()
        assert (sl.num_origins, sl.ring_bytes, sl.words) == (0, 0, MR.row_words(2, 9))
        ctx.run_graph(100, 50)
        static.run_graph(100, 50)
        dm = ctx.modes_read(reset=True)
        f = ctx.frames_read()
        assert (dm.samples, dm.dropped) == (5, 5) and list(f.step) == list(range(10, 101, 10))
        assert_equal(dm, expected(f, w, groups, lay, MODES[:9], which=range(5)))
        assert np.array_equal(dm.count, MR.lag_counts(5, 2, 4))
        st = static.modes_read()
        assert (st.samples, st.dropped) == (5, 5) and st.words.shape == (1, MR.row_words(2, 9))
        assert np.array_equal(st.words[0], dm.words[0]) and eq(st.box_sum, dm.box_sum)      # S(k) only: row 0 of the run with lags
        z = ctx.modes_read()
        assert (z.samples, z.dropped, z.out_of_range, z.invalid_samples, z.origin_floor) == (0, 0, 0, 0, 0) and not z.words.any() and not z.box_sum.any()
        # the schedule continues without gap or repeat; the ordinal restarts at 0 with no live origin (the ring still holds the old sums)
        ctx.run_graph(40, 50)
        t, f = ctx.modes_read(), ctx.frames_read()
        assert list(f.step[10:]) == [110, 120, 130, 140] and (t.samples, t.dropped) == (4, 0)
        assert_equal(t, expected(f, w, groups, lay, MODES[:9], which=range(10, 14)))
        assert np.array_equal(t.count, MR.lag_counts(4, 2, 4))
    finally:
        ctx.close()
        static.close()


# ------------------------------------------------------------------------------------------ 6. a NaN position
def test_a_nan_position_makes_the_sample_invalid_and_no_origin():
    """Two valid samples, then one recorded particle's x is NaN for the next two (whatever else the NaN does to the run, the frames say
    which particles are out of range), then positions, velocities and the thermostat are put back and three more samples are valid: none
    of them may use sample 2 or 3 as an origin."""
    spec = spec_for("C1")
    n = spec.num_atoms
    groups = np.where(np.arange(n) % 3 == 0, 0, -1).astype(np.int8)
    w = np.asarray(spec.charges, dtype=np.float64)
    it, ctx = make("C1", spec, precision="double")
    try:
        ctx.frames_start(10, capacity=16, float64=True)
        ctx.modes_start(10, MODES[:8], num_lags=4, origin_every=1, weights=w, groups=groups, max_samples=100)
        lay = ctx.modes_info()
        ctx.run_graph(20, 10)
        saved = (ctx.getPosq(), ctx.getVelm(), ctx.getNHState())
        posq = saved[0].copy()
        posq[9, 0] = np.nan
        ctx.posq.upload(posq)
        ctx.forces_valid = False
        ctx.run_graph(20, 10)
        ctx.synchronize()
        ctx.posq.upload(saved[0])
        ctx.velm.upload(saved[1])
        ctx.setNHState(saved[2])
        ctx.forces_valid = False
        ctx.run_graph(30, 10)
        dm, f = ctx.modes_read(), ctx.frames_read()
        want = expected(f, w, groups, lay, MODES[:8])
        bad = [int(np.count_nonzero(~np.all(np.abs(f.positions[j][groups >= 0]) < 64.0, axis=1))) for j in range(7)]
        assert bad[0] == bad[1] == 0 and bad[2] >= 1 and bad[3] >= 1 and bad[4:] == [0, 0, 0], bad      # the premise
        assert (dm.samples, dm.dropped, dm.invalid_samples, dm.out_of_range) == (7, 0, 2, bad[2] + bad[3])
        assert_equal(dm, want)
        assert list(dm.count) == [5, 3, 1, 1, 2]                      # valid: 0, 1, 4, 5, 6.  Lag 1: (0,1) (4,5) (5,6); lag 2: (4,6), not (2,4) or (3,5); lag 3: (1,4); lag 4: (0,4) (1,5)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 7. the barostat
def test_barostat_moves_set_the_origin_floor_and_the_modes_follow_the_box():
    spec = spec_for("C3")
    groups, w = groups_for("C3", spec), np.asarray(spec.charges, dtype=np.float64)
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(10, capacity=32, float64=True)
        ctx.modes_start(10, MODES[:10], num_lags=8, origin_every=1, weights=w, groups=groups, max_samples=100)
        lay = ctx.modes_info()
        ctx.run_graph(50, 50)                                       # samples 0 .. 4
        before = ctx.modes_read()
        assert (before.samples, before.origin_floor) == (5, 0)
        ctx.scale_box((1.01, 0.99, 1.02))
        after = ctx.modes_read()
        assert (after.samples, after.origin_floor) == (5, 5) and np.array_equal(after.words, before.words)      # the table is kept
        ctx.run_graph(40, 20)                                       # samples 5 .. 8, with the new box's wave vectors (the graphs are re-captured)
        assert ctx.modes_read().origin_floor == 5
        ctx.scale_box((1.05, 1.05, 1.05))
        assert ctx.modes_read().origin_floor == 9
        ctx.restore_box()
        ctx.run_graph(30, 10)                                       # samples 9 .. 11
        ctx.scale_box((0.99, 0.99, 0.99))
        ctx.restore_box()
        ctx.run_eager(30)                                           # samples 12 .. 14
        dm, f = ctx.modes_read(), ctx.frames_read()
        assert (dm.samples, dm.origin_floor, dm.out_of_range) == (15, 12, 0) and list(f.step) == list(range(10, 151, 10))
        floors = [0] * 5 + [5] * 4 + [9] * 3 + [12] * 3
        assert_equal(dm, expected(f, w, groups, lay, MODES[:10], floor=floors))
        assert len(set(map(tuple, f.box))) > 1                       # (the box differs between the samples: so do inv_L and box_sum)
        assert dm.count[0] == 15 and 0 < dm.count[1:].sum() < MR.lag_counts(15, 1, 8)[1:].sum()
        assert np.allclose(dm.mean_box, f.box.mean(axis=0), rtol=1e-14)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 8. recovery
def test_a_repair_puts_table_and_ring_back_with_the_step_counter():
    """vvhip_debug_recover repairs on request: the snapshot of the run call goes back -- the recorder's whole allocation, sums, table and
    ring of origins, with the step counter -- and the call is repeated.  A ring of two slots is overwritten five times inside the repeated
    window."""
    spec = spec_for("C3")
    groups, w = groups_for("C3", spec), np.asarray(spec.charges, dtype=np.float64)
    (it1, rec), (it2, calm) = make("C3", spec), make("C3", spec)
    try:
        for c in (rec, calm):
            c.run_graph(50, 50)
            c.modes_start(10, MODES[:10], num_lags=2, origin_every=1, weights=w, groups=groups, max_samples=100)
            c.run_graph(30, 10)                                     # three samples before the snapshot
            c.synchronize()
        assert rec.modes_info().num_origins == 2
        assert rec.fused_status()[0] and rec.recovery_count() == 0
        rec.run_graph(100, 50)
        calm.run_graph(100, 50)
        H.check(H.lib.vvhip_debug_recover(rec.plan), rec.plan)
        assert rec.recovery_count() == 1 and not rec.fused_status()[0] and rec.status_words() == [0, 0, 0, 0]
        m, q = rec.modes_read(), calm.modes_read()
        assert (m.samples, m.dropped, m.out_of_range, m.invalid_samples, m.origin_floor) == (q.samples, q.dropped, q.out_of_range, q.invalid_samples, q.origin_floor) == (13, 0, 0, 0, 0)
        assert np.array_equal(m.words, q.words) and m.count[1:].sum() > 0 and eq(m.box_sum, q.box_sum)
        assert same_bits(state(rec), state(calm))
    finally:
        rec.close()
        calm.close()


# ------------------------------------------------------------------------------------------ 9. stop, the checkpoint, a sharded plan
def test_stop_and_the_checkpoint():
    spec = spec_for("C3")
    (it1, rec), (it2, plain) = make("C3", spec), make("C3", spec)
    try:
        rec.modes_start(10, MODES[:5], num_lags=8, origin_every=3, max_samples=100)
        rec.run_graph(100, 50)
        plain.run_graph(100, 50)
        assert rec.modes_read().samples == 10
        blob = plain.createCheckpoint()
        with pytest.raises(H.VVHipError) as e:
            rec.loadCheckpoint(blob)
        assert e.value.code == H.ERR_INVALID and "a density-mode recorder is running: stop it, load, start it again" in str(e.value)
        rec.modes_stop()
        info = rec.modes_info()
        assert info.active == 0 and info.words == 0
        with pytest.raises(H.VVHipError):
            rec.modes_read()
        # stopped: further steps as if there never was a recorder; then stop, load, start works
        rec.run_graph(50, 50)
        plain.run_graph(50, 50)
        assert same_bits(state(rec), state(plain))
        rec.loadCheckpoint(blob)
        rec.modes_start(10, MODES[:5], num_lags=8, origin_every=3, max_samples=100)
        assert rec.modes_info().active == 1 and rec.modes_info().start_step == 100
    finally:
        rec.close()
        plain.close()


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
            ctx.modes_start(10, MODES[:5], num_lags=3)
        assert e.value.code == H.ERR_UNSUPPORTED and "shard" in str(e.value)
        assert live() == before and ctx.modes_info().active == 0
    finally:
        ctx.close()
