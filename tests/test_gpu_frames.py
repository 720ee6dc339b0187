"""Trajectory frames (include/vvhip.h: vvhip_frames_*) on the GPU: frames recorded inside graph replays are the positions and velocities a
second context downloads at the same steps, bit for bit, and leave the run untouched; one schedule, linear or logarithmic, on the three
stepping paths and a graph cache that settles; capacity, draining and the guard frame; subsets, tails and capped grids; shards; the recorder
next to a series and scheduled removals of the centre-of-mass motion; stop and the checkpoint."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import checkpoint_cases as K     # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S, I = pkg.systems, pkg.integrator
H = I.H

pytestmark = pytest.mark.gpu

NH_FIELDS = ("eta", "eta_dot", "eta_dotdot", "ke2", "vscale", "v_bias")
SCALE = {"C1": 1.0, "C3": 0.1, "C5": 0.25}


def spec_for(cfg):
    if cfg == "VS":      # a polarisable liquid with a lone pair and a two-particle average per molecule, stored behind the last real particle
        return S.add_virtual_sites(S.drude_il(cells=(1, 1, 1), pairs_per_cell=16, seed=4), kinds=(3, 0), interleaved=False)
    return S.make_config(cfg, scale=SCALE[cfg])


def integrator_for(cfg, spec, middle=True):
    it = I.VVIntegrator(333.0, 10.0, 1.0, 40.0, 0.001, 3, 1)
    if cfg != "C1":
        it.setMaxDrudeDistance(0.02)
    if cfg == "C5":
        lz = float(spec.box[2])
        it.setMirrorLocation(lz / 2)
        it.setElectricField(2.0 / lz * 2 * 1.602176634e-22)
    it.setUseMiddleScheme(middle)
    return it


def make(cfg, spec, precision="mixed", middle=True, **kw):
    it = integrator_for(cfg, spec, middle)
    return it, I.Context(spec, it, precision=precision, force_provider="tether", **kw)


def state(ctx):
    st = ctx.getNHState()
    return [ctx.getPosq(), ctx.getPosqCorrection(), ctx.getVelm()] + [np.array(getattr(st, f)) for f in NH_FIELDS]


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def eq(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def frames_equal(a, b):
    if list(a.step) != list(b.step) or a.dropped != b.dropped or not eq(a.box, b.box) or not eq(a.particles, b.particles):
        return False
    for f in ("positions", "velocities"):
        x, y = getattr(a, f), getattr(b, f)
        if (x is None) != (y is None) or (x is not None and not eq(x, y)):
            return False
    return True


def guard_intact(ctx):
    ok = C.c_int32(0)
    H.check(H.lib.vvhip_debug_frames_guard(ctx.plan, C.byref(ok)), ctx.plan)
    return ok.value == 1


# ------------------------------------------------------------------------------------------ 1. frames inside replays are the state at those steps
CASES = [("C1", "mixed", True), ("C3", "mixed", True), ("C5", "mixed", True), ("C3", "single", True), ("C3", "double", True),
         ("C3", "mixed", False), ("VS", "mixed", True)]


@pytest.mark.parametrize("cfg,precision,middle", CASES, ids=[f"{c}-{p}-{'middle' if m else 'classic'}" for c, p, m in CASES])
def test_frames_inside_replays_are_the_state_at_those_steps(cfg, precision, middle):
    spec = spec_for(cfg)
    k, chunks = 50, 6
    if cfg == "C5":
        assert len(spec.image_pairs) > 0                           # image particles: no lane of their own
    if cfg == "VS":
        assert len(spec.virtual_sites) > 0
    ctxs = [make(cfg, spec, precision, middle)[1] for _ in range(3)]
    rec64, rec32, ref = ctxs
    try:
        rec64.frames_start(k, capacity=8, velocities=True, float64=True)
        rec32.frames_start(k, capacity=8, velocities=True)
        rec64.run_graph(k * chunks, 50)
        rec32.run_graph(k * chunks, 50)
        f64, f32 = rec64.frames_read(), rec32.frames_read()
        assert f64.positions.dtype == np.float64 and f32.positions.dtype == np.float32
        for f in (f64, f32):
            assert list(f.step) == [k * (j + 1) for j in range(chunks)] and f.dropped == 0
            assert eq(f.particles, np.arange(spec.num_atoms, dtype=np.int32))
            assert eq(f.box, np.tile(np.asarray(spec.box, dtype=np.float64), (chunks, 1)))
        for j in range(chunks):
            # (a Langevin subset draws its numbers from a refill at the head of every graph: the per-call context replays the same graphs)
            if cfg == "C5":
                ref.run_graph(k, 50)
            else:
                ref.run_eager(k)
            x, v = ref.getPositions(), ref.getVelocities()
            assert eq(f64.positions[j], x) and eq(f64.velocities[j], v), j
            assert eq(f32.positions[j], x.astype(np.float32)) and eq(f32.velocities[j], v.astype(np.float32)), j
        assert guard_intact(rec64) and guard_intact(rec32)
        # the recorder changes nothing of the run
        assert same_bits(state(rec64), state(ref)) and same_bits(state(rec32), state(ref))
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------------------------------ 2. one schedule on every path
def _scheduled(path, interval, logarithmic, n=317):
    spec = spec_for("C3")
    it, ctx = make("C3", spec)
    try:
        it.step(3)                                                  # an unaligned start, host-driven
        ctx.frames_start(interval, capacity=64, logarithmic=logarithmic, velocities=True)
        assert ctx.frames_info().start_step == 3
        if path == "step":
            it.step(n)
        elif path == "eager":
            ctx.run_eager(n)
        else:
            ctx.run_graph(n, 50)
        return ctx.frames_read()
    finally:
        ctx.close()


@pytest.mark.parametrize("interval,logarithmic", [(7, False), (50, False), (30, True)], ids=["linear-7", "linear-50", "log10-30"])
def test_schedule_is_the_same_on_every_stepping_path(interval, logarithmic):
    g = _scheduled("graph", interval, logarithmic)
    want = H.frames_steps(interval, 3, 320, logarithmic)
    assert len(want) > 0 and list(g.step) == list(want) and g.dropped == 0
    for path in ("step", "eager"):
        assert frames_equal(g, _scheduled(path, interval, logarithmic)), path


@pytest.mark.parametrize("interval,logarithmic", [(50, False), (10, True)], ids=["linear-50", "log10-10"])
def test_steady_state_replays_capture_nothing(interval, logarithmic):
    spec = spec_for("C3")
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(interval, capacity=64, logarithmic=logarithmic)
        ctx.run_graph(2000, 50)
        before = ctx.series_info().graph_captures
        ctx.run_graph(1000, 50)
        assert ctx.series_info().graph_captures == before, (before, ctx.series_info().graph_captures)
        f = ctx.frames_read()
        assert list(f.step) == list(H.frames_steps(interval, 0, 3000, logarithmic)) and f.dropped == 0
        assert eq(f.positions[-1], ctx.getPositions().astype(np.float32))       # the frame after step 3000 is the state as it stands
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 3. capacity
def test_capacity_drops_frames_and_nothing_is_written_past_it():
    spec = spec_for("C3")
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(10, capacity=5)
        ctx.run_graph(100, 50)
        f = ctx.frames_read()
        assert list(f.step) == [10, 20, 30, 40, 50] and f.dropped == 5 and f.positions.shape == (5, spec.num_atoms, 3)
        assert guard_intact(ctx)
        # drained: the next frames continue after the dropped ones' steps (those are gone), without a repeat
        ctx.frames_read(reset=True)
        ctx.run_graph(40, 50)
        t = ctx.frames_read()
        assert list(t.step) == [110, 120, 130, 140] and t.dropped == 0
        assert eq(t.positions[-1], ctx.getPositions().astype(np.float32))
        assert guard_intact(ctx)
    finally:
        ctx.close()


def test_reading_with_reset_in_the_middle_continues_the_recording():
    spec = spec_for("C3")
    it1, ctx1 = make("C3", spec)
    it2, ctx2 = make("C3", spec)
    try:
        ctx1.frames_start(30, capacity=32, logarithmic=True, velocities=True)
        ctx2.frames_start(30, capacity=32, logarithmic=True, velocities=True)
        pieces = []
        for n in (150, 150, 100):
            ctx1.run_graph(n, 50)
            pieces.append(ctx1.frames_read(reset=True))
        ctx2.run_graph(400, 50)
        whole = ctx2.frames_read()
        assert list(np.concatenate([p.step for p in pieces])) == list(whole.step) == [30, 40, 50, 60, 70, 80, 90, 100, 200, 300, 400]
        for f in ("box", "positions", "velocities"):
            assert eq(np.concatenate([getattr(p, f) for p in pieces]), getattr(whole, f)), f
    finally:
        ctx1.close()
        ctx2.close()


# ------------------------------------------------------------------------------------------ 4. subsets and tails
_FULL = {}


def _full_c1():
    """Every particle of C1 (1 992: no multiple of 16, 64 or 512) with the default launch shape, computed once: (spec, frames)."""
    if "f" not in _FULL:
        spec = spec_for("C1")
        assert spec.num_atoms % 16 != 0 and spec.num_atoms % 64 != 0 and spec.num_atoms % 512 != 0
        it, ctx = make("C1", spec)
        try:
            ctx.frames_start(25, capacity=4, velocities=True)
            ctx.run_graph(100, 50)
            _FULL["f"] = (spec, ctx.frames_read())
        finally:
            ctx.close()
    return _FULL["f"]


@pytest.mark.parametrize("tune", [None, {"grid_cap_a": 1}, {"block_threads": 128}], ids=["default", "grid_cap_a-1", "block_threads-128"])
def test_subsets_and_tails(tune):
    spec, full = _full_c1()
    n = spec.num_atoms
    assert list(full.step) == [25, 50, 75, 100]
    rng = np.random.default_rng(17)
    third = np.sort(rng.choice(n, size=n // 3, replace=False))
    subsets = [None, [n - 1], list(range(3, 3 + 65)), third]
    for sub in subsets:
        for velocities in (False, True):
            it, ctx = make("C1", spec, tune=tune)
            try:
                ctx.frames_start(25, capacity=4, subset=sub, velocities=velocities)
                ctx.run_graph(100, 50)
                f = ctx.frames_read()
                assert guard_intact(ctx)
            finally:
                ctx.close()
            idx = np.arange(n) if sub is None else np.asarray(sub)
            assert list(f.step) == list(full.step) and eq(f.particles, idx.astype(np.int32)), (sub is None, velocities)
            assert eq(f.positions, full.positions[:, idx]), (len(idx), velocities)
            assert (f.velocities is None) if not velocities else eq(f.velocities, full.velocities[:, idx]), (len(idx), velocities)


# ------------------------------------------------------------------------------------------ 5. shards
def test_shards_record_their_own_particles():
    spec = spec_for("C3")
    n = spec.num_atoms
    mol = np.asarray(spec.mol_id)
    cut = int(np.nonzero(mol == mol[n // 2])[0].min())             # a molecule boundary
    assert 0 < cut < n and mol[cut - 1] != mol[cut]
    for shard in ((0, cut), (cut, n)):
        it = integrator_for("C3", spec)
        it.setUseCOMTempGroup(False)
        ctx = I.Context(spec, it, precision="mixed", force_provider="tether", shard=shard)
        try:
            ctx.frames_start(10, capacity=8, velocities=True, float64=True)
            want = []
            for _ in range(3):
                ctx.run_eager(10)
                want.append((ctx.getPositions(), ctx.getVelocities()))
            f = ctx.frames_read()
            assert list(f.step) == [10, 20, 30] and eq(f.particles, np.arange(shard[0], shard[1], dtype=np.int32))
            for j, (x, v) in enumerate(want):
                assert x.shape == (shard[1] - shard[0], 3) and eq(f.positions[j], x) and eq(f.velocities[j], v), (shard, j)
            # a subset that straddles the cut: this shard's part of it, as global indices
            sub = np.arange(cut - 40, cut + 25)
            ctx.frames_start(10, capacity=8, subset=sub)
            ctx.run_eager(10)
            g = ctx.frames_read()
            mine = sub[(sub >= shard[0]) & (sub < shard[1])]
            assert list(g.step) == [40] and eq(g.particles, mine.astype(np.int32))
            assert eq(g.positions[0], ctx.getPositions()[mine - shard[0]].astype(np.float32))
            # a subset that lies wholly in the other shard: frames without particles, at the right steps
            other = np.arange(cut, cut + 10) if shard[0] == 0 else np.arange(5, 15)
            ctx.frames_start(10, capacity=2, subset=other, velocities=True)
            ctx.run_eager(35)
            e = ctx.frames_read()
            assert list(e.step) == [50, 60] and e.dropped == 1 and e.positions.shape == (2, 0, 3) and e.velocities.shape == (2, 0, 3)
            assert len(e.particles) == 0 and guard_intact(ctx)
        finally:
            ctx.close()


# ------------------------------------------------------------------------------------------ 6. together with the rest
def test_recorder_next_to_a_series_and_scheduled_removals():
    spec = spec_for("C3")
    assert spec.has_cm_motion_remover
    ctxs = [make("C3", spec)[1] for _ in range(3)]
    rec, plain, short = ctxs
    try:
        for c in ctxs:
            c.series_start(20, capacity=16)
            c.remove_cm_motion_every(10)
        rec.frames_start(20, capacity=16, velocities=True, float64=True)
        rec.run_graph(200, 50)
        plain.run_graph(200, 50)
        f, a, b = rec.frames_read(), rec.series_read(), plain.series_read()
        assert list(f.step) == list(a.step) == list(b.step) == list(range(20, 201, 20)) and f.dropped == 0
        for name in ("raw", "ke", "t", "box") + NH_FIELDS:
            assert eq(getattr(a, name), getattr(b, name)), name
        ra, rb = rec.cm_motion_record(), plain.cm_motion_record()
        assert ra.removals == rb.removals == 20 and ra.skipped == rb.skipped == 0 and list(ra.last_v) == list(rb.last_v)
        # the frame after step 20: the state after 20 steps, before the removal in front of step 21 touches the velocities
        short.run_graph(20, 20)
        assert eq(f.positions[0], short.getPositions()) and eq(f.velocities[0], short.getVelocities())
        assert short.cm_motion_record().removals == 2
        # loading a checkpoint while the recorder runs is refused as with a series running; after the stop it works
        plain.series_stop()
        blob = plain.createCheckpoint()
        rec.series_stop()
        with pytest.raises(H.VVHipError) as e:
            rec.loadCheckpoint(blob)
        assert e.value.code == H.ERR_INVALID and "a frame recorder is running: stop it, load, start it again" in str(e.value)
        rec.frames_stop()
        info = rec.frames_info()
        assert info.active == 0 and info.frame_bytes == 0
        with pytest.raises(H.VVHipError):
            rec.frames_read()
        rec.loadCheckpoint(blob)
        assert same_bits(state(rec), state(plain))
        # stopped: further steps as if there never was a recorder
        rec.run_graph(100, 50)
        rec.run_eager(13)
        plain.run_graph(100, 50)
        plain.run_eager(13)
        assert same_bits(state(rec), state(plain))
        assert rec.cm_motion_record().removals == plain.cm_motion_record().removals
    finally:
        for c in ctxs:
            c.close()


def test_three_riders_with_windows_that_shift_between_replays():
    """Series every 7, removals every 5, frames on the logarithmic schedule from 3, graphs of 20 steps: no interval divides the graph's
    length, so the replays' windows differ and the cache has to pick (or capture) the graph that fits -- against a context driven one
    vvhip_step_middle at a time."""
    spec = spec_for("C3")
    (it1, graph), (it2, single) = make("C3", spec), make("C3", spec)
    try:
        for c in (graph, single):
            c.series_start(7, capacity=32)
            c.remove_cm_motion_every(5)
            c.frames_start(3, capacity=32, logarithmic=True, velocities=True, float64=True)
        graph.run_graph(130, 20)
        for _ in range(130):
            it2.step(1)
        rows = [[c.series_read(reset=True)] for c in (graph, single)]
        frames = [[c.frames_read(reset=True)] for c in (graph, single)]
        graph.run_eager(3)
        graph.run_graph(47, 20)
        for _ in range(50):
            it2.step(1)
        for k, c in enumerate((graph, single)):
            rows[k].append(c.series_read())
            frames[k].append(c.frames_read())
            assert [r.dropped for r in rows[k]] == [0, 0] and [f.dropped for f in frames[k]] == [0, 0]
            assert list(np.concatenate([r.step for r in rows[k]])) == list(range(7, 181, 7))
            assert list(np.concatenate([f.step for f in frames[k]])) == list(H.frames_steps(3, 0, 180, True))
            ok = C.c_int32(0)
            H.check(H.lib.vvhip_debug_series_guard(c.plan, C.byref(ok)), c.plan)
            assert ok.value == 1 and guard_intact(c)
        assert len(frames[0][0]) == 17 and len(frames[0][1]) == 0          # 3 .. 10, 20 .. 100; the next one is step 200
        for a, b in zip(rows[0], rows[1]):
            for name in ("raw", "ke", "t", "box") + NH_FIELDS:
                assert eq(getattr(a, name), getattr(b, name)), name
        for a, b in zip(frames[0], frames[1]):
            assert frames_equal(a, b)
        ra, rb = graph.cm_motion_record(), single.cm_motion_record()
        assert ra.removals == rb.removals == 36 and ra.skipped == rb.skipped == 0 and list(ra.last_v) == list(rb.last_v)
        # every section's digest, the thermostat's over its copies without the rendezvous wait's self-tuning words (rv_delay / rv_calm follow
        # the timing, not the trajectory: tests/checkpoint_cases.py), and the particle arrays as downloaded
        K.assert_same(K.state(graph), K.state(single), "replays against single steps")
        # The cache neither captures more nor keeps fewer than before the riders' schedules were stated once: 8 is what that commit's
        # library counts for this exact sequence (the six windows of the first call all differ, and so do the two of the last, at the other
        # thermostat parity).
        print("graph_captures", graph.series_info().graph_captures)
        assert graph.series_info().graph_captures == 8
    finally:
        graph.close()
        single.close()


def test_stop_leaves_the_run_as_if_there_never_was_a_recorder():
    spec = spec_for("C3")
    it1, ctx1 = make("C3", spec)
    it2, ctx2 = make("C3", spec)
    try:
        ctx1.frames_start(10, capacity=4, velocities=True)
        ctx1.run_graph(200, 50)
        assert len(ctx1.frames_read()) == 4
        ctx1.frames_stop()
        ctx1.run_graph(200, 50)
        ctx1.run_eager(13)
        ctx2.run_graph(400, 50)
        ctx2.run_eager(13)
        assert same_bits(state(ctx1), state(ctx2))
        # restarting drops what was recorded and begins at the step count as it stands
        ctx1.frames_start(10, capacity=4)
        assert ctx1.frames_info().start_step == 413 and len(ctx1.frames_read()) == 0
        ctx1.run_eager(7)
        ctx2.run_eager(7)
        f = ctx1.frames_read()
        assert list(f.step) == [420] and eq(f.positions[0], ctx2.getPositions().astype(np.float32))
    finally:
        ctx1.close()
        ctx2.close()
