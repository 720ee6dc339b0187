"""Device-side profiles (include/vvhip.h: vvhip_profile_*) on the GPU.  The ground truth needs no second definition: the same context also
runs the frame recorder (float64, with velocities) at the same interval, and the expected table is the sum over those frames of
tests/profile_reference.py with the charges of posq.w and the System's masses.  Every comparison is np.array_equal on int64."""
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
import profile_reference as PR   # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S, I, D = pkg.systems, pkg.integrator, pkg.distributed
H = I.H

pytestmark = pytest.mark.gpu

NH_FIELDS = ("eta", "eta_dot", "eta_dotdot", "ke2", "vscale", "v_bias")
SCALE = {"C1": 1.0, "C3": 0.1, "C5": 0.25}
ALL = dict(charge=True, mass=True, momentum=True, kinetic=True)
_SPECS = {}


def spec_for(cfg):
    if cfg not in _SPECS:
        _SPECS[cfg] = S.make_config(cfg, scale=SCALE[cfg])
    return _SPECS[cfg]


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


def groups_for(cfg, spec):
    """{Drude, non-Drude}; for C5 {electrode, ions, images -> -1}."""
    n = spec.num_atoms
    if cfg == "C5":
        g = np.full(n, -1, dtype=np.int8)
        g[np.asarray(spec.particles_ld, dtype=int)] = 0
        g[np.asarray(spec.particles_electrolyte, dtype=int)] = 1
        assert len(spec.image_pairs) > 0 and np.all(g[[a for a, _ in spec.image_pairs]] == -1)
        return g
    g = np.ones(n, dtype=np.int8)
    if len(spec.drude_pairs):
        g[np.asarray(spec.drude_pairs)[:, 0]] = 0
    return g


def state(ctx):
    st = ctx.getNHState()
    return [ctx.getPosq(), ctx.getPosqCorrection(), ctx.getVelm()] + [np.array(getattr(st, f)) for f in NH_FIELDS]


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def eq(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def expected(frames, spec, charges, groups, lay, which=None):
    """(sum over the frames `which` (all) of the reference's table, of its out-of-range count) for the layout `lay`."""
    idx = np.asarray(frames.particles, dtype=int)
    masses = np.asarray(spec.masses, dtype=np.float64)[idx]
    g = None if groups is None else np.asarray(groups)[idx]
    table, out = np.zeros((lay.num_groups, lay.rows, lay.nbins), dtype=np.int64), 0
    for j in (range(len(frames)) if which is None else which):
        t, o = PR.profile_reference(frames.positions[j], frames.velocities[j], charges, masses, g, frames.box[j], lay, list(lay.frac_bits))
        table += t
        out += o
    return table, out


def charges_of(ctx):
    return ctx.getPosq()[:, 3].astype(np.float64)


# ------------------------------------------------------------------------------------------ 1. the table is the sum over the frames
CASES = [("C1", "mixed", True), ("C3", "mixed", True), ("C5", "mixed", True), ("C3", "single", True), ("C3", "double", True), ("C3", "mixed", False)]


@pytest.mark.parametrize("cfg,precision,middle", CASES, ids=[f"{c}-{p}-{'middle' if m else 'classic'}" for c, p, m in CASES])
def test_table_equals_the_sum_over_frames(cfg, precision, middle):
    spec = spec_for(cfg)
    groups = groups_for(cfg, spec)
    (_, rec), (_, plain) = make(cfg, spec, precision, middle), make(cfg, spec, precision, middle)
    try:
        rec.frames_start(10, capacity=32, velocities=True, float64=True)
        rec.profile_start(10, 64, axis=2, groups=groups, max_samples=1000, **ALL)
        lay = rec.profile_info()
        assert (lay.active, lay.rows, lay.num_groups, lay.words) == (1, 7, int(groups.max()) + 1, (int(groups.max()) + 1) * 7 * 64)
        assert lay.num_particles == np.count_nonzero(groups >= 0) and min(list(lay.frac_bits)[1:]) >= 8
        rec.run_graph(300, 50)
        plain.run_graph(300, 50)
        p, f = rec.profile_read(), rec.frames_read()
        assert list(f.step) == list(range(10, 301, 10))
        want, want_out = expected(f, spec, charges_of(rec), groups, lay)
        assert (p.samples, p.dropped, p.out_of_range) == (30, 0, 0) and want_out == 0
        assert p.words.dtype == np.int64 and np.array_equal(p.words, want)
        assert p.words[:, 0].sum() == 30 * lay.num_particles
        if cfg == "C5":                                            # the ions sit between the electrode and the mirror plane
            assert p.count[1][: 32].sum() == p.count[1].sum() > 0
        # the recorder changes nothing of the run
        assert same_bits(state(rec), state(plain))
    finally:
        rec.close()
        plain.close()


# ------------------------------------------------------------------------------------------ 2. both add paths and the shapes
# C1 (1 992 particles: no multiple of 16, 64 or 512); every description takes the next 100 steps of one context per tune, which records
# its own frames beside it.
LDS_WORDS = 64 * 1024 // 8


def _descriptions(n):
    rng = np.random.default_rng(17)
    two = (np.arange(n) % 2).astype(np.int8)
    out = [dict(nbins=nb, axis=2, groups=two) for nb in (1, 63, 64, 1000)]
    out += [dict(nbins=585, axis=2, groups=two), dict(nbins=586, axis=2, groups=two)]      # the last table that fits the LDS copy, the first that does not
    out += [dict(nbins=4096, axis=2, groups=two), dict(nbins=64, axis=0, groups=two), dict(nbins=64, axis=1, groups=two), dict(nbins=64, axis=2, groups=None)]
    last, run, third = np.full(n, -1, dtype=np.int8), np.full(n, -1, dtype=np.int8), np.full(n, -1, dtype=np.int8)
    last[n - 1] = 0
    run[3:3 + 65] = np.arange(65) % 2
    third[rng.choice(n, size=n // 3, replace=False)] = 1
    out += [dict(nbins=64, axis=2, groups=g) for g in (last, run, third)]
    return out


_FIRST = []      # per tune: (frames of the first description's steps, its table)


@pytest.mark.parametrize("tune", [None, {"grid_cap_a": 1}, {"block_threads": 128}], ids=["default", "grid_cap_a-1", "block_threads-128"])
def test_both_add_paths_and_the_shapes(tune):
    spec = spec_for("C1")
    n = spec.num_atoms
    assert n % 16 != 0 and n % 64 != 0 and n % 512 != 0
    descriptions = _descriptions(n)
    assert 2 * 7 * 585 <= LDS_WORDS < 2 * 7 * 586 and 2 * 7 * 4096 * 8 > 64 * 1024
    it, ctx = make("C1", spec, tune=tune)
    try:
        ctx.frames_start(25, capacity=4 * len(descriptions), velocities=True, float64=True)
        charges = charges_of(ctx)
        for k, d in enumerate(descriptions):
            ctx.profile_start(25, d["nbins"], axis=d["axis"], groups=d["groups"], max_samples=100, **ALL)
            lay = ctx.profile_info()
            assert lay.start_step == 100 * k and lay.num_particles == (n if d["groups"] is None else np.count_nonzero(d["groups"] >= 0))
            ctx.run_graph(100, 50)
            p, frames = ctx.profile_read(), ctx.frames_read()
            want, want_out = expected(frames, spec, charges, d["groups"], lay, which=range(4 * k, 4 * k + 4))
            assert list(frames.step[4 * k:]) == [100 * k + 25 * (j + 1) for j in range(4)]
            assert (p.samples, p.dropped, p.out_of_range) == (4, 0, want_out) and want_out == 0, (k, p.samples, p.out_of_range)
            assert np.array_equal(p.words, want), (k, d["nbins"], d["axis"])
            assert p.words[:, 0].sum() == 4 * lay.num_particles
            if k == 0:
                _FIRST.append((frames.positions[:4].copy(), frames.velocities[:4].copy(), p.words))
        # ... and for the first description equal to each other across the tunes: the same inputs (the launch shapes of the step give the
        # same trajectory bits over these 100 steps, as tests/test_gpu_frames.py finds; later they part in the last bits), the same table
        for x, v, words in _FIRST:
            assert eq(x, _FIRST[0][0]) and eq(v, _FIRST[0][1]) and np.array_equal(words, _FIRST[0][2])
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 3. the edges of the binning
@pytest.mark.parametrize("precision", ["mixed", "double"])
def test_edges_of_the_binning(precision):
    """One particle exactly on every 5th bin edge (0 and L included), one at -1e-20, one 400 boxes out, one at -0.5 box, planted before the
    first step with zero velocity on their own tether sites, so that the one step (dt at its smallest, 1e-5 ps) leaves them where they are."""
    spec = spec_for("C1")
    nbins, axis = 64, 2
    length = float(spec.box[axis])
    planted = [k * (length / nbins) for k in range(0, nbins + 1, 5)] + [-1e-20, 400 * length + 0.37 * length, -0.5 * length, np.nextafter(length, 0.0)]
    it, ctx = make("C1", spec, precision, dt=1e-5)
    try:
        posq, corr, velm = ctx.getPosq(), ctx.getPosqCorrection(), ctx.getVelm()
        idx = np.arange(len(planted)) * 7 + 3
        posq[idx, axis] = np.asarray(planted).astype(posq.dtype)
        if precision == "mixed":
            corr[idx, axis] = (np.asarray(planted) - posq[idx, axis].astype(np.float64)).astype(corr.dtype)
        velm[idx, :3] = 0.0
        ctx.posq.upload(posq)
        ctx.posq_corr.upload(corr)
        ctx.site.upload(posq)
        ctx.velm.upload(velm)
        ctx.frames_start(1, capacity=2, velocities=True, float64=True)
        ctx.profile_start(1, nbins, axis=axis, max_samples=4, **ALL)
        lay = ctx.profile_info()
        it.step(1)
        p, f = ctx.profile_read(), ctx.frames_read()
        assert p.samples == 1 and list(f.step) == [1]
        want, want_out = expected(f, spec, charges_of(ctx), None, lay)
        assert p.out_of_range == want_out == 0 and np.array_equal(p.words, want)
        # the planted particles have not moved, and sit where the definition puts them
        x = f.positions[0][idx, axis]
        sent = posq[idx, axis].astype(np.float64) + (corr[idx, axis].astype(np.float64) if precision == "mixed" else 0.0)
        assert eq(x, sent)
        b = PR.bins(x, length, nbins)
        j = len(planted) - 4
        assert x[j] < 0 and b[j] == nbins - 1                       # -1e-20: u = 1.0, the last bin by the clamp
        assert b[0] == 0 and 0 <= b.min() and b.max() <= nbins - 1
        if precision == "double":
            assert eq(x, np.asarray(planted))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 4. out of range and capacity
def test_out_of_range_particles_are_absent_from_every_row():
    """C5: the electrode's Mo (95.94) is the heaviest species, three times the next (S, 32.06).  Every particle starts with the same velocity
    v0 along x, v0 = limit / sqrt(m_Mo m_S): m v0 is 73 % above the momentum limit for Mo and 42 % below it for S, and three steps (the
    electrode's Langevin kicks move a velocity by a few per cent) keep it so: exactly the heaviest species is out of range."""
    spec = spec_for("C5")
    groups = groups_for("C5", spec)
    masses = np.asarray(spec.masses, dtype=np.float64)
    kinds = np.unique(masses)
    m1, m2 = kinds[-1], kinds[-2]
    limit = 16.0
    v0 = limit / np.sqrt(m1 * m2)
    assert m1 * v0 > 1.5 * limit and m2 * v0 < limit / 1.5
    heavy = masses == m1
    light = (groups >= 0) & ~heavy
    assert np.all(groups[heavy] == 0) and np.count_nonzero(heavy) > 100
    it, ctx = make("C5", spec)
    try:
        v = np.zeros((spec.num_atoms, 3))
        v[:, 0] = v0
        ctx.setVelocities(v)
        ctx.frames_start(1, capacity=4, velocities=True, float64=True)
        ctx.profile_start(1, 64, groups=groups, max_samples=8, limits={"momentum": limit}, **ALL)
        lay = ctx.profile_info()
        assert lay.limit[3] == limit
        it.step(3)
        p, f = ctx.profile_read(), ctx.frames_read()
        mv = np.abs(masses[None, :, None] * f.velocities)
        assert np.all(mv[:, heavy, 0] >= limit) and np.all(mv[:, light] < limit)      # the premise
        want, want_out = expected(f, spec, charges_of(ctx), groups, lay)
        assert p.samples == 3 and p.out_of_range == want_out == 3 * np.count_nonzero(heavy)
        assert np.array_equal(p.words, want)
        assert p.words[:, 0].sum() == 3 * np.count_nonzero(light)              # absent from the count ...
        light_mass = sum(int(np.rint(m * 2.0 ** lay.frac_bits[2])) for m in masses[light])
        assert int(p.words[:, lay.row_of[2]].sum()) == 3 * light_mass          # ... and from the mass row, whose own term is in range
    finally:
        ctx.close()


def test_capacity_and_reset():
    spec = spec_for("C3")
    groups = groups_for("C3", spec)
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(10, capacity=16, velocities=True, float64=True)
        ctx.profile_start(10, 64, groups=groups, max_samples=5, **ALL)
        lay = ctx.profile_info()
        ctx.run_graph(100, 50)
        p = ctx.profile_read(reset=True)
        f = ctx.frames_read()
        q = charges_of(ctx)
        assert (p.samples, p.dropped) == (5, 5) and list(f.step) == list(range(10, 101, 10))
        assert np.array_equal(p.words, expected(f, spec, q, groups, lay, which=range(5))[0])
        z = ctx.profile_read()
        assert (z.samples, z.dropped, z.out_of_range) == (0, 0, 0) and not z.words.any()
        ctx.run_graph(40, 50)
        t, f = ctx.profile_read(), ctx.frames_read()
        assert list(f.step[10:]) == [110, 120, 130, 140] and (t.samples, t.dropped) == (4, 0)
        assert np.array_equal(t.words, expected(f, spec, q, groups, lay, which=range(10, 14))[0])
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 5. stepping paths and the graph cache
def _scheduled(path, interval, n=317):
    spec = spec_for("C3")
    it, ctx = make("C3", spec)
    try:
        it.step(3)                                                  # an unaligned start, host-driven
        ctx.profile_start(interval, 63, groups=groups_for("C3", spec), max_samples=100, **ALL)
        assert ctx.profile_info().start_step == 3
        if path == "step":
            it.step(n)
        elif path == "eager":
            ctx.run_eager(n)
        else:
            ctx.run_graph(n, 50)
        return ctx.profile_read()
    finally:
        ctx.close()


@pytest.mark.parametrize("interval", [7, 50])
def test_every_stepping_path_gives_the_same_table(interval):
    g = _scheduled("graph", interval)
    assert g.samples == 320 // interval and g.dropped == 0 and g.out_of_range == 0
    for path in ("step", "eager"):
        p = _scheduled(path, interval)
        assert (p.samples, p.dropped, p.out_of_range) == (g.samples, 0, 0) and np.array_equal(p.words, g.words), path


def test_steady_state_replays_capture_nothing():
    spec = spec_for("C3")
    it, ctx = make("C3", spec)
    try:
        ctx.profile_start(50, 64, max_samples=100)
        ctx.run_graph(2000, 50)
        before = ctx.series_info().graph_captures
        ctx.run_graph(1000, 50)
        assert ctx.series_info().graph_captures == before, (before, ctx.series_info().graph_captures)
        p = ctx.profile_read()
        assert p.samples == 60 and p.words[:, 0].sum() == 60 * spec.num_atoms
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 6. shards
def test_shards_tables_add_to_the_unsharded_table():
    """A shard's thermostat sees its own particles' sums only, so a shard and the unsharded run do not take the same step: the states are
    uploaded from one unsharded context, every context then takes ONE step with a sample behind it, and each table is compared with the
    definition on that context's own frame.  The shards' fixed point and limits are the unsharded ones (both follow the description over
    the whole System), so profile_sum of the shards' tables is the table of the definition -- in the unsharded layout -- on the union of
    the shards' particles: what an unsharded recorder adds for that state."""
    spec = spec_for("C3")
    n = spec.num_atoms
    groups = groups_for("C3", spec)
    mol = np.asarray(spec.mol_id)
    cut = int(np.nonzero(mol == mol[n // 2])[0].min())             # a molecule boundary
    assert 0 < cut < n and mol[cut - 1] != mol[cut]
    it0, whole = make("C3", spec)
    shards = []
    try:
        whole.run_eager(20)
        posq, corr, velm = whole.getPosq(), whole.getPosqCorrection(), whole.getVelm()
        whole.frames_start(1, capacity=2, velocities=True, float64=True)
        whole.profile_start(1, 64, groups=groups, max_samples=50, **ALL)
        lay0 = whole.profile_info()
        it0.step(1)
        p0, f0 = whole.profile_read(), whole.frames_read()
        assert p0.samples == 1 and np.array_equal(p0.words, expected(f0, spec, posq[:, 3].astype(np.float64), groups, lay0)[0])
        tables, pos, vel = [], [], []
        for shard in ((0, cut), (cut, n)):
            it = integrator_for("C3", spec)
            it.setUseCOMTempGroup(False)
            ctx = I.Context(spec, it, precision="mixed", force_provider="tether", shard=shard)
            shards.append(ctx)
            sl = slice(*shard)
            ctx.posq.upload(posq[sl]); ctx.posq_corr.upload(corr[sl]); ctx.velm.upload(velm[sl])
            ctx.frames_start(1, capacity=2, velocities=True, float64=True)
            ctx.profile_start(1, 64, groups=groups, max_samples=50, **ALL)
            lay = ctx.profile_info()
            assert lay.num_particles == np.count_nonzero(groups[sl] >= 0) == shard[1] - shard[0]
            assert list(lay.frac_bits) == list(lay0.frac_bits) and list(lay.limit) == list(lay0.limit) and lay.words == lay0.words
            it.step(1)
            p, f = ctx.profile_read(), ctx.frames_read()
            assert p.samples == 1 and eq(f.particles, np.arange(shard[0], shard[1], dtype=np.int32))
            assert np.array_equal(p.words, expected(f, spec, posq[sl, 3].astype(np.float64), groups, lay)[0]), shard
            assert p.words[:, 0].sum() == shard[1] - shard[0]
            tables.append(p)
            pos.append(f.positions[0]); vel.append(f.velocities[0])
        total = D.profile_sum(tables)
        union, _ = PR.profile_reference(np.concatenate(pos), np.concatenate(vel), posq[:, 3].astype(np.float64), np.asarray(spec.masses, dtype=np.float64),
                                        groups, spec.box, lay0, list(lay0.frac_bits))
        assert np.array_equal(total.words, union) and total.words[:, 0].sum() == n and total.out_of_range == 0
    finally:
        whole.close()
        for c in shards:
            c.close()


# ------------------------------------------------------------------------------------------ 7. four riders together
def test_four_riders_with_windows_that_shift_between_replays():
    """Series every 7, removals every 5, frames every 3, profile every 11, graphs of 20 steps: no interval divides the graph's length, so
    the replays' windows differ.  `graph` against `single` (one vvhip_step_middle at a time), all four riders on in both; `truth` has the
    series and the removals on too (the removal changes the trajectory: like with like) and its frames at the profile's steps."""
    spec = spec_for("C3")
    groups = groups_for("C3", spec)
    (it1, graph), (it2, single), (it3, truth) = make("C3", spec), make("C3", spec), make("C3", spec)
    try:
        for c in (graph, single, truth):
            c.series_start(7, capacity=32)
            c.remove_cm_motion_every(5)
        for c in (graph, single):
            c.frames_start(3, capacity=64, velocities=True, float64=True)
            c.profile_start(11, 64, groups=groups, max_samples=100, **ALL)
        truth.frames_start(11, capacity=32, velocities=True, float64=True)
        lay = graph.profile_info()
        graph.run_graph(130, 20)
        graph.run_eager(3)
        graph.run_graph(47, 20)
        for _ in range(180):
            it2.step(1)
        truth.run_graph(180, 20)
        pg, ps = graph.profile_read(), single.profile_read()
        assert (pg.samples, pg.dropped, pg.out_of_range) == (ps.samples, ps.dropped, ps.out_of_range) == (16, 0, 0)
        assert np.array_equal(pg.words, ps.words)
        ft = truth.frames_read()
        assert list(ft.step) == list(range(11, 181, 11))
        assert np.array_equal(pg.words, expected(ft, spec, charges_of(truth), groups, lay)[0])
        fg, fs = graph.frames_read(), single.frames_read()
        assert list(fg.step) == list(fs.step) == list(range(3, 181, 3)) and fg.dropped == fs.dropped == 0
        assert eq(fg.positions, fs.positions) and eq(fg.velocities, fs.velocities)
        assert eq(fg.positions[10::11], ft.positions[2::3]) and eq(fg.velocities[10::11], ft.velocities[2::3])      # (steps 33, 66, ... are both's)
        rows = [c.series_read() for c in (graph, single, truth)]
        for r in rows:
            assert list(r.step) == list(range(7, 181, 7)) and r.dropped == 0
        for name in ("raw", "ke", "t", "box") + NH_FIELDS:
            assert eq(getattr(rows[0], name), getattr(rows[1], name)) and eq(getattr(rows[0], name), getattr(rows[2], name)), name
        recs = [c.cm_motion_record() for c in (graph, single, truth)]
        assert [r.removals for r in recs] == [36, 36, 36] and [r.skipped for r in recs] == [0, 0, 0]
        assert list(recs[0].last_v) == list(recs[1].last_v) == list(recs[2].last_v)
        K.assert_same(K.state(graph), K.state(single), "replays against single steps")
    finally:
        for c in (graph, single, truth):
            c.close()


# ------------------------------------------------------------------------------------------ 8. stop and the checkpoint
def test_stop_and_the_checkpoint():
    spec = spec_for("C3")
    (it1, rec), (it2, plain) = make("C3", spec), make("C3", spec)
    try:
        rec.profile_start(10, 64, max_samples=100, **ALL)
        rec.run_graph(200, 50)
        plain.run_graph(200, 50)
        assert rec.profile_read().samples == 20
        blob = plain.createCheckpoint()
        with pytest.raises(H.VVHipError) as e:
            rec.loadCheckpoint(blob)
        assert e.value.code == H.ERR_INVALID and "a profile recorder is running: stop it, load, start it again" in str(e.value)
        rec.profile_stop()
        info = rec.profile_info()
        assert info.active == 0 and info.words == 0
        with pytest.raises(H.VVHipError):
            rec.profile_read()
        # stopped: further steps as if there never was a recorder
        rec.run_graph(100, 50)
        rec.run_eager(13)
        plain.run_graph(100, 50)
        plain.run_eager(13)
        assert same_bits(state(rec), state(plain))
        # stop, load, start works: the recorder begins at the loaded step counter
        rec.loadCheckpoint(blob)
        plain.loadCheckpoint(blob)
        rec.frames_start(10, capacity=8, velocities=True, float64=True)
        rec.profile_start(10, 64, max_samples=100, **ALL)
        lay = rec.profile_info()
        assert lay.active == 1 and lay.start_step == 200
        rec.run_graph(50, 50)
        plain.run_graph(50, 50)
        p, f = rec.profile_read(), rec.frames_read()
        assert p.samples == 5 and list(f.step) == [210, 220, 230, 240, 250]
        assert np.array_equal(p.words, expected(f, spec, charges_of(rec), None, lay)[0])
        assert same_bits(state(rec), state(plain))
    finally:
        rec.close()
        plain.close()


# ------------------------------------------------------------------------------------------ 9. recovery
def test_a_repair_puts_the_table_back_with_the_step_counter():
    """vvhip_debug_recover repairs on request, without anything having failed: the snapshot of the run call goes back -- the profile's
    whole allocation with the step counter -- and the call is repeated.  Samples added twice would show as 20 samples and a doubled table."""
    spec = spec_for("C3")
    (it1, rec), (it2, calm) = make("C3", spec), make("C3", spec)
    try:
        for c in (rec, calm):
            c.run_graph(50, 50)
            c.profile_start(10, 64, groups=groups_for("C3", spec), max_samples=100, **ALL)
            c.run_graph(30, 10)                                     # three samples in the table before the snapshot
            c.synchronize()
        assert rec.fused_status()[0] and rec.recovery_count() == 0
        rec.run_graph(100, 50)
        calm.run_graph(100, 50)
        H.check(H.lib.vvhip_debug_recover(rec.plan), rec.plan)
        assert rec.recovery_count() == 1 and not rec.fused_status()[0] and rec.status_words() == [0, 0, 0, 0]
        p, q = rec.profile_read(), calm.profile_read()
        assert (p.samples, p.dropped, p.out_of_range) == (q.samples, q.dropped, q.out_of_range) == (13, 0, 0)
        assert np.array_equal(p.words, q.words)
        assert same_bits(state(rec), state(calm))
        assert rec.series_info().steps == calm.series_info().steps == 180
        # nothing in hand: refused
        assert H.lib.vvhip_debug_recover(rec.plan) == H.ERR_INVALID
    finally:
        rec.close()
        calm.close()
