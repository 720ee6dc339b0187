"""Device-side mean-squared displacements (include/vvhip.h: vvhip_msd_*) on the GPU.  The ground truth needs no second trajectory: the
same context also runs the frame recorder (float64) at the same interval, and the expected table is tests/msd_reference.py over those
frames.  Every comparison is np.array_equal on int64."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import barostat_cases as BK      # noqa: E402
import checkpoint_cases as K     # noqa: E402
import msd_reference as MR       # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S, I, D = pkg.systems, pkg.integrator, pkg.distributed
H = I.H

pytestmark = pytest.mark.gpu

NH_FIELDS = ("eta", "eta_dot", "eta_dotdot", "ke2", "vscale", "v_bias")
SCALE = {"C1": 1.0, "C3": 0.1, "C5": 0.25}
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


def groups_for(cfg, spec, molecules=False):
    """Particles: {Drude, non-Drude}; molecules: the molecule's id mod 2 (a Drude particle shares its parent's molecule); for C5 in both
    modes {electrode, ions, images -> -1}."""
    n = spec.num_atoms
    if cfg == "C5":
        g = np.full(n, -1, dtype=np.int8)
        g[np.asarray(spec.particles_ld, dtype=int)] = 0
        g[np.asarray(spec.particles_electrolyte, dtype=int)] = 1
        assert len(spec.image_pairs) > 0 and np.all(g[[a for a, _ in spec.image_pairs]] == -1)
        return g
    if molecules:
        return (np.asarray(spec.mol_id) % 2).astype(np.int8)
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


def centres(frames, spec, groups, lay, which=None):
    """(c [J, U, 3], g [U]): the units of the frames `which` (all) of a context, as the layout's mode defines them."""
    idx = np.asarray(frames.particles, dtype=int)
    masses, mol = np.asarray(spec.masses, dtype=np.float64)[idx], np.asarray(spec.mol_id)[idx]
    g = None if groups is None else np.asarray(groups)[idx]
    molecules = lay.mode == H.MSD_MOLECULES
    units = MR.molecule_units(masses, mol, g) if molecules else None
    out = [MR.unit_positions(frames.positions[j], masses, mol, g, molecules, units) for j in (range(len(frames)) if which is None else which)]
    return np.array([c for c, _ in out]), out[0][1]


def expected(frames, spec, groups, lay, which=None, floor=0):
    """(table, out of range) of the reference over the frames `which` (all) as samples 0, 1, ... for the layout `lay`."""
    c, g = centres(frames, spec, groups, lay, which)
    assert c.shape[1] == lay.num_units
    return MR.msd_reference(c, g, lay.num_groups, lay.num_lags, lay.origin_every, lay.frac_bits, lay.limit, floor)


def per_unit_pairs(msd, lay):
    """The pairs rows as they stand when nothing was out of range: units per group x the closed form per lag."""
    return MR.pair_counts(msd.samples, lay.origin_every, lay.num_lags)


# ------------------------------------------------------------------------------------------ 1. the table equals the reference over the frames
CASES = [("C1", "mixed", True), ("C3", "mixed", True), ("C5", "mixed", True), ("C3", "single", True), ("C3", "double", True), ("C3", "mixed", False)]
LAGS = [(8, 3), (8, 1), (8, 8)]


@pytest.mark.parametrize("cfg,precision,middle", CASES, ids=[f"{c}-{p}-{'middle' if m else 'classic'}" for c, p, m in CASES])
def test_table_equals_the_reference_over_the_frames(cfg, precision, middle):
    """Every description -- (num_lags, origin_every) of (8, 3), (8, 1), (8, 8), particles and molecules -- takes the next 300 steps of one
    context, which records its own frames beside it; a context without a recorder runs the same steps."""
    spec = spec_for(cfg)
    (_, rec), (_, plain) = make(cfg, spec, precision, middle), make(cfg, spec, precision, middle)
    try:
        rec.frames_start(10, capacity=30 * 2 * len(LAGS), float64=True)
        k = 0
        for molecules in (False, True):
            groups = groups_for(cfg, spec, molecules)
            for num_lags, every in LAGS:
                rec.msd_start(10, num_lags, every, molecules=molecules, groups=groups, max_samples=1000)
                lay = rec.msd_info()
                assert (lay.active, lay.num_groups, lay.words, lay.num_origins) == (1, int(groups.max()) + 1, (int(groups.max()) + 1) * num_lags * 4, -(-num_lags // every))
                assert lay.start_step == 300 * k and lay.frac_bits >= 8 and lay.limit == 64.0
                if not molecules:
                    assert lay.num_units == np.count_nonzero(groups >= 0)
                rec.run_graph(300, 50)
                m, f = rec.msd_read(), rec.frames_read()
                assert list(f.step[30 * k:]) == list(range(300 * k + 10, 300 * k + 301, 10))
                want, want_out = expected(f, spec, groups, lay, which=range(30 * k, 30 * k + 30))
                assert (m.samples, m.dropped, m.out_of_range, m.origin_floor) == (30, 0, 0, 0) and want_out == 0
                assert m.words.dtype == np.int64 and np.array_equal(m.words, want), (molecules, num_lags, every)
                assert np.array_equal(m.pairs.sum(axis=0), lay.num_units * per_unit_pairs(m, lay)) and m.pairs.sum() > 0
                assert np.all(m.total[m.pairs > 0] > 0)
                k += 1
        # the recorder changes nothing of the run
        plain.run_graph(300 * k, 50)
        assert same_bits(state(rec), state(plain))
    finally:
        rec.close()
        plain.close()


def test_molecules_whose_particles_alternate_in_index():
    """The barostat tests' synthetic system: molecules whose particles alternate in index, massless particles inside them, one molecule of
    130 particles, 3 000 of one -- a centre of mass is the sequential sum over the massive members in ascending index wherever they lie."""
    spec = BK.synthetic()
    it = I.VVIntegrator(300.0, 10.0, 1.0, 40.0, 0.001, 3, 1)
    it.setUseCOMTempGroup(False)
    ctx = I.Context(spec, it, precision="mixed", force_provider="tether")
    try:
        groups = (np.asarray(spec.mol_id) % 3).astype(np.int8)
        ctx.frames_start(5, capacity=16, float64=True)
        ctx.msd_start(5, 6, 2, molecules=True, groups=groups, max_samples=100)
        lay = ctx.msd_info()
        assert lay.num_units == len(MR.molecule_units(spec.masses, spec.mol_id, groups)) and lay.num_units % 16 != 0
        ctx.run_graph(60, 20)
        m, f = ctx.msd_read(), ctx.frames_read()
        want, want_out = expected(f, spec, groups, lay)
        assert (m.samples, m.out_of_range) == (12, 0) and want_out == 0 and np.array_equal(m.words, want) and m.pairs.sum() > 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 2. both add paths and the shapes
# C1 (1 992 particles: no multiple of 16, 64 or 512); every description takes the next 60 steps of one context per tune, sampled after
# every step, which records its own frames beside it.  The accumulating kernel's blocks have 64 threads at this size by default; two
# tunes give it 512 (what a large System gets) and 192 on a grid of three blocks.
LDS_WORDS = 64 * 1024 // 8


def _descriptions(n):
    rng = np.random.default_rng(17)
    sixteen, two = (np.arange(n) % 16).astype(np.int8), (np.arange(n) % 2).astype(np.int8)
    blocks = (np.arange(n) * 3 // n).astype(np.int8)
    last, run, third = np.full(n, -1, dtype=np.int8), np.full(n, -1, dtype=np.int8), np.full(n, -1, dtype=np.int8)
    last[n - 1] = 0
    run[3:3 + 65] = np.arange(65) % 2
    third[rng.choice(n, size=n // 3, replace=False)] = 1
    return [dict(num_lags=8, every=1, groups=two),                   # interleaved: the units are ordered by group, the wave at the seam adds per lane
            dict(num_lags=128, every=5, groups=sixteen),             # the last table that fits the LDS copy; every wave holds several groups
            dict(num_lags=129, every=5, groups=sixteen),             # the first that does not
            dict(num_lags=8, every=3, groups=blocks),
            dict(num_lags=8, every=8, groups=None),                  # no groups: every wave adds once
            dict(num_lags=4, every=1, groups=last),                  # one unit, the last particle
            dict(num_lags=8, every=2, groups=run),
            dict(num_lags=8, every=3, groups=third)]


_FIRST = []      # per tune: (frames of the first description's steps, its table)
TUNES = [None, {"grid_cap_a": 1}, {"block_threads": 128}, {"msd_wave_reduce": 0}, {"msd_block_threads": 512}, {"msd_block_threads": 192, "grid_cap_a": 3}]


@pytest.mark.parametrize("tune", TUNES, ids=["default", "grid_cap_a-1", "block_threads-128", "msd_wave_reduce-0", "msd_block_threads-512", "msd_block_threads-192-grid_cap_a-3"])
def test_both_add_paths_and_the_shapes(tune):
    spec = spec_for("C1")
    n = spec.num_atoms
    assert n % 16 != 0 and n % 64 != 0 and n % 512 != 0
    descriptions = _descriptions(n)
    assert 16 * 128 * 4 == LDS_WORDS < 16 * 129 * 4
    it, ctx = make("C1", spec, tune=tune)
    try:
        ctx.frames_start(1, capacity=60 * len(descriptions), float64=True)
        for k, d in enumerate(descriptions):
            ctx.msd_start(1, d["num_lags"], d["every"], groups=d["groups"], max_samples=100)
            lay = ctx.msd_info()
            assert lay.start_step == 60 * k and lay.num_units == (n if d["groups"] is None else np.count_nonzero(d["groups"] >= 0))
            ctx.run_graph(60, 20)
            m, frames = ctx.msd_read(), ctx.frames_read()
            assert list(frames.step[60 * k:]) == list(range(60 * k + 1, 60 * k + 61))
            want, want_out = expected(frames, spec, d["groups"], lay, which=range(60 * k, 60 * k + 60))
            assert (m.samples, m.dropped, m.out_of_range) == (60, 0, want_out) and want_out == 0, (k, m.samples, m.out_of_range)
            assert np.array_equal(m.words, want), (k, d["num_lags"], d["every"])
            assert np.array_equal(m.pairs.sum(axis=0), lay.num_units * per_unit_pairs(m, lay))
            if k == 0:
                _FIRST.append((frames.positions[:60].copy(), m.words))
        # ... and for the first description equal to each other across the tunes: the same inputs (the launch shapes of the step give the
        # same trajectory bits over these 60 steps, as tests/test_gpu_frames.py finds; later they part in the last bits), the same table
        for x, words in _FIRST:
            assert eq(x, _FIRST[0][0]) and np.array_equal(words, _FIRST[0][1])
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 3. out of range
def test_out_of_range_pairs_are_absent_from_all_four_words():
    """A limit of 2^-10 nm and a sample after every step: a particle moves about 5e-4 nm per component and step, so the short lags are
    mostly in range and the long ones mostly out -- asserted from the frames."""
    spec = spec_for("C3")
    groups = groups_for("C3", spec)
    limit = 2.0 ** -10
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(1, capacity=32, float64=True)
        ctx.msd_start(1, 8, 1, groups=groups, max_samples=64, limit=limit * 0.9)      # (rounded up to the power of two)
        lay = ctx.msd_info()
        assert lay.limit == limit and lay.frac_bits == 40
        ctx.run_graph(20, 10)
        m, f = ctx.msd_read(), ctx.frames_read()
        c, g = centres(f, spec, groups, lay)
        d1, d8 = np.abs(c[1:] - c[:-1]).max(axis=2), np.abs(c[8:] - c[:-8]).max(axis=2)
        assert np.count_nonzero(d1 < limit) > d1.size // 4 and np.count_nonzero(d8 >= limit) > d8.size // 4      # the premise: some in, some out
        want, want_out = expected(f, spec, groups, lay)
        assert m.samples == 20 and m.out_of_range == want_out > 0
        assert np.array_equal(m.words, want)
        # the pairs rows are short by exactly the pairs left out
        assert m.pairs.sum() == lay.num_units * per_unit_pairs(m, lay).sum() - m.out_of_range and m.pairs.sum() > 0
        assert np.all(m.words[:, :, 1:] <= m.words[:, :, :1] * int(limit * limit * 2.0 ** lay.frac_bits))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 4. max_samples, reset, the schedule
def test_max_samples_and_reset():
    spec = spec_for("C3")
    groups = groups_for("C3", spec)
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(10, capacity=16, float64=True)
        ctx.msd_start(10, 4, 2, groups=groups, max_samples=5)
        lay = ctx.msd_info()
        ctx.run_graph(100, 50)
        m = ctx.msd_read(reset=True)
        f = ctx.frames_read()
        assert (m.samples, m.dropped) == (5, 5) and list(f.step) == list(range(10, 101, 10))
        assert np.array_equal(m.words, expected(f, spec, groups, lay, which=range(5))[0])
        z = ctx.msd_read()
        assert (z.samples, z.dropped, z.out_of_range, z.origin_floor) == (0, 0, 0, 0) and not z.words.any()
        # the schedule continues without gap or repeat; the ordinal restarts at 0 with no live origin (the ring still holds the old ones)
        ctx.run_graph(40, 50)
        t, f = ctx.msd_read(), ctx.frames_read()
        assert list(f.step[10:]) == [110, 120, 130, 140] and (t.samples, t.dropped) == (4, 0)
        assert np.array_equal(t.words, expected(f, spec, groups, lay, which=range(10, 14))[0])
        assert np.array_equal(t.pairs.sum(axis=0), lay.num_units * MR.pair_counts(4, 2, 4))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 5. stepping paths and the graph cache
def _scheduled(path, interval, n=317):
    spec = spec_for("C3")
    it, ctx = make("C3", spec)
    try:
        it.step(3)                                                  # an unaligned start, host-driven
        ctx.msd_start(interval, 8, 3, groups=groups_for("C3", spec), max_samples=100)
        assert ctx.msd_info().start_step == 3
        if path == "step":
            it.step(n)
        elif path == "eager":
            ctx.run_eager(n)
        else:
            ctx.run_graph(n, 50)
        return ctx.msd_read()
    finally:
        ctx.close()


@pytest.mark.parametrize("interval", [7, 50])
def test_every_stepping_path_gives_the_same_table(interval):
    g = _scheduled("graph", interval)
    assert g.samples == 320 // interval and g.dropped == 0 and g.out_of_range == 0 and g.pairs.sum() > 0
    for path in ("step", "eager"):
        m = _scheduled(path, interval)
        assert (m.samples, m.dropped, m.out_of_range) == (g.samples, 0, 0) and np.array_equal(m.words, g.words), path


def test_steady_state_replays_capture_nothing():
    spec = spec_for("C3")
    it, ctx = make("C3", spec)
    try:
        ctx.msd_start(50, 8, 3, max_samples=100)
        ctx.run_graph(2000, 50)
        before = ctx.series_info().graph_captures
        ctx.run_graph(1000, 50)
        assert ctx.series_info().graph_captures == before, (before, ctx.series_info().graph_captures)
        m = ctx.msd_read()
        assert m.samples == 60 and np.array_equal(m.pairs[0], spec.num_atoms * MR.pair_counts(60, 3, 8))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 6. shards
@pytest.mark.parametrize("molecules", [False, True], ids=["particles", "molecules"])
def test_shards_tables_add_to_the_unsharded_definition(molecules):
    """A shard's thermostat sees its own particles' sums only, so a shard and the unsharded run do not take the same steps: the state is
    uploaded from one unsharded context, every context then takes six steps with a sample behind each, and each table is compared with
    the definition on that context's own frames.  The shards' fixed point is the unsharded one (it follows the description over the whole
    System), so msd_sum of the shards' tables is the table of the definition -- in the unsharded layout -- on the union of the shards'
    units."""
    spec = spec_for("C3")
    n = spec.num_atoms
    groups = groups_for("C3", spec, molecules)
    mol = np.asarray(spec.mol_id)
    cut = int(np.nonzero(mol == mol[n // 2])[0].min())             # a molecule boundary
    assert 0 < cut < n and mol[cut - 1] != mol[cut] and not set(mol[:cut].tolist()) & set(mol[cut:].tolist())
    it0, whole = make("C3", spec)
    shards = []
    try:
        whole.run_eager(20)
        posq, corr, velm = whole.getPosq(), whole.getPosqCorrection(), whole.getVelm()
        whole.frames_start(1, capacity=8, float64=True)
        whole.msd_start(1, 4, 2, molecules=molecules, groups=groups, max_samples=50)
        lay0 = whole.msd_info()
        it0.step(6)
        m0, f0 = whole.msd_read(), whole.frames_read()
        assert m0.samples == 6 and np.array_equal(m0.words, expected(f0, spec, groups, lay0)[0])
        tables, cs, gs = [], [], []
        for shard in ((0, cut), (cut, n)):
            it = integrator_for("C3", spec)
            it.setUseCOMTempGroup(False)
            ctx = I.Context(spec, it, precision="mixed", force_provider="tether", shard=shard)
            shards.append(ctx)
            sl = slice(*shard)
            ctx.posq.upload(posq[sl]); ctx.posq_corr.upload(corr[sl]); ctx.velm.upload(velm[sl])
            ctx.frames_start(1, capacity=8, float64=True)
            ctx.msd_start(1, 4, 2, molecules=molecules, groups=groups, max_samples=50)
            lay = ctx.msd_info()
            assert (lay.frac_bits, lay.limit, lay.words, lay.num_origins) == (lay0.frac_bits, lay0.limit, lay0.words, lay0.num_origins)
            it.step(6)
            m, f = ctx.msd_read(), ctx.frames_read()
            assert m.samples == 6 and eq(f.particles, np.arange(shard[0], shard[1], dtype=np.int32))
            assert np.array_equal(m.words, expected(f, spec, groups, lay)[0]), shard
            tables.append(m)
            c, g = centres(f, spec, groups, lay)
            cs.append(c); gs.append(g)
        assert sum(t.pairs.sum() for t in tables) == m0.pairs.sum()
        total = D.msd_sum(tables)
        union, _ = MR.msd_reference(np.concatenate(cs, axis=1), np.concatenate(gs), lay0.num_groups, lay0.num_lags, lay0.origin_every, lay0.frac_bits, lay0.limit)
        assert np.array_equal(total.words, union) and np.array_equal(total.pairs, m0.pairs) and total.out_of_range == 0
    finally:
        whole.close()
        for c in shards:
            c.close()


def test_a_shard_that_cuts_a_molecule_is_refused_in_molecule_mode():
    spec = BK.synthetic()
    it = I.VVIntegrator(300.0, 10.0, 1.0, 40.0, 0.001, 3, 1)
    it.setUseCOMTempGroup(False)
    ctx = I.Context(spec, it, precision="mixed", force_provider="tether", shard=(0, 3))
    try:
        with pytest.raises(H.VVHipError) as e:
            ctx.msd_start(1, 4, 1, molecules=True)
        assert e.value.code == H.ERR_UNSUPPORTED and "cuts a molecule" in str(e.value) and ctx.msd_info().active == 0
        ctx.msd_start(1, 4, 1)                                      # particles: every shard records its own
        assert ctx.msd_info().active == 1 and ctx.msd_info().num_units == 3
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 7. five riders together
def test_five_riders_with_windows_that_shift_between_replays():
    """Series every 7, removals every 5, frames every 3, profile every 11, MSD every 13, graphs of 20 steps: no interval divides the
    graph's length, so the replays' windows differ.  `graph` against `single` (one vvhip_step_middle at a time), all five riders on in
    both; `truth` has the series and the removals on too (the removal changes the trajectory: like with like) and its frames at the
    MSD's steps."""
    spec = spec_for("C3")
    groups = groups_for("C3", spec)
    (it1, graph), (it2, single), (it3, truth) = make("C3", spec), make("C3", spec), make("C3", spec)
    try:
        for c in (graph, single, truth):
            c.series_start(7, capacity=32)
            c.remove_cm_motion_every(5)
        for c in (graph, single):
            c.frames_start(3, capacity=64, velocities=True, float64=True)
            c.profile_start(11, 64, groups=groups, max_samples=100, charge=True, mass=True, momentum=True, kinetic=True)
            c.msd_start(13, 8, 3, groups=groups, max_samples=100)
        truth.frames_start(13, capacity=32, float64=True)
        lay = graph.msd_info()
        graph.run_graph(130, 20)
        graph.run_eager(3)
        graph.run_graph(47, 20)
        for _ in range(180):
            it2.step(1)
        truth.run_graph(180, 20)
        mg, ms = graph.msd_read(), single.msd_read()
        assert (mg.samples, mg.dropped, mg.out_of_range) == (ms.samples, ms.dropped, ms.out_of_range) == (13, 0, 0)
        assert np.array_equal(mg.words, ms.words)
        ft = truth.frames_read()
        assert list(ft.step) == list(range(13, 181, 13))
        assert np.array_equal(mg.words, expected(ft, spec, groups, lay)[0]) and mg.pairs.sum() > 0
        pg, ps = graph.profile_read(), single.profile_read()
        assert pg.samples == ps.samples == 16 and np.array_equal(pg.words, ps.words)
        fg, fs = graph.frames_read(), single.frames_read()
        assert list(fg.step) == list(fs.step) == list(range(3, 181, 3)) and fg.dropped == fs.dropped == 0
        assert eq(fg.positions, fs.positions) and eq(fg.velocities, fs.velocities)
        rows = [c.series_read() for c in (graph, single, truth)]
        for r in rows:
            assert list(r.step) == list(range(7, 181, 7)) and r.dropped == 0
        for name in ("raw", "ke", "t", "box") + NH_FIELDS:
            assert eq(getattr(rows[0], name), getattr(rows[1], name)) and eq(getattr(rows[0], name), getattr(rows[2], name)), name
        recs = [c.cm_motion_record() for c in (graph, single, truth)]
        assert [r.removals for r in recs] == [36, 36, 36] and [r.skipped for r in recs] == [0, 0, 0]
        K.assert_same(K.state(graph), K.state(single), "replays against single steps")
    finally:
        for c in (graph, single, truth):
            c.close()


# ------------------------------------------------------------------------------------------ 8. stop and the checkpoint
def test_stop_and_the_checkpoint():
    spec = spec_for("C3")
    (it1, rec), (it2, plain) = make("C3", spec), make("C3", spec)
    try:
        rec.msd_start(10, 8, 3, max_samples=100)
        rec.run_graph(200, 50)
        plain.run_graph(200, 50)
        assert rec.msd_read().samples == 20
        blob = plain.createCheckpoint()
        with pytest.raises(H.VVHipError) as e:
            rec.loadCheckpoint(blob)
        assert e.value.code == H.ERR_INVALID and "an MSD recorder is running: stop it, load, start it again" in str(e.value)
        rec.msd_stop()
        info = rec.msd_info()
        assert info.active == 0 and info.words == 0
        with pytest.raises(H.VVHipError):
            rec.msd_read()
        # stopped: further steps as if there never was a recorder
        rec.run_graph(100, 50)
        rec.run_eager(13)
        plain.run_graph(100, 50)
        plain.run_eager(13)
        assert same_bits(state(rec), state(plain))
        # stop, load, start works: the recorder begins at the loaded step counter
        rec.loadCheckpoint(blob)
        plain.loadCheckpoint(blob)
        rec.frames_start(10, capacity=8, float64=True)
        rec.msd_start(10, 8, 3, max_samples=100)
        lay = rec.msd_info()
        assert lay.active == 1 and lay.start_step == 200
        rec.run_graph(50, 50)
        plain.run_graph(50, 50)
        m, f = rec.msd_read(), rec.frames_read()
        assert m.samples == 5 and list(f.step) == [210, 220, 230, 240, 250]
        assert np.array_equal(m.words, expected(f, spec, None, lay)[0]) and m.pairs.sum() > 0
        assert same_bits(state(rec), state(plain))
    finally:
        rec.close()
        plain.close()


# ------------------------------------------------------------------------------------------ 9. recovery
def test_a_repair_puts_table_and_ring_back_with_the_step_counter():
    """vvhip_debug_recover repairs on request, without anything having failed: the snapshot of the run call goes back -- the recorder's
    whole allocation, the ring of origins included, with the step counter -- and the call is repeated.  origin_every = 1 and num_lags = 2
    make a ring of two slots, each overwritten five times inside the repeated window of 100 steps: the repeat's first samples measure
    against the origins of samples 1 and 2, which the window's last samples overwrote.  A ring that did not go back shows as a different
    table, samples added twice as 23 samples."""
    spec = spec_for("C3")
    (it1, rec), (it2, calm) = make("C3", spec), make("C3", spec)
    try:
        for c in (rec, calm):
            c.run_graph(50, 50)
            c.msd_start(10, 2, 1, groups=groups_for("C3", spec), max_samples=100)
            c.run_graph(30, 10)                                     # three samples before the snapshot
            c.synchronize()
        assert rec.msd_info().num_origins == 2
        assert rec.fused_status()[0] and rec.recovery_count() == 0
        rec.run_graph(100, 50)
        calm.run_graph(100, 50)
        H.check(H.lib.vvhip_debug_recover(rec.plan), rec.plan)
        assert rec.recovery_count() == 1 and not rec.fused_status()[0] and rec.status_words() == [0, 0, 0, 0]
        m, q = rec.msd_read(), calm.msd_read()
        assert (m.samples, m.dropped, m.out_of_range, m.origin_floor) == (q.samples, q.dropped, q.out_of_range, q.origin_floor) == (13, 0, 0, 0)
        assert np.array_equal(m.words, q.words) and m.pairs.sum() > 0
        assert same_bits(state(rec), state(calm))
        assert rec.series_info().steps == calm.series_info().steps == 180
    finally:
        rec.close()
        calm.close()


# ------------------------------------------------------------------------------------------ 10. the barostat
def test_barostat_moves_set_the_origin_floor():
    """scale_box and restore_box rewrite the positions outside the steps: origins stored before are dead, the table is kept."""
    spec = spec_for("C3")
    groups = groups_for("C3", spec)
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(10, capacity=32, float64=True)
        ctx.msd_start(10, 8, 1, groups=groups, max_samples=100)
        lay = ctx.msd_info()
        ctx.run_graph(50, 50)                                       # samples 0 .. 4
        before = ctx.msd_read()
        assert (before.samples, before.origin_floor) == (5, 0)
        ctx.scale_box((1.01, 0.99, 1.02))
        after = ctx.msd_read()
        assert (after.samples, after.origin_floor) == (5, 5) and np.array_equal(after.words, before.words)      # the table is kept
        ctx.run_graph(40, 20)                                       # samples 5 .. 8
        assert ctx.msd_read().origin_floor == 5
        ctx.scale_box((1.05, 1.05, 1.05))
        assert ctx.msd_read().origin_floor == 9
        ctx.restore_box()
        ctx.run_graph(30, 10)                                       # samples 9 .. 11
        ctx.scale_box((0.99, 0.99, 0.99))
        ctx.restore_box()
        ctx.run_eager(30)                                           # samples 12 .. 14
        m, f = ctx.msd_read(), ctx.frames_read()
        assert (m.samples, m.origin_floor, m.out_of_range) == (15, 12, 0) and list(f.step) == list(range(10, 151, 10))
        floors = [0] * 5 + [5] * 4 + [9] * 3 + [12] * 3
        want, want_out = expected(f, spec, groups, lay, floor=floors)
        assert want_out == 0 and np.array_equal(m.words, want)
        # ... which is fewer pairs than an undisturbed run of 15 samples has
        assert 0 < m.pairs.sum() < lay.num_units * MR.pair_counts(15, 1, 8).sum()
        assert m.pairs.sum() == lay.num_units * len(MR.pairs(15, 1, 8, floors))
    finally:
        ctx.close()
