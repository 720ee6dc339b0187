"""Device-side self van Hove functions (include/vvhip.h: vvhip_vanhove_*) on the GPU.  The ground truth needs no second trajectory: the
same context also runs the frame recorder (float64) at the same interval, and the expected table is tests/vanhove_reference.py over those
frames.  Every comparison is np.array_equal on int64."""
import ctypes as C
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
import vanhove_reference as VR   # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S, I, D = pkg.systems, pkg.integrator, pkg.distributed
H = I.H

pytestmark = pytest.mark.gpu

NH_FIELDS = ("eta", "eta_dot", "eta_dotdot", "ke2", "vscale", "v_bias")
SCALE = {"C1": 1.0, "C3": 0.1}
_SPECS = {}
# the tethered particles move about 5e-4 nm per component and step: logarithmic bins from 1e-4 nm to 0.2 nm hold every displacement of
# these runs but the shortest, which are counted in `below`
LOG_EDGES = I.vanhove_edges(0.2, 48, 1e-4)


def spec_for(cfg):
    if cfg not in _SPECS:
        _SPECS[cfg] = S.make_config(cfg, scale=SCALE[cfg])
    return _SPECS[cfg]


def integrator_for(cfg, spec, middle=True, dt=0.001):
    it = I.VVIntegrator(333.0, 10.0, 1.0, 40.0, dt, 3, 1)
    if cfg != "C1":
        it.setMaxDrudeDistance(0.02)
    it.setUseMiddleScheme(middle)
    return it


def make(cfg, spec, precision="mixed", middle=True, dt=0.001, **kw):
    it = integrator_for(cfg, spec, middle, dt)
    return it, I.Context(spec, it, precision=precision, force_provider="tether", **kw)


def groups_for(spec, molecules=False):
    """Particles: {Drude, non-Drude}; molecules: the molecule's id mod 2 (a Drude particle shares its parent's molecule)."""
    if molecules:
        return (np.asarray(spec.mol_id) % 2).astype(np.int8)
    g = np.ones(spec.num_atoms, dtype=np.int8)
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


def live_buffers():
    n, b = C.c_int64(0), C.c_int64(0)
    assert H.lib.vvhip_debug_live_buffers(C.byref(n), C.byref(b)) == H.OK
    return n.value


def centres(frames, spec, groups, lay, which=None):
    """(c [J, U, 3], g [U]): the units of the frames `which` (all) of a context, as the layout's mode defines them."""
    idx = np.asarray(frames.particles, dtype=int)
    masses, mol = np.asarray(spec.masses, dtype=np.float64)[idx], np.asarray(spec.mol_id)[idx]
    g = None if groups is None else np.asarray(groups)[idx]
    molecules = lay.mode == H.VANHOVE_MOLECULES
    units = VR.molecule_units(masses, mol, g) if molecules else None
    out = [VR.unit_positions(frames.positions[j], masses, mol, g, molecules, units) for j in (range(len(frames)) if which is None else which)]
    return np.array([c for c, _ in out]), out[0][1]


def exps_of(lay):
    return (lay.frac2_bits, lay.r4_hi_bits, lay.r4_lo_bits)


def expected(frames, spec, groups, lay, edges, which=None, floor=0):
    """(head, hist, out of range) of the reference over the frames `which` (all) as samples 0, 1, ... for the layout `lay`."""
    c, g = centres(frames, spec, groups, lay, which)
    assert c.shape[1] == lay.num_units
    return VR.vanhove_reference(c, g, lay.num_groups, lay.num_lags, lay.origin_every, edges, exps_of(lay), lay.limit, floor)


def assert_table(v, want, what=None):
    assert v.head.dtype == np.int64 and v.hist.dtype == np.int64
    assert np.array_equal(v.head, want[0]), what
    assert np.array_equal(v.hist, want[1]), what
    assert np.array_equal(v.below + v.hist.sum(axis=2) + v.beyond, v.pairs), what      # the invariant


def same_table(a, b):
    return np.array_equal(a.head, b.head) and np.array_equal(a.hist, b.hist)


# ------------------------------------------------------------------------------------------ 1. the table equals the reference over the frames
CASES = [("C3", "mixed", True), ("C3", "single", True), ("C3", "double", True), ("C3", "mixed", False), ("C1", "mixed", True)]


@pytest.mark.parametrize("cfg,precision,middle", CASES, ids=[f"{c}-{p}-{'middle' if m else 'classic'}" for c, p, m in CASES])
def test_table_equals_the_reference_over_the_frames(cfg, precision, middle):
    """Particles and molecules take the next 150 steps each of one context, which records its own frames beside it; a context without a
    recorder runs the same steps."""
    spec = spec_for(cfg)
    (_, rec), (_, plain) = make(cfg, spec, precision, middle), make(cfg, spec, precision, middle)
    try:
        rec.frames_start(10, capacity=15 * 2, float64=True)
        for k, molecules in enumerate((False, True)):
            groups = groups_for(spec, molecules)
            G = int(groups.max()) + 1
            rec.vanhove_start(10, 7, LOG_EDGES, 3, molecules=molecules, groups=groups, max_samples=1000)
            lay = rec.vanhove_info()
            assert (lay.active, lay.num_groups, lay.num_bins, lay.num_origins) == (1, G, 48, 3)
            assert (lay.head_words, lay.hist_words, lay.words) == (G * 7 * 6, G * 7 * 48, G * 7 * 54)
            assert lay.start_step == 150 * k and lay.limit == 16.0 and lay.frac2_bits >= 8 and lay.r4_hi_bits >= 0
            if not molecules:
                assert lay.num_units == np.count_nonzero(groups >= 0)
            rec.run_graph(150, 50)
            v, f = rec.vanhove_read(), rec.frames_read()
            assert list(f.step[15 * k:]) == list(range(150 * k + 10, 150 * k + 151, 10))
            want = expected(f, spec, groups, lay, LOG_EDGES, which=range(15 * k, 15 * k + 15))
            assert (v.samples, v.dropped, v.out_of_range, v.origin_floor) == (15, 0, 0, 0) and want[2] == 0
            assert_table(v, want, molecules)
            assert np.array_equal(v.pairs.sum(axis=0), lay.num_units * MR.pair_counts(15, 3, 7)) and v.hist.sum() > 0
            assert np.all(v.msd[v.pairs > 0] > 0) and np.all(v.r4[v.pairs > 0] > 0)
        # the recorder changes nothing of the run
        plain.run_graph(300, 50)
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
        ctx.vanhove_start(5, 6, LOG_EDGES, 2, molecules=True, groups=groups, max_samples=100)
        lay = ctx.vanhove_info()
        assert lay.num_units == len(MR.molecule_units(spec.masses, spec.mol_id, groups)) and lay.num_units % 16 != 0
        ctx.run_graph(60, 20)
        v, f = ctx.vanhove_read(), ctx.frames_read()
        want = expected(f, spec, groups, lay, LOG_EDGES)
        assert (v.samples, v.out_of_range) == (12, 0) and want[2] == 0 and v.pairs.sum() > 0
        assert_table(v, want)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 2. both add paths and the shapes
# C1 (1 992 particles: no multiple of 16, 64 or 512); every description takes the next 40 steps of one context per tune, sampled after
# every step, which records its own frames beside it.  The accumulating kernel's blocks have 64 threads at this size by default.
def _first(n, count, of=1):
    g = np.full(n, -1, dtype=np.int8)
    g[5:5 + count] = np.arange(count) % of
    return g


def _descriptions(n):
    sixteen, two = (np.arange(n) % 16).astype(np.int8), (np.arange(n) % 2).astype(np.int8)
    last = np.full(n, -1, dtype=np.int8)
    last[n - 1] = 0
    three = np.full(n, -1, dtype=np.int8)
    three[100:200], three[700:900], three[1500:1713] = 0, 1, 2       # 513 units; the seams at units 100 and 300 lie inside a wave
    return [dict(num_lags=8, every=4, groups=two, edges=I.vanhove_edges(0.05, 128, 1e-4)),           # interleaved: ordered by group, the seam at unit 996 inside a wave
            dict(num_lags=1, every=1, groups=last, edges=np.array([0.0, 1.0])),                      # U = 1, one bin
            dict(num_lags=7, every=3, groups=_first(n, 63), edges=np.array([1e-3, 2e-3, 4e-3])),     # U = 63, two bins, below and beyond populated
            dict(num_lags=8, every=4, groups=_first(n, 64), edges=I.vanhove_edges(0.01, 16)),        # U = 64, uniform
            dict(num_lags=7, every=3, groups=_first(n, 65, 2), edges=I.vanhove_edges(0.05, 32, 5e-4)),      # U = 65 in two groups of 33 and 32
            dict(num_lags=7, every=3, groups=three, edges=I.vanhove_edges(0.02, 1024)),              # U = 513 in three groups, 1024 uniform bins: 3 x 1024 words of the LDS histogram
            dict(num_lags=8, every=4, groups=sixteen, edges=I.vanhove_edges(0.05, 1024, 1e-4)),      # sixteen groups of 1024 bins: four fit the LDS histogram, a chunk of 512 units holds five
            dict(num_lags=1, every=1, groups=None, edges=I.vanhove_edges(0.01, 2, 1e-3))]            # no groups: every wave adds once


_FIRST = []      # per tune: (frames of the first description's steps, its table)
TUNES = [None, {"vanhove_lds": 0}, {"vanhove_block_threads": 64, "grid_cap_a": 3}, {"vanhove_block_threads": 192, "grid_cap_a": 3},
         {"vanhove_block_threads": 512}, {"vanhove_block_threads": 512, "vanhove_lds": 0}, {"vanhove_wave_reduce": 0}, {"grid_cap_a": 1}]


@pytest.mark.parametrize("tune", TUNES, ids=["default", "lds-0", "threads-64-grid-3", "threads-192-grid-3", "threads-512", "threads-512-lds-0",
                                             "wave_reduce-0", "grid-1"])
def test_both_add_paths_and_the_shapes(tune):
    spec = spec_for("C1")
    n = spec.num_atoms
    assert n % 16 != 0 and n % 64 != 0 and n % 512 != 0
    descriptions = _descriptions(n)
    it, ctx = make("C1", spec, tune=tune)
    try:
        ctx.frames_start(1, capacity=40 * len(descriptions), float64=True)
        for k, d in enumerate(descriptions):
            ctx.vanhove_start(1, d["num_lags"], d["edges"], d["every"], groups=d["groups"], max_samples=100)
            lay = ctx.vanhove_info()
            assert lay.start_step == 40 * k and lay.num_units == (n if d["groups"] is None else np.count_nonzero(d["groups"] >= 0))
            assert lay.num_bins == len(d["edges"]) - 1
            ctx.run_graph(40, 20)
            v, frames = ctx.vanhove_read(), ctx.frames_read()
            assert list(frames.step[40 * k:]) == list(range(40 * k + 1, 40 * k + 41))
            want = expected(frames, spec, d["groups"], lay, d["edges"], which=range(40 * k, 40 * k + 40))
            assert (v.samples, v.dropped, v.out_of_range) == (40, 0, 0) and want[2] == 0, (k, v.samples, v.out_of_range)
            assert_table(v, want, k)
            assert np.array_equal(v.pairs.sum(axis=0), lay.num_units * MR.pair_counts(40, d["every"], d["num_lags"]))
            if k == 2:
                assert v.below.sum() > 0 and v.beyond.sum() > 0 and v.hist.sum() > 0
            if k == 0:
                _FIRST.append((frames.positions[:40].copy(), v))
        # ... and for the first description equal to each other across the tunes: the same inputs, the same table
        for x, v in _FIRST:
            assert eq(x, _FIRST[0][0]) and same_table(v, _FIRST[0][1])
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 3. out of range
def test_out_of_range_pairs_are_absent_from_every_word():
    """One unit jumps by three times the limit between two samples and one position becomes NaN before the last: their pairs across the
    jump, and with the NaN, are in no word and are counted.  The only test with out_of_range > 0."""
    spec = spec_for("C1")
    limit = 2.0 ** -5
    it, ctx = make("C1", spec)
    try:
        ctx.frames_start(1, capacity=16, float64=True)
        ctx.vanhove_start(1, 8, LOG_EDGES, 1, max_samples=64, limit=limit * 0.9)      # (rounded up to the power of two)
        lay = ctx.vanhove_info()
        assert lay.limit == limit
        it.step(6)
        x = ctx.getPosq()
        x[17, 0] += 3 * limit
        ctx.posq.upload(x)
        it.step(3)
        x = ctx.getPosq()
        x[40, 1] = np.nan
        ctx.posq.upload(x)
        it.step(1)
        v, f = ctx.vanhove_read(), ctx.frames_read()
        c, g = centres(f, spec, None, lay)
        assert abs(c[6, 17, 0] - c[5, 17, 0]) > 2 * limit and np.isnan(c[9, 40, 1]) and np.all(np.isfinite(c[:9]))      # the premise
        want = expected(f, spec, None, lay, LOG_EDGES)
        assert v.samples == 10 and v.out_of_range == want[2] >= 6 * 3 + 8
        assert_table(v, want)
        # the pairs rows are short by exactly the pairs left out
        assert v.pairs.sum() == lay.num_units * MR.pair_counts(10, 1, 8).sum() - v.out_of_range and v.pairs.sum() > 0
        assert np.all(v.head[:, :, 3] <= v.pairs * int(3 * limit * limit * 2.0 ** lay.frac2_bits))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 4. max_samples, reset, the schedule
def test_max_samples_and_reset():
    spec = spec_for("C3")
    groups = groups_for(spec)
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(10, capacity=16, float64=True)
        ctx.vanhove_start(10, 4, LOG_EDGES, 2, groups=groups, max_samples=5)
        lay = ctx.vanhove_info()
        ctx.run_graph(100, 50)
        v = ctx.vanhove_read(reset=True)
        f = ctx.frames_read()
        assert (v.samples, v.dropped) == (5, 5) and list(f.step) == list(range(10, 101, 10))
        assert_table(v, expected(f, spec, groups, lay, LOG_EDGES, which=range(5)))
        z = ctx.vanhove_read()
        assert (z.samples, z.dropped, z.out_of_range, z.origin_floor) == (0, 0, 0, 0) and not z.head.any() and not z.hist.any()
        # the schedule continues without gap or repeat; the ordinal restarts at 0 with no live origin (the ring still holds the old ones)
        ctx.run_graph(40, 50)
        t, f = ctx.vanhove_read(), ctx.frames_read()
        assert list(f.step[10:]) == [110, 120, 130, 140] and (t.samples, t.dropped) == (4, 0)
        assert_table(t, expected(f, spec, groups, lay, LOG_EDGES, which=range(10, 14)))
        assert np.array_equal(t.pairs.sum(axis=0), lay.num_units * MR.pair_counts(4, 2, 4))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 5. stepping paths and the graph cache
def _scheduled(path, interval, n=317):
    spec = spec_for("C3")
    it, ctx = make("C3", spec)
    try:
        it.step(3)                                                  # an unaligned start, host-driven
        ctx.vanhove_start(interval, 8, LOG_EDGES, 3, groups=groups_for(spec), max_samples=100)
        assert ctx.vanhove_info().start_step == 3
        if path == "step":
            it.step(n)
        elif path == "eager":
            ctx.run_eager(n)
        else:
            ctx.run_graph(n, 50)
        return ctx.vanhove_read()
    finally:
        ctx.close()


@pytest.mark.parametrize("interval", [7, 50])
def test_every_stepping_path_gives_the_same_table(interval):
    g = _scheduled("graph", interval)
    assert g.samples == 320 // interval and g.dropped == 0 and g.out_of_range == 0 and g.pairs.sum() > 0 and g.hist.sum() > 0
    for path in ("step", "eager"):
        v = _scheduled(path, interval)
        assert (v.samples, v.dropped, v.out_of_range) == (g.samples, 0, 0) and same_table(v, g), path


def test_steady_state_replays_capture_nothing():
    spec = spec_for("C3")
    it, ctx = make("C3", spec)
    try:
        ctx.vanhove_start(50, 8, LOG_EDGES, 3, max_samples=100)
        ctx.run_graph(2000, 50)
        before = ctx.series_info().graph_captures
        ctx.run_graph(1000, 50)
        assert ctx.series_info().graph_captures == before, (before, ctx.series_info().graph_captures)
        v = ctx.vanhove_read()
        assert v.samples == 60 and np.array_equal(v.pairs[0], spec.num_atoms * MR.pair_counts(60, 3, 8))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 6. shards
@pytest.mark.parametrize("molecules", [False, True], ids=["particles", "molecules"])
def test_shards_tables_add_to_the_unsharded_definition(molecules):
    """As for the MSD: the state is uploaded from one unsharded context, every context then takes six steps with a sample behind each,
    and each table is compared with the definition on that context's own frames.  The shards' fixed point is the unsharded one, so
    vanhove_sum of the shards' tables is the table of the definition -- in the unsharded layout -- on the union of the shards' units."""
    spec = spec_for("C3")
    n = spec.num_atoms
    groups = groups_for(spec, molecules)
    mol = np.asarray(spec.mol_id)
    cut = int(np.nonzero(mol == mol[n // 2])[0].min())             # a molecule boundary
    assert 0 < cut < n and mol[cut - 1] != mol[cut] and not set(mol[:cut].tolist()) & set(mol[cut:].tolist())
    it0, whole = make("C3", spec)
    shards = []
    try:
        whole.run_eager(20)
        posq, corr, velm = whole.getPosq(), whole.getPosqCorrection(), whole.getVelm()
        whole.frames_start(1, capacity=8, float64=True)
        whole.vanhove_start(1, 4, LOG_EDGES, 2, molecules=molecules, groups=groups, max_samples=50)
        lay0 = whole.vanhove_info()
        it0.step(6)
        v0, f0 = whole.vanhove_read(), whole.frames_read()
        assert v0.samples == 6
        assert_table(v0, expected(f0, spec, groups, lay0, LOG_EDGES))
        tables, cs, gs = [], [], []
        for shard in ((0, cut), (cut, n)):
            it = integrator_for("C3", spec)
            it.setUseCOMTempGroup(False)
            ctx = I.Context(spec, it, precision="mixed", force_provider="tether", shard=shard)
            shards.append(ctx)
            sl = slice(*shard)
            ctx.posq.upload(posq[sl]); ctx.posq_corr.upload(corr[sl]); ctx.velm.upload(velm[sl])
            ctx.frames_start(1, capacity=8, float64=True)
            ctx.vanhove_start(1, 4, LOG_EDGES, 2, molecules=molecules, groups=groups, max_samples=50)
            lay = ctx.vanhove_info()
            assert exps_of(lay) + (lay.limit, lay.words, lay.num_origins) == exps_of(lay0) + (lay0.limit, lay0.words, lay0.num_origins)
            it.step(6)
            v, f = ctx.vanhove_read(), ctx.frames_read()
            assert v.samples == 6 and eq(f.particles, np.arange(shard[0], shard[1], dtype=np.int32))
            assert_table(v, expected(f, spec, groups, lay, LOG_EDGES), shard)
            tables.append(v)
            c, g = centres(f, spec, groups, lay)
            cs.append(c); gs.append(g)
        assert sum(t.pairs.sum() for t in tables) == v0.pairs.sum()
        total = D.vanhove_sum(tables)
        union = VR.vanhove_reference(np.concatenate(cs, axis=1), np.concatenate(gs), lay0.num_groups, lay0.num_lags, lay0.origin_every, LOG_EDGES,
                                     exps_of(lay0), lay0.limit)
        assert_table(total, union)
        assert np.array_equal(total.pairs, v0.pairs) and total.out_of_range == 0
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
            ctx.vanhove_start(1, 4, LOG_EDGES, 1, molecules=True)
        assert e.value.code == H.ERR_UNSUPPORTED and "cuts a molecule" in str(e.value) and ctx.vanhove_info().active == 0
        ctx.vanhove_start(1, 4, LOG_EDGES, 1)                       # particles: every shard records its own
        assert ctx.vanhove_info().active == 1 and ctx.vanhove_info().num_units == 3
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 7. beside other riders
def test_beside_the_msd_recorder_with_the_same_description():
    """The same units, schedule and pairs: `pairs` is the MSD's word 0 everywhere, and the sum of r2 is the MSD's three sums added, up to
    the roundings -- per pair three halves of the MSD's unit and one half of this recorder's: at most 2 units of the coarser scale."""
    spec = spec_for("C3")
    groups = groups_for(spec)
    it, ctx = make("C3", spec)
    try:
        ctx.msd_start(10, 8, 3, groups=groups, max_samples=100)
        ctx.vanhove_start(10, 8, LOG_EDGES, 3, groups=groups, max_samples=100)
        ctx.run_graph(200, 50)
        m, v = ctx.msd_read(), ctx.vanhove_read()
        assert m.samples == v.samples == 20 and m.out_of_range == v.out_of_range == 0
        assert np.array_equal(v.pairs, m.words[:, :, 0]) and v.pairs.sum() > 0
        top = max(m.frac_bits, v.frac2_bits)
        a = v.head[:, :, 3].astype(object) * 2 ** (top - v.frac2_bits)
        b = m.words[:, :, 1:].astype(object).sum(axis=2) * 2 ** (top - m.frac_bits)
        bound = 2 * v.pairs.astype(object) * 2 ** (top - min(m.frac_bits, v.frac2_bits))
        assert all(abs(int(x) - int(y)) <= int(z) for x, y, z in zip(a.ravel(), b.ravel(), bound.ravel()))
    finally:
        ctx.close()


def test_five_riders_with_windows_that_shift_between_replays():
    """Series every 7, removals every 5, frames every 3, profile every 11, van Hove every 13, graphs of 20 steps: no interval divides the
    graph's length, so the replays' windows differ.  `graph` against `single` (one vvhip_step_middle at a time), all five riders on in
    both; `truth` has the series and the removals on too (the removal changes the trajectory: like with like) and its frames at the
    recorder's steps."""
    spec = spec_for("C3")
    groups = groups_for(spec)
    (it1, graph), (it2, single), (it3, truth) = make("C3", spec), make("C3", spec), make("C3", spec)
    try:
        for c in (graph, single, truth):
            c.series_start(7, capacity=32)
            c.remove_cm_motion_every(5)
        for c in (graph, single):
            c.frames_start(3, capacity=64, velocities=True, float64=True)
            c.profile_start(11, 64, groups=groups, max_samples=100, charge=True, mass=True, momentum=True, kinetic=True)
            c.vanhove_start(13, 8, LOG_EDGES, 3, groups=groups, max_samples=100)
        truth.frames_start(13, capacity=32, float64=True)
        lay = graph.vanhove_info()
        graph.run_graph(130, 20)
        graph.run_eager(3)
        graph.run_graph(47, 20)
        for _ in range(180):
            it2.step(1)
        truth.run_graph(180, 20)
        vg, vs = graph.vanhove_read(), single.vanhove_read()
        assert (vg.samples, vg.dropped, vg.out_of_range) == (vs.samples, vs.dropped, vs.out_of_range) == (13, 0, 0)
        assert same_table(vg, vs)
        ft = truth.frames_read()
        assert list(ft.step) == list(range(13, 181, 13))
        assert_table(vg, expected(ft, spec, groups, lay, LOG_EDGES))
        assert vg.pairs.sum() > 0
        pg, ps = graph.profile_read(), single.profile_read()
        assert pg.samples == ps.samples == 16 and np.array_equal(pg.words, ps.words)
        fg, fs = graph.frames_read(), single.frames_read()
        assert list(fg.step) == list(fs.step) == list(range(3, 181, 3)) and fg.dropped == fs.dropped == 0
        assert eq(fg.positions, fs.positions) and eq(fg.velocities, fs.velocities)
        K.assert_same(K.state(graph), K.state(single), "replays against single steps")
    finally:
        for c in (graph, single, truth):
            c.close()


# ------------------------------------------------------------------------------------------ 8. stop and the checkpoint
def test_stop_and_the_checkpoint():
    spec = spec_for("C3")
    (it1, rec), (it2, plain) = make("C3", spec), make("C3", spec)
    try:
        rec.vanhove_start(10, 8, LOG_EDGES, 3, max_samples=100)
        rec.run_graph(200, 50)
        plain.run_graph(200, 50)
        assert rec.vanhove_read().samples == 20
        blob = plain.createCheckpoint()
        with pytest.raises(H.VVHipError) as e:
            rec.loadCheckpoint(blob)
        assert e.value.code == H.ERR_INVALID and "a self van Hove recorder is running: stop it, load, start it again" in str(e.value)
        rec.vanhove_stop()
        info = rec.vanhove_info()
        assert info.active == 0 and info.words == 0
        with pytest.raises(H.VVHipError):
            rec.vanhove_read()
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
        rec.vanhove_start(10, 8, LOG_EDGES, 3, max_samples=100)
        lay = rec.vanhove_info()
        assert lay.active == 1 and lay.start_step == 200
        rec.run_graph(50, 50)
        plain.run_graph(50, 50)
        v, f = rec.vanhove_read(), rec.frames_read()
        assert v.samples == 5 and list(f.step) == [210, 220, 230, 240, 250]
        assert_table(v, expected(f, spec, None, lay, LOG_EDGES))
        assert v.pairs.sum() > 0 and same_bits(state(rec), state(plain))
        rec.vanhove_stop()
        rec.frames_stop()
    finally:
        rec.close()
        plain.close()


def test_live_buffers_return_to_their_start_value_after_stop():
    spec = spec_for("C3")
    it, ctx = make("C3", spec)
    try:
        it.step(2)
        start = live_buffers()
        ctx.vanhove_start(1, 8, LOG_EDGES, 3, molecules=True, groups=groups_for(spec, True), max_samples=100)
        assert live_buffers() == start + 7                          # the words with the ring, index, first, weight, total, group, the squared edges
        it.step(5)
        assert ctx.vanhove_read().samples == 5
        ctx.vanhove_stop()
        assert live_buffers() == start
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 9. recovery
def test_a_repair_puts_table_and_ring_back_with_the_step_counter():
    """vvhip_debug_recover repairs on request, without anything having failed, exactly as the MSD's test does: the recorder's whole
    allocation, the ring of origins included, goes back with the step counter and the call is repeated.  A ring that did not go back
    shows as a different table, samples added twice as 23 samples."""
    spec = spec_for("C3")
    (it1, rec), (it2, calm) = make("C3", spec), make("C3", spec)
    try:
        for c in (rec, calm):
            c.run_graph(50, 50)
            c.vanhove_start(10, 2, LOG_EDGES, 1, groups=groups_for(spec), max_samples=100)
            c.run_graph(30, 10)                                     # three samples before the snapshot
            c.synchronize()
        assert rec.vanhove_info().num_origins == 2
        assert rec.fused_status()[0] and rec.recovery_count() == 0
        rec.run_graph(100, 50)
        calm.run_graph(100, 50)
        H.check(H.lib.vvhip_debug_recover(rec.plan), rec.plan)
        assert rec.recovery_count() == 1 and not rec.fused_status()[0] and rec.status_words() == [0, 0, 0, 0]
        v, q = rec.vanhove_read(), calm.vanhove_read()
        assert (v.samples, v.dropped, v.out_of_range, v.origin_floor) == (q.samples, q.dropped, q.out_of_range, q.origin_floor) == (13, 0, 0, 0)
        assert same_table(v, q) and v.pairs.sum() > 0
        assert same_bits(state(rec), state(calm))
        assert rec.series_info().steps == calm.series_info().steps == 180
    finally:
        rec.close()
        calm.close()


# ------------------------------------------------------------------------------------------ 10. the barostat
def test_barostat_moves_set_the_origin_floor():
    """scale_box and restore_box rewrite the positions outside the steps: origins stored before are dead, the table is kept."""
    spec = spec_for("C3")
    groups = groups_for(spec)
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(10, capacity=32, float64=True)
        ctx.vanhove_start(10, 8, LOG_EDGES, 1, groups=groups, max_samples=100)
        lay = ctx.vanhove_info()
        ctx.run_graph(50, 50)                                       # samples 0 .. 4
        before = ctx.vanhove_read()
        assert (before.samples, before.origin_floor) == (5, 0)
        ctx.scale_box((1.01, 0.99, 1.02))
        after = ctx.vanhove_read()
        assert (after.samples, after.origin_floor) == (5, 5) and same_table(after, before)      # the table is kept
        ctx.run_graph(40, 20)                                       # samples 5 .. 8
        assert ctx.vanhove_read().origin_floor == 5
        ctx.scale_box((1.05, 1.05, 1.05))
        assert ctx.vanhove_read().origin_floor == 9
        ctx.restore_box()
        ctx.run_graph(30, 10)                                       # samples 9 .. 11
        ctx.scale_box((0.99, 0.99, 0.99))
        ctx.restore_box()
        ctx.run_eager(30)                                           # samples 12 .. 14
        v, f = ctx.vanhove_read(), ctx.frames_read()
        assert (v.samples, v.origin_floor, v.out_of_range) == (15, 12, 0) and list(f.step) == list(range(10, 151, 10))
        floors = [0] * 5 + [5] * 4 + [9] * 3 + [12] * 3
        want = expected(f, spec, groups, lay, LOG_EDGES, floor=floors)
        assert want[2] == 0
        assert_table(v, want)
        assert v.pairs.sum() == lay.num_units * len(MR.pairs(15, 1, 8, floors)) > 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 11. a plan that never starts the recorder
def test_a_plan_that_never_starts_the_recorder_launches_what_it_launched_before():
    """Three contexts, one after the other, take the same 130 steps: one never hears of the recorder, one is asked for its info and told
    to stop (nothing was started), one starts and stops it before the steps.  Generic launches, the buffers the context holds after the
    steps and the state's digest agree."""
    spec = spec_for("C3")
    seen = []
    for touch in ("never", "info", "start-stop"):
        base = live_buffers()
        it, ctx = make("C3", spec)
        try:
            if touch != "never":
                assert ctx.vanhove_info().active == 0
                created = live_buffers()
                if touch == "start-stop":
                    ctx.vanhove_start(10, 8, LOG_EDGES, 3, max_samples=100)
                    assert live_buffers() == created + 2             # the words with the ring, and the squared edges
                ctx.vanhove_stop()
                assert ctx.vanhove_info().active == 0 and ctx.vanhove_info().words == 0 and live_buffers() == created
            ctx.run_graph(100, 50)
            ctx.run_eager(30)
            seen.append((ctx.generic_launches(), live_buffers() - base, ctx.state_digest()))
        finally:
            ctx.close()
        assert live_buffers() == base
    assert seen[1] == seen[0] and seen[2] == seen[0]
