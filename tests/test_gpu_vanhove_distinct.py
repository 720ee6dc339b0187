"""Device-side distinct van Hove functions (include/vvhip.h: vvhip_vanhove_distinct_*) on the GPU.  The ground truth needs no second
trajectory: the same context also runs the frame recorder (float64) at the same interval, and the expected table is
tests/vanhove_distinct_reference.py over those frames, each with the box its step ran with.  Every comparison is np.array_equal on
int64 (the float64 sums of 1 / V through their bits)."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vanhove_distinct_reference as DR      # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S, I = pkg.systems, pkg.integrator
H = I.H

pytestmark = pytest.mark.gpu

NH_FIELDS = ("eta", "eta_dot", "eta_dotdot", "ke2", "vscale", "v_bias")
SCALE = {"C1": 1.0, "C3": 0.1}
_SPECS = {}
CLASSES = [(0, 1), (0, 0), (1, 0)]


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


def two_groups(n, most=300):
    """Groups by particle index: every k-th particle in group 0, its successor in group 1, the rest no site; at most `most` sites each.
    Neighbours in index share a molecule, so the exclusion has pairs to leave out."""
    k = max(2, -(-n // most))
    g = np.full(n, -1, dtype=np.int8)
    g[np.arange(n) % k == 0] = 0
    g[np.arange(n) % k == 1] = 1
    return g


def short_r(spec):
    """0.6 nm, or less where the box is small: in range also after the barostat test's moves."""
    return min(0.6, 0.45 * float(min(spec.box)))


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


def expected(frames, which, groups, classes, lay, mol_id=None, floor=0):
    """(head, hist, invalid) of the reference over the frames `which` as samples 0, 1, ..., each with the box its step ran with."""
    assert eq(frames.particles, np.arange(len(frames.particles), dtype=np.int32))
    which = list(which)
    return DR.vanhove_distinct_reference(frames.positions[which], frames.box[which], groups, classes, lay.r_max, lay.nbins, lay.num_lags,
                                         lay.origin_every, mol_id, floor)


def assert_table(v, want, what=None):
    assert v.head.dtype == np.int64 and v.hist.dtype == np.int64
    assert np.array_equal(v.head, want[0]), what
    assert np.array_equal(v.hist, want[1]), what
    assert v.invalid == want[2], what


def same_table(a, b):
    return np.array_equal(a.head, b.head) and np.array_equal(a.hist, b.hist)


# ------------------------------------------------------------------------------------------ 1. tile edges, bins and every hook
def _tile_groups(n, tile):
    """Site counts of 1, 2, 255, 256, 257, 0 and 513; runs of the index, three particles without a site between them, and groups 4 and 6
    with one site in front of all runs."""
    sizes = [1, 2, tile - 1, tile, tile + 1, 0, 2 * tile + 1]
    apart = {4: 0, 6: 2}
    assert sum(sizes) + 7 * 3 <= n
    groups, at = np.full(n, -1, dtype=np.int8), 5
    for g, size in enumerate(sizes):
        run = size - (g in apart)
        groups[at:at + run] = g
        at += run + 3
    for g, i in apart.items():
        groups[i] = g
    assert [int(np.count_nonzero(groups == g)) for g in range(7)] == sizes
    return groups, sizes


TILE_CLASSES = [(g, g) for g in range(7)] + [(0, 4), (4, 0), (1, 3), (2, 6), (6, 2), (3, 4), (5, 2), (2, 5)]
TUNES = [None, {"vhd_hist_copies": 4}, {"vhd_items_target": 1}, {"vhd_items_target": 1 << 20}, {"vhd_lds": 0}, {"vhd_lds": 0, "vhd_items_target": 3},
         {"vhd_hist_copies": 4, "vhd_items_target": 7}]
_TILE = {}      # per description: (the frames' positions, the reference, the first tune's table)


@pytest.mark.parametrize("tune", TUNES, ids=["default", "hist_copies-4", "items_target-1", "items_target-2^20", "lds-0", "lds-0-items_target-3",
                                             "hist_copies-4-items_target-7"])
def test_tile_edges_bins_and_every_hook(tune):
    """Every description -- (nbins, r_max, exclusion) of (7, min(L) / 2, off), (8192, min(L) / 2, on), (1, 0.4, off), (1024, 0.5, off) --
    takes the next 5 steps of one context, a sample behind each, with two lags and every sample an origin: three ring slots, reused.  The
    hooks give every wave a histogram of its own, one block all the j-sites of its i-tile (three j-tiles for the group of 513), many
    small items, or plain global adds: the same table.  The reference is computed once, for the first tune's frames; the others' frames
    are the same bits."""
    spec = spec_for("C1")
    n = spec.num_atoms
    it, ctx = make("C1", spec, tune=tune)
    try:
        half = float(min(spec.box)) / 2
        mol = np.asarray(spec.mol_id)
        groups, sizes = None, None
        ctx.frames_start(1, capacity=32, float64=True)
        for k, (nbins, r_max, exclude) in enumerate([(7, half, False), (8192, half, True), (1, 0.4, False), (1024, 0.5, False)]):
            if groups is None:
                ctx.vanhove_distinct_start(1, 2, 0.5, 4, [(0, 0)])
                tile = int(ctx.vanhove_distinct_info().tile)
                assert tile == 256
                groups, sizes = _tile_groups(n, tile)
            ctx.vanhove_distinct_start(1, 2, r_max, nbins, TILE_CLASSES, groups=groups, exclude_same_molecule=exclude, max_samples=100)
            lay = ctx.vanhove_distinct_info()
            assert list(lay.num_sites[:7]) == sizes and (lay.num_origins, lay.num_rows, lay.nbins) == (2, 3, nbins)
            assert list(lay.pairs_per_sample[:len(TILE_CLASSES)]) == list(DR.pairs_per_sample(groups, TILE_CLASSES))
            assert lay.pairs_per_sample[0] == 0 and lay.pairs_per_sample[1] == 2 and lay.pairs_per_sample[6] == 513 * 512
            if tune and tune.get("vhd_items_target") == 1:
                assert lay.num_items == sum(-(-sizes[a] // tile) for a, b in TILE_CLASSES if sizes[b] and (a != b or sizes[a] > 1))      # one item per i-tile
            ctx.run_graph(5, 5) if k % 2 == 0 else ctx.run_eager(5)
            v, f = ctx.vanhove_distinct_read(), ctx.frames_read()
            assert list(f.step[5 * k:]) == list(range(5 * k + 1, 5 * k + 6))
            if k not in _TILE:
                _TILE[k] = (f.positions[5 * k:5 * k + 5].copy(), expected(f, range(5 * k, 5 * k + 5), groups, TILE_CLASSES, lay, mol if exclude else None), v)
            x, want, first = _TILE[k]
            assert eq(f.positions[5 * k:5 * k + 5], x)
            assert (v.samples, v.dropped, v.invalid, v.origin_floor) == (5, 0, 0, 0) and want[2] == 0
            assert_table(v, want, (k, nbins))
            assert same_table(v, first)
            assert list(v.visits) == [5, 4, 3] and not v.hist[[0, 5, 13, 14]].any()
            if not exclude:
                assert v.hist[6, 2].sum() > 0 and v.hist[10].sum() > 0
            assert np.array_equal(v.hist[7, 0], v.hist[8, 0]) and np.array_equal(v.hist[10, 0], v.hist[11, 0])      # row 0 is symmetric in the groups
        # a recorder whose only class has no sites still counts its samples and visits
        ctx.vanhove_distinct_start(1, 2, half, 8, [(5, 5)], groups=groups)
        ctx.run_eager(3)
        v = ctx.vanhove_distinct_read()
        assert (v.samples, v.dropped) == (3, 0) and not v.hist.any() and list(v.visits) == [3, 2, 1] and ctx.vanhove_distinct_info().num_items == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 2. the schedule: slots reused, the oldest origin read before it goes
@pytest.mark.parametrize("interval", [1, 7])
@pytest.mark.parametrize("num_lags,every", [(1, 1), (4, 1), (5, 2), (6, 3), (8, 8)])
def test_schedule_of_origins_and_lags(num_lags, every, interval):
    """2 R E + 3 samples: every slot of the ring is written at least twice, and where R E == num_lags the origin in the slot next to be
    overwritten still contributes at lag num_lags.  Graphs of 20 steps: with interval 7 the replays' windows shift."""
    spec = spec_for("C3")
    groups = two_groups(spec.num_atoms, most=150)
    R = DR.num_origins(num_lags, every)
    J = 2 * R * every + 3
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(interval, capacity=J + 1, float64=True)
        ctx.vanhove_distinct_start(interval, num_lags, short_r(spec), 48, CLASSES, origin_every=every, groups=groups, max_samples=1000)
        lay = ctx.vanhove_distinct_info()
        assert (lay.num_origins, lay.num_rows, lay.words) == (R, num_lags + 1, (num_lags + 1) * (2 + 3 * 48))
        ctx.run_graph(J * interval, 20)
        v, f = ctx.vanhove_distinct_read(), ctx.frames_read()
        assert list(f.step) == list(range(interval, J * interval + 1, interval)) and np.array_equal(v.lag_steps, np.arange(num_lags + 1) * interval)
        want = expected(f, range(J), groups, CLASSES, lay)
        assert (v.samples, v.dropped, v.invalid, v.origin_floor) == (J, 0, 0, 0)
        assert_table(v, want)
        l = np.arange(1, num_lags + 1)
        assert v.visits[0] == J and np.array_equal(v.visits[1:], (J - 1 - l) // every + 1) and v.visits[num_lags] >= 2
        assert np.all(v.hist.sum(axis=2)[:, v.visits > 0] > 0)
        assert eq(v.inv_volume_sum, want[0][:, 1].view(np.float64)) and np.all(v.inv_volume_sum[v.visits > 0] > 0)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 3. precisions and schemes
CASES = [("mixed", True), ("single", True), ("double", True), ("mixed", False), ("double", False)]


@pytest.mark.parametrize("precision,middle", CASES, ids=[f"{p}-{'middle' if m else 'classic'}" for p, m in CASES])
def test_table_equals_the_reference_over_the_frames(precision, middle):
    """The exclusion off and on take the next 60 steps each of one context, which records its own frames beside it; a context without a
    recorder runs the same steps."""
    spec = spec_for("C3")
    groups, mol = two_groups(spec.num_atoms), np.asarray(spec.mol_id)
    (_, rec), (_, plain) = make("C3", spec, precision, middle), make("C3", spec, precision, middle)
    try:
        rec.frames_start(10, capacity=16, float64=True)
        for k, exclude in enumerate((False, True)):
            rec.vanhove_distinct_start(10, 3, short_r(spec), 64, CLASSES, origin_every=2, groups=groups, exclude_same_molecule=exclude, max_samples=100)
            lay = rec.vanhove_distinct_info()
            assert (lay.active, lay.start_step, lay.exclude_same_molecule, lay.num_origins) == (1, 60 * k, int(exclude), 2)
            rec.run_graph(60, 20)
            v, f = rec.vanhove_distinct_read(), rec.frames_read()
            want = expected(f, range(6 * k, 6 * k + 6), groups, CLASSES, lay, mol if exclude else None)
            assert (v.samples, v.dropped, v.origin_floor) == (6, 0, 0)
            assert_table(v, want, exclude)
            assert list(v.visits) == [6, 3, 2, 2] and v.hist.sum() > 0
            assert np.array_equal(v.hist[0, 0], v.hist[2, 0])      # the sample against itself: (a, b) and (b, a) are one histogram
            G = v.G_d(1)
            assert G.shape == (4, 64) and np.all(np.isfinite(G))
        plain.run_graph(120, 20)
        assert same_bits(state(rec), state(plain))                  # the recorder changes nothing of the run
    finally:
        rec.close()
        plain.close()


# ------------------------------------------------------------------------------------------ 4. stepping paths and the graph cache
def _scheduled(path, interval, n=117):
    spec = spec_for("C3")
    it, ctx = make("C3", spec, tune={"fused": 0} if path == "unfused" else None)
    try:
        it.step(3)                                                  # an unaligned start, host-driven
        ctx.vanhove_distinct_start(interval, 5, short_r(spec), 32, CLASSES, origin_every=2, groups=two_groups(spec.num_atoms), max_samples=100)
        assert ctx.vanhove_distinct_info().start_step == 3
        if path == "step":
            it.step(n)
        elif path in ("eager", "unfused"):
            ctx.run_eager(n)
        else:
            ctx.run_graph(n, 20)
        return ctx.vanhove_distinct_read()
    finally:
        ctx.close()


@pytest.mark.parametrize("interval", [7, 20])
def test_every_stepping_path_gives_the_same_table(interval):
    g = _scheduled("graph", interval)
    assert g.samples == 120 // interval and g.dropped == 0 and g.invalid == 0 and g.hist.sum() > 0 and g.visits[-1] > 0
    for path in ("step", "eager", "unfused"):
        v = _scheduled(path, interval)
        assert (v.samples, v.dropped, v.invalid) == (g.samples, 0, 0) and same_table(v, g), path


def test_steady_state_replays_capture_nothing():
    spec = spec_for("C3")
    it, ctx = make("C3", spec)
    try:
        ctx.vanhove_distinct_start(50, 4, short_r(spec), 32, CLASSES, origin_every=2, groups=two_groups(spec.num_atoms))
        ctx.run_graph(400, 50)
        before = ctx.series_info().graph_captures
        ctx.run_graph(300, 50)
        assert ctx.series_info().graph_captures == before, (before, ctx.series_info().graph_captures)
        v = ctx.vanhove_distinct_read()
        assert v.samples == 14 and list(v.visits) == [14, 7, 6, 6, 5]
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 5. beside other recorders
def test_row_zero_is_the_rdf_recorder_running_beside_it():
    spec = spec_for("C3")
    groups = two_groups(spec.num_atoms)
    it, ctx = make("C3", spec)
    try:
        for exclude in (False, True):
            ctx.rdf_start(10, short_r(spec), 128, [(0, 1), (0, 0), (1, 1)], groups=groups, exclude_same_molecule=exclude)
            ctx.vanhove_distinct_start(10, 2, short_r(spec), 128, [(0, 1), (0, 0), (1, 1), (1, 0)], groups=groups, exclude_same_molecule=exclude)
            ctx.run_graph(40, 20)
            r, v = ctx.rdf_read(), ctx.vanhove_distinct_read()
            assert r.samples == v.samples == v.visits[0] == 4 and r.counts.sum() > 0
            assert np.array_equal(v.hist[0, 0], r.counts[0]) and np.array_equal(v.hist[3, 0], r.counts[0])
            assert np.array_equal(v.hist[1, 0], 2 * r.counts[1]) and np.array_equal(v.hist[2, 0], 2 * r.counts[2])
            assert eq(v.inv_volume_sum[:1], np.array([r.inv_volume_sum]))
            g = r.g()
            assert eq(v.g(0), g[0]) and eq(v.g(1), g[1]) and eq(v.g(2), g[2])
    finally:
        ctx.close()


def test_beside_the_self_van_hove_and_msd_recorders():
    """MSD every 7, self van Hove every 10, distinct van Hove every 10, frames every 10, graphs of 20 steps with an eager stretch between:
    beside a context with the first two only, those give what they give there, and the distinct part the reference over the frames."""
    spec = spec_for("C3")
    groups = two_groups(spec.num_atoms)
    edges = I.vanhove_edges(0.2, 32, 1e-4)
    (it1, three), (it2, two) = make("C3", spec), make("C3", spec)
    try:
        for c in (three, two):
            c.msd_start(7, 4, 2, groups=groups, max_samples=100)
            c.vanhove_start(10, 4, edges, 2, groups=groups, max_samples=100)
        three.frames_start(10, capacity=16, float64=True)
        three.vanhove_distinct_start(10, 4, short_r(spec), 100, CLASSES, origin_every=2, groups=groups, exclude_same_molecule=True)
        lay = three.vanhove_distinct_info()
        for c in (three, two):
            c.run_graph(40, 20)
            c.run_eager(3)
            c.run_graph(37, 20)
        m3, m2 = three.msd_read(), two.msd_read()
        assert m3.samples == m2.samples == 11 and np.array_equal(m3.words, m2.words) and m3.pairs.sum() > 0
        s3, s2 = three.vanhove_read(), two.vanhove_read()
        assert s3.samples == s2.samples == 8 and np.array_equal(s3.head, s2.head) and np.array_equal(s3.hist, s2.hist) and s3.pairs.sum() > 0
        v, f = three.vanhove_distinct_read(), three.frames_read()
        assert list(f.step) == list(range(10, 81, 10)) and (v.samples, v.dropped) == (8, 0)
        assert_table(v, expected(f, range(8), groups, CLASSES, lay, np.asarray(spec.mol_id)))
        assert v.hist[:, 4].sum() > 0
        assert same_bits(state(three), state(two))
    finally:
        three.close()
        two.close()


# ------------------------------------------------------------------------------------------ 6. max_samples, reset
def test_max_samples_and_reset():
    spec = spec_for("C3")
    groups = two_groups(spec.num_atoms)
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(10, capacity=16, float64=True)
        ctx.vanhove_distinct_start(10, 4, short_r(spec), 40, CLASSES, origin_every=2, groups=groups, max_samples=5)
        lay = ctx.vanhove_distinct_info()
        ctx.run_graph(100, 50)
        v = ctx.vanhove_distinct_read(reset=True)
        f = ctx.frames_read()
        assert (v.samples, v.dropped) == (5, 5) and list(f.step) == list(range(10, 101, 10))
        assert_table(v, expected(f, range(5), groups, CLASSES, lay))
        z = ctx.vanhove_distinct_read()
        assert (z.samples, z.dropped, z.invalid, z.origin_floor) == (0, 0, 0, 0) and not z.head.any() and not z.hist.any()
        # the schedule continues without gap or repeat; the ordinal restarts at 0 with no live origin (the ring still holds the old ones)
        ctx.run_graph(40, 50)
        t, f = ctx.vanhove_distinct_read(), ctx.frames_read()
        assert list(f.step[10:]) == [110, 120, 130, 140] and (t.samples, t.dropped) == (4, 0)
        assert_table(t, expected(f, range(10, 14), groups, CLASSES, lay))
        assert list(t.visits) == [4, 2, 1, 1, 0]
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 7. the box
def test_box_changes_set_the_floor_and_a_small_box_drops_the_sample():
    """scale_box / restore_box and setPeriodicBoxSize put the floor at the current ordinal; a sample in a box that no longer holds r_max
    adds nothing, stores nothing, leaves the ordinal, puts the floor there and counts as dropped."""
    spec = spec_for("C3")
    groups = two_groups(spec.num_atoms)
    box = np.asarray(spec.box, dtype=np.float64)
    r_max = short_r(spec)
    it, ctx = make("C3", spec)
    try:
        ctx.frames_start(10, capacity=32, float64=True)
        ctx.vanhove_distinct_start(10, 6, r_max, 50, CLASSES, groups=groups, max_samples=100)
        lay = ctx.vanhove_distinct_info()
        ctx.run_graph(30, 10)                                       # samples 0 .. 2 (frames 0 .. 2)
        before = ctx.vanhove_distinct_read()
        assert (before.samples, before.origin_floor) == (3, 0)
        ctx.scale_box((1.01, 0.99, 1.02))
        after = ctx.vanhove_distinct_read()
        assert (after.samples, after.origin_floor) == (3, 3) and same_table(after, before)      # the table is kept
        ctx.run_graph(20, 20)                                       # samples 3, 4 (frames 3, 4)
        ctx.scale_box((1.05, 1.05, 1.05))
        assert ctx.vanhove_distinct_read().origin_floor == 5
        ctx.restore_box()
        ctx.run_eager(20)                                           # samples 5, 6 (frames 5, 6)
        now = np.asarray(ctx.barostat_record().box_before, dtype=np.float64)
        ctx.setPeriodicBoxSize(*now)                                # the same box: nothing happens
        assert ctx.vanhove_distinct_read().origin_floor == 5
        ctx.setPeriodicBoxSize(*(now * 1.001))
        assert ctx.vanhove_distinct_read().origin_floor == 7
        ctx.run_graph(10, 10)                                       # sample 7 (frame 7)
        small = np.full(3, 2 * r_max * 0.99)
        ctx.setPeriodicBoxSize(*small)
        assert ctx.vanhove_distinct_read().origin_floor == 8
        ctx.run_graph(20, 10)                                       # two samples dropped (frames 8, 9)
        d = ctx.vanhove_distinct_read()
        assert (d.samples, d.dropped, d.origin_floor) == (8, 2, 8)
        ctx.setPeriodicBoxSize(*(now * 1.001))
        ctx.run_eager(30)                                           # samples 8 .. 10 (frames 10 .. 12)
        v, f = ctx.vanhove_distinct_read(), ctx.frames_read()
        assert (v.samples, v.dropped, v.origin_floor, v.invalid) == (11, 2, 8, 0) and list(f.step) == list(range(10, 131, 10))
        which = list(range(8)) + [10, 11, 12]
        floors = [0] * 3 + [3] * 2 + [5] * 2 + [7] + [8] * 3
        want = expected(f, which, groups, CLASSES, lay, floor=floors)
        assert_table(v, want)
        assert list(v.visits) == [11, 2 + 1 + 1 + 0 + 2, 1 + 1, 0, 0, 0, 0]
        assert not eq(f.box[0], f.box[3]) and not eq(f.box[6], f.box[7])
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 8. stop, the checkpoint, a sharded plan
def test_stop_and_the_checkpoint():
    spec = spec_for("C3")
    groups = two_groups(spec.num_atoms)
    (it1, rec), (it2, plain) = make("C3", spec), make("C3", spec)
    try:
        rec.run_eager(2)
        plain.run_eager(2)
        rec.vanhove_distinct_start(10, 4, short_r(spec), 32, CLASSES, origin_every=2, groups=groups, exclude_same_molecule=True)
        rec.run_graph(98, 50)
        plain.run_graph(98, 50)
        assert rec.vanhove_distinct_read().samples == 10
        blob = plain.createCheckpoint()
        with pytest.raises(H.VVHipError) as e:
            rec.loadCheckpoint(blob)
        assert e.value.code == H.ERR_INVALID and "a distinct van Hove recorder is running: stop it, load, start it again" in str(e.value)
        rec.vanhove_distinct_stop()
        info = rec.vanhove_distinct_info()
        assert info.active == 0 and info.words == 0
        with pytest.raises(H.VVHipError):
            rec.vanhove_distinct_read()
        # stopped: further steps as if there never was a recorder
        rec.run_graph(100, 50)
        rec.run_eager(13)
        plain.run_graph(100, 50)
        plain.run_eager(13)
        assert same_bits(state(rec), state(plain))
        # stop, load, start works: the recorder begins at the loaded step counter
        rec.loadCheckpoint(blob)
        rec.frames_start(10, capacity=8, float64=True)
        rec.vanhove_distinct_start(10, 4, short_r(spec), 32, CLASSES, origin_every=2, groups=groups)
        lay = rec.vanhove_distinct_info()
        assert lay.active == 1 and lay.start_step == 100
        rec.run_graph(50, 50)
        v, f = rec.vanhove_distinct_read(), rec.frames_read()
        assert v.samples == 5 and list(f.step) == [110, 120, 130, 140, 150]
        assert_table(v, expected(f, range(5), groups, CLASSES, lay))
    finally:
        rec.close()
        plain.close()


def test_live_buffers_return_to_their_start_value_after_stop():
    spec = spec_for("C3")
    it, ctx = make("C3", spec)
    try:
        it.step(2)
        start = live_buffers()
        ctx.vanhove_distinct_start(1, 4, short_r(spec), 32, CLASSES, origin_every=2, groups=two_groups(spec.num_atoms), exclude_same_molecule=True)
        assert live_buffers() == start + 4                          # the words with the ring, index, mol, the work items
        it.step(5)
        assert ctx.vanhove_distinct_read().samples == 5
        ctx.vanhove_distinct_stop()
        assert live_buffers() == start
    finally:
        ctx.close()


def test_a_sharded_plan_is_refused():
    spec = spec_for("C3")
    n = spec.num_atoms
    mol = np.asarray(spec.mol_id)
    cut = int(np.nonzero(mol == mol[n // 2])[0].min())              # a molecule boundary
    it = integrator_for("C3", spec)
    it.setUseCOMTempGroup(False)
    ctx = I.Context(spec, it, precision="mixed", force_provider="tether", shard=(0, cut))
    try:
        with pytest.raises(H.VVHipError) as e:
            ctx.vanhove_distinct_start(10, 4, short_r(spec), 32, CLASSES, groups=two_groups(n))
        assert e.value.code == H.ERR_UNSUPPORTED and "shard" in str(e.value) and ctx.vanhove_distinct_info().active == 0
        ctx.run_eager(3)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 9. recovery
def test_a_repair_puts_table_ring_and_ordinal_back_with_the_step_counter():
    """vvhip_debug_recover repairs on request, without anything having failed, exactly as the self recorder's test does: the recorder's
    whole allocation, the ring of origins included, goes back with the step counter and the call is repeated.  A ring that did not go
    back shows as a different table, samples added twice as 23 samples."""
    spec = spec_for("C3")
    groups = two_groups(spec.num_atoms)
    (it1, rec), (it2, calm) = make("C3", spec), make("C3", spec)
    try:
        for c in (rec, calm):
            c.run_graph(50, 50)
            c.vanhove_distinct_start(10, 2, short_r(spec), 64, CLASSES, groups=groups, max_samples=100)
            c.run_graph(30, 10)                                     # three samples before the snapshot
            c.synchronize()
        assert rec.vanhove_distinct_info().num_origins == 2
        assert rec.fused_status()[0] and rec.recovery_count() == 0
        rec.run_graph(100, 50)
        calm.run_graph(100, 50)
        H.check(H.lib.vvhip_debug_recover(rec.plan), rec.plan)
        assert rec.recovery_count() == 1 and not rec.fused_status()[0] and rec.status_words() == [0, 0, 0, 0]
        v, q = rec.vanhove_distinct_read(), calm.vanhove_distinct_read()
        assert (v.samples, v.dropped, v.invalid, v.origin_floor) == (q.samples, q.dropped, q.invalid, q.origin_floor) == (13, 0, 0, 0)
        assert same_table(v, q) and v.hist.sum() > 0 and list(v.visits) == [13, 12, 11]
        assert same_bits(state(rec), state(calm))
        assert rec.series_info().steps == calm.series_info().steps == 180
    finally:
        rec.close()
        calm.close()


# ------------------------------------------------------------------------------------------ 10. a plan that never starts the recorder
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
                assert ctx.vanhove_distinct_info().active == 0
                created = live_buffers()
                if touch == "start-stop":
                    ctx.vanhove_distinct_start(10, 8, short_r(spec), 32, CLASSES, origin_every=3, groups=two_groups(spec.num_atoms))
                    assert live_buffers() == created + 3             # the words with the ring, index, the work items
                ctx.vanhove_distinct_stop()
                assert ctx.vanhove_distinct_info().active == 0 and ctx.vanhove_distinct_info().words == 0 and live_buffers() == created
            ctx.run_graph(100, 50)
            ctx.run_eager(30)
            seen.append((ctx.generic_launches(), live_buffers() - base, ctx.state_digest()))
        finally:
            ctx.close()
        assert live_buffers() == base
    assert seen[1] == seen[0] and seen[2] == seen[0]
