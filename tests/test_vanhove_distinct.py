"""Device-side distinct van Hove functions (include/vvhip.h: vvhip_vanhove_distinct_*), the host half, no GPU:
tests/vanhove_distinct_reference.py against a plain triple loop, row 0 against the RDF's reference, the time-reversal symmetry of the
ordered classes, the layout and the word cap of an unbound plan, every refusal of the start in its documented order, the struct sizes,
the Python views on a hand-made table (g(c) equal to Rdf.g on the same numbers), the text writer read back, the digest of the host
tables."""
import ctypes as C
import importlib
import io
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rdf_reference as RR                  # noqa: E402
import vanhove_distinct_reference as DR     # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S = pkg.systems
R = pkg.reporters

ENTRY_POINTS = ("vvhip_vanhove_distinct_start", "vvhip_vanhove_distinct_read", "vvhip_vanhove_distinct_stop", "vvhip_vanhove_distinct_info")


def _I():
    return importlib.import_module("openmm-velocityverlet_amd.integrator")


_SPEC = {}


def _spec():
    if "s" not in _SPEC:
        _SPEC["s"] = S.make_config("C3", scale=0.05)
    return _SPEC["s"]


def _plan(shard=None, box=None):
    I = _I()
    it = I.VVIntegrator(333.0, 10.0, 1.0, 40.0, 0.001)
    plan, _, keep = I.create_plan(_spec(), it, "mixed", shard)
    if box is not None:
        b = (C.c_double * 3)(*box)
        assert I.H.lib.vvhip_set_box(plan, C.byref(b)) == I.H.OK
    return plan, keep


def _describe(plan, interval=10, num_lags=8, origin_every=1, nbins=64, num_groups=1, classes=((0, 0),), exclude=0, group=None, max_samples=1000,
              r_max=0.5, num_classes=None, null_classes=False):
    """vvhip_vanhove_distinct_start on an unbound plan: (return code, error text); a description that passes the checks in front of the
    bind is kept."""
    H = _I().H
    grp = None if group is None else np.ascontiguousarray(group, dtype=np.int8)
    cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1, 2)
    desc = H.VanHoveDistinctDesc(interval, num_lags, origin_every, nbins, num_groups, len(cls) if num_classes is None else num_classes, exclude, 0,
                                 None if grp is None else grp.ctypes.data, None if null_classes else cls.ctypes.data, max_samples, r_max)
    rc = H.lib.vvhip_vanhove_distinct_start(plan, C.byref(desc))
    return rc, H.lib.vvhip_last_error(plan).decode()


def _info(plan):
    H = _I().H
    lay = H.VanHoveDistinctLayout()
    assert H.lib.vvhip_vanhove_distinct_info(plan, C.byref(lay)) == H.OK
    return lay


def test_entry_points_and_struct_sizes():
    H = _I().H
    for name in ENTRY_POINTS:
        assert name in H.EXPORTS and hasattr(H.lib, name)
    header = open(os.path.join(ROOT, "include", "vvhip.h")).read()
    for name in ENTRY_POINTS:
        assert "int %s(" % name in header
    assert "vvhip_vanhove_distinct_sample" not in header             # no manual sample: a sample is a step of the lag schedule
    assert C.sizeof(H.VanHoveDistinctDesc) == 64 and C.sizeof(H.VanHoveDistinctCounts) == 32
    assert C.sizeof(H.VanHoveDistinctLayout) == 12 * 4 + 16 * 4 + 64 * 4 + 32 * 8 + 6 * 8 + 2 * 8
    assert H.VANHOVE_DISTINCT_MAX_WORDS == DR.MAX_WORDS and "#define VVHIP_VANHOVE_DISTINCT_MAX_WORDS (1ll << 22)" in header


# ------------------------------------------------------------------------------------------ the reference against a plain loop
def _loop(x, boxes, groups, classes, r_max, nbins, num_lags, every, mol_id, floors):
    """The statement, one scalar at a time (Python floats are float64; round() is round-half-even)."""
    dr = r_max / nbins
    e = [(k * dr) * (k * dr) for k in range(nbins + 1)]
    rows = num_lags + 1
    visits, ivs = [0] * rows, [0.0] * rows
    hist, invalid = np.zeros((len(classes), rows, nbins), dtype=np.int64), 0
    n = len(x[0])
    for j in range(len(x)):
        box = boxes[j]
        origins = [(j, 0)] + [(o, j - o) for o in range(0, j, every) if o >= floors[j] and j - o <= num_lags]
        for o, row in origins:
            visits[row] += 1
            ivs[row] = ivs[row] + 1.0 / ((box[0] * box[1]) * box[2])
            for c, (ga, gb) in enumerate(classes):
                for i in range(n):
                    if groups[i] != ga:
                        continue
                    for k in range(n):
                        if groups[k] != gb or (ga == gb and i == k) or (mol_id is not None and mol_id[i] == mol_id[k]):
                            continue
                        d = []
                        for a in range(3):
                            t = x[j][k][a] - x[o][i][a]
                            q = t * (1.0 / box[a])
                            if math.isnan(q):
                                d.append(float("nan"))
                                continue
                            d.append(t - box[a] * float(round(q)))
                        r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                        if math.isnan(r2):
                            invalid += 1
                            continue
                        for b in range(nbins):
                            if e[b] <= r2 < e[b + 1]:
                                hist[c, row, b] += 1
    head = np.stack([np.array(visits, dtype=np.int64), np.array(ivs, dtype=np.float64).view(np.int64)], axis=1)
    return head, hist, invalid


def _sequence(rng, J, n, nan=True):
    """J samples of n sites drifting through several images of the box, one pair exactly on an edge of (1.0, 8), one of distance 0."""
    x0 = rng.uniform(-4.0, 7.0, size=(n, 3))
    x = x0[None] + np.cumsum(rng.normal(0.0, 0.2, size=(J, n, 3)), axis=0)
    x[0, 5] = x[0, 4] + np.array([0.25, 0.0, 0.0])
    x[1, 9] = x[0, 8]                                                # site 9 at sample 1 exactly where site 8 was at sample 0
    if nan:
        x[2, 7, 1] = np.nan
    return x


@pytest.mark.parametrize("exclude", [False, True], ids=["all-pairs", "exclude-same-molecule"])
@pytest.mark.parametrize("num_lags,every,floor", [(1, 1, 0), (4, 1, 0), (5, 2, 0), (6, 3, 0), (5, 2, 3)])
def test_reference_equals_a_plain_loop(exclude, num_lags, every, floor):
    rng = np.random.default_rng(11)
    n, J = 12, 2 * DR.num_origins(num_lags, every) * every + 3
    x = _sequence(rng, J, n)
    boxes = np.array([2.5, 3.0, 2.75]) * (1.0 + 0.01 * np.arange(J))[:, None]      # a box that changes from sample to sample
    groups = np.array([0, 1, 0, 2, 0, 1, -1, 1, 0, 0, 2, 1], dtype=np.int8)
    mol_id = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 5, 5])
    classes = [(0, 1), (0, 0), (2, 2), (1, 0)]
    floors = [0] * 4 + [floor] * (J - 4)
    got = DR.vanhove_distinct_reference(x, boxes, groups, classes, 1.0, 8, num_lags, every, mol_id if exclude else None, floors)
    want = _loop(x.tolist(), boxes.tolist(), groups.tolist(), classes, 1.0, 8, num_lags, every, mol_id.tolist() if exclude else None, floors)
    assert got[2] == want[2] > 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].sum() > 0
    assert got[0][0, 0] == J and np.all(got[0][1:, 0] > 0)           # every row is visited: slots are reused
    if floor == 0:
        l = np.arange(1, num_lags + 1)
        assert np.array_equal(got[0][1:, 0], np.maximum(0, (J - 1 - l) // every + 1))


# ------------------------------------------------------------------------------------------ row 0 is the RDF
def test_row_zero_is_the_rdf_reference_and_twice_it_for_one_group():
    rng = np.random.default_rng(5)
    n, J = 12, 4
    x = _sequence(rng, J, n)
    box = np.array([2.5, 3.0, 2.75])
    groups = np.array([0, 1, 0, 1, 0, 1, -1, 1, 0, 0, 0, 1], dtype=np.int8)
    mol_id = np.arange(n) // 2
    classes = [(0, 1), (0, 0), (1, 0), (1, 1)]
    for exclude in (None, mol_id):
        head, hist, invalid = DR.vanhove_distinct_reference(x, box, groups, classes, 1.2, 16, 2, 1, exclude)
        rdf, bad = np.zeros((4, 16), dtype=np.int64), 0
        for j in range(J):
            t, b = RR.rdf_reference(x[j], box, groups, classes, 1.2, 16, exclude)
            rdf += t
            bad += b
        assert np.array_equal(hist[0, 0], rdf[0]) and np.array_equal(hist[2, 0], rdf[2]) and np.array_equal(hist[0, 0], hist[2, 0])
        assert np.array_equal(hist[1, 0], 2 * rdf[1]) and np.array_equal(hist[3, 0], 2 * rdf[3]) and rdf[1].sum() > 0
        assert head[0, 0] == J and head[0, 1:2].view(np.float64)[0] == RR.inv_volume_sum([box] * J)
    assert list(DR.pairs_per_sample(groups, classes)) == [6 * 5, 6 * 5, 5 * 6, 5 * 4]
    assert list(DR.pairs_per_sample(groups, [(0, 0), (0, 1)])) == [2 * RR.pairs_per_sample(groups, [(0, 0)])[0], RR.pairs_per_sample(groups, [(0, 1)])[0]]


# ------------------------------------------------------------------------------------------ time reversal
@pytest.mark.parametrize("num_lags", [1, 4])
def test_row_l_of_a_class_is_row_l_of_the_swapped_class_on_the_reversed_sequence(num_lags):
    """d = X_j(t) - X_i(0) forwards is -(X_i(0') - X_j(t')) backwards, and r2 is even in d: with E = 1 and num_lags + 1 samples every
    pair of samples (o, j) is visited once in either direction."""
    rng = np.random.default_rng(7)
    n, J = 12, num_lags + 1
    x = _sequence(rng, J, n, nan=False)
    box = np.array([2.5, 3.0, 2.75])
    groups = np.array([0, 1, 0, 1, 0, 1, -1, 1, 0, 0, 1, 1], dtype=np.int8)
    forward = DR.vanhove_distinct_reference(x, box, groups, [(0, 1), (1, 0), (0, 0)], 1.2, 16, num_lags, 1)
    backward = DR.vanhove_distinct_reference(x[::-1], box, groups, [(1, 0), (0, 1), (0, 0)], 1.2, 16, num_lags, 1)
    assert np.array_equal(forward[0], backward[0]) and np.array_equal(forward[1], backward[1]) and forward[1][:, 1:].sum() > 0
    assert not np.array_equal(forward[1][0, 1:], forward[1][1, 1:])  # (the ordered classes do differ at a lag)


# ------------------------------------------------------------------------------------------ the layout of an unbound plan
def test_layout_of_an_unbound_plan_and_the_word_cap():
    H = _I().H
    spec = _spec()
    n = spec.num_atoms
    plan, keep = _plan(box=(3.0, 3.2, 3.4))
    try:
        lay = _info(plan)
        assert (lay.active, lay.words, lay.nbins, lay.num_rows, lay.ring_bytes) == (0, 0, 0, 0, 0)
        assert H.lib.vvhip_vanhove_distinct_stop(plan) == H.OK
        groups = (np.arange(n) % 3).astype(np.int8) - 1               # -1, 0, 1
        classes = [(0, 1), (0, 0), (1, 1), (1, 0)]
        rc, text = _describe(plan, interval=7, num_lags=5, origin_every=2, nbins=300, num_groups=2, classes=classes, group=groups, r_max=1.5, exclude=1,
                             max_samples=123)
        assert rc == H.ERR_INVALID and "vvhip_bind has not been called" in text
        lay = _info(plan)
        n0, n1 = int(np.count_nonzero(groups == 0)), int(np.count_nonzero(groups == 1))
        assert (lay.active, lay.interval, lay.num_lags, lay.origin_every, lay.nbins, lay.num_groups, lay.num_classes) == (0, 7, 5, 2, 300, 2, 4)
        assert (lay.exclude_same_molecule, lay.max_samples, lay.num_origins, lay.num_rows) == (1, 123, 3, 6) and lay.num_origins == DR.num_origins(5, 2)
        assert list(lay.num_sites[:3]) == [n0, n1, 0]
        assert [tuple(lay.classes[c]) for c in range(4)] == classes
        assert list(lay.pairs_per_sample[:5]) == [n0 * n1, n0 * (n0 - 1), n1 * (n1 - 1), n1 * n0, 0]
        assert list(lay.pairs_per_sample[:4]) == list(DR.pairs_per_sample(groups, classes))
        assert lay.dr == 1.5 / 300 and lay.r_max == 1.5
        assert (lay.head_words, lay.hist_words, lay.words) == (6 * 2, 4 * 6 * 300, 6 * 2 + 4 * 6 * 300)
        stride = (n0 + n1 + 15) // 16 * 16
        assert lay.ring_bytes == (3 + 2) * 3 * stride * 8 and lay.tile >= 64 and lay.tile % 64 == 0
        # a small workload: per i-tile ALL the j-sites in runs of 64, also for a class of one group with itself
        runs = lambda na, nb: -(-na // lay.tile) * -(-nb // 64)
        assert lay.num_items == runs(n0, n1) + runs(n0, n0) + runs(n1, n1) + runs(n1, n0)
        # the word cap: (num_lags + 1) * (2 + num_classes * nbins) <= 2^22, refused with the count
        rc, text = _describe(plan, num_lags=510, nbins=8192, r_max=1.5)
        assert rc == H.ERR_INVALID and "vvhip_bind has not been called" in text and _info(plan).words == 511 * 8194 <= DR.MAX_WORDS
        rc, text = _describe(plan, num_lags=511, nbins=8192, r_max=1.5)
        assert rc == H.ERR_INVALID and str(512 * 8194) in text and "above the cap" in text and 512 * 8194 > DR.MAX_WORDS
        assert _info(plan).words == 511 * 8194                       # (a refused description leaves the one before it in place)
        assert H.lib.vvhip_vanhove_distinct_stop(plan) == H.OK and _info(plan).words == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)


# ------------------------------------------------------------------------------------------ the refusals, in their order
def test_start_refuses_in_the_documented_order():
    """Everything wrong at once, then one thing put right at a time: the error names the next one."""
    H = _I().H
    n = _spec().num_atoms
    bad_group = np.zeros(n, dtype=np.int8)
    bad_group[3] = 2
    pairs = n * (n - 1)
    plan, keep = _plan(box=(2.0, 2.0, 2.0))
    try:
        assert H.lib.vvhip_vanhove_distinct_start(plan, None) == H.ERR_INVALID and "null description" in H.lib.vvhip_last_error(plan).decode()
        kw = dict(interval=0, num_lags=5000, origin_every=0, r_max=float("inf"), nbins=8193, num_groups=17, num_classes=33, null_classes=True,
                  max_samples=0, group=bad_group, classes=[(0, 1), (0, 5)])
        steps = [("interval must be >= 1", dict(interval=10)), ("num_lags must be in [1, 4096]", dict(num_lags=4096)),
                 ("origin_every must be in [1, num_lags]", dict(origin_every=1)), ("r_max must be finite and > 0", dict(r_max=-1.0)),
                 ("r_max must be finite and > 0", dict(r_max=1.5)), ("nbins must be in [1, 8192]", dict(nbins=0)),
                 ("nbins must be in [1, 8192]", dict(nbins=8192)), ("num_groups must be in [1, 16]", dict(num_groups=2)),
                 ("num_classes must be in [1, 32]", dict(num_classes=None)), ("classes must not be NULL", dict(null_classes=False)),
                 ("max_samples must be >= 1", dict(max_samples=1 << 62)), ("group[3] = 2 is outside [-1, num_groups = 2)", dict(group=None)),
                 ("classes[1][1] = 5 is outside [0, num_groups = 2)", dict(classes=[(0, 0)])),
                 ("above the cap", dict(nbins=8)),                    # 4097 * (2 + 8192) words
                 ("num_origins = ceil(num_lags / origin_every) = 4096 is above 1024", dict(origin_every=4)),
                 ("reaches 2^62", dict(max_samples=(1 << 62) // pairs + 1)),
                 ("reaches 2^62", dict(max_samples=((1 << 62) - 1) // pairs)),
                 ("above half the shortest edge of the box", dict(r_max=1.0)),      # exactly min(L) / 2 passes
                 ("vvhip_bind has not been called", None)]
        for text, fix in steps:
            rc, err = _describe(plan, **kw)
            assert rc == H.ERR_INVALID and text in err, (text, rc, err)
            if fix:
                assert _info(plan).words == 0                        # nothing of a refused description is kept
                kw.update(fix)
        lay = _info(plan)
        assert lay.words == 4097 * (2 + 8) and lay.num_origins == 1024 and lay.active == 0 and lay.pairs_per_sample[0] == pairs
        # the rest of the surface on an unbound plan
        assert H.lib.vvhip_vanhove_distinct_read(plan, None, 0, None, 0) == H.ERR_INVALID
        assert H.lib.vvhip_vanhove_distinct_stop(plan) == H.OK and _info(plan).words == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)
    # a sharded plan: behind the box, in front of the bind
    mol = np.asarray(_spec().mol_id)
    cut = int(np.nonzero(mol == mol[n // 2])[0].min())                # a molecule boundary
    assert 0 < cut < n
    plan, keep = _plan(shard=(0, cut), box=(2.0, 2.0, 2.0))
    try:
        rc, err = _describe(plan, r_max=1.5)
        assert rc == H.ERR_INVALID and "above half the shortest edge" in err
        rc, err = _describe(plan, r_max=1.0)
        assert rc == H.ERR_UNSUPPORTED and "shard" in err and "partial histogram" in err
        assert _info(plan).words == 0 and _info(plan).active == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)


# ------------------------------------------------------------------------------------------ the Python views, the writer
def _hand_made(hist, visits, volumes, r_max, classes, num_sites, interval=10, every=1):
    """A VanHoveDistinct from hist [classes, rows, bins], the rows' visits and the volume of every visit's box (one number: all the same)."""
    I = _I()
    hist = np.asarray(hist, dtype=np.int64)
    classes = np.asarray(classes, dtype=np.int32).reshape(-1, 2)
    num_sites = np.asarray(num_sites, dtype=np.int64)
    pps = np.array([num_sites[a] * (num_sites[a] - 1) if a == b else num_sites[a] * num_sites[b] for a, b in classes], dtype=np.int64)
    ivs = np.array([v / volumes for v in visits], dtype=np.float64)
    head = np.stack([np.asarray(visits, dtype=np.int64), ivs.view(np.int64)], axis=1)
    return I.VanHoveDistinct(samples=int(visits[0]), dropped=1, invalid=3, origin_floor=2, interval=interval, origin_every=every, r_max=r_max,
                             dr=r_max / hist.shape[2], classes=classes, num_sites=num_sites, pairs_per_sample=pps, head=head, hist=hist)


def test_views_against_their_formulas_and_g_equal_to_the_rdfs():
    I = _I()
    # two bins of width 1: shells 4 pi / 3 and 4 pi / 3 * 7; 10 and 20 sites, 4 samples in a volume of 100, rows 0 .. 2 with 4, 3, 0 visits
    hist = [[[30, 70], [12, 40], [0, 0]], [[10, 0], [4, 2], [0, 0]]]
    v = _hand_made(hist, [4, 3, 0], 100.0, 2.0, [(0, 1), (1, 1)], [10, 20])
    assert np.array_equal(v.lag_steps, [0, 10, 20]) and np.array_equal(v.visits, [4, 3, 0])
    assert np.array_equal(v.inv_volume_sum, [0.04, 0.03, 0.0])
    assert np.array_equal(v.edges, [0.0, 1.0, 2.0]) and np.array_equal(v.r, [0.5, 1.5]) and np.array_equal(v.edges2, RR.edges2(2.0, 2))
    shell = 4 * np.pi / 3 * np.array([1.0, 7.0])
    assert np.allclose(v.shell_volumes, shell, rtol=1e-15)
    G = v.G_d(0)
    assert G.shape == (3, 2)
    assert np.allclose(G[0], np.array([30, 70]) / (200 * shell * 0.04), rtol=1e-15) and np.allclose(G[1], np.array([12, 40]) / (200 * shell * 0.03), rtol=1e-15)
    assert np.all(np.isnan(G[2]))                                    # a row without a visit
    assert np.allclose(v.G_d(1)[1], np.array([4, 2]) / (20 * 19 * shell * 0.03), rtol=1e-15)
    n = v.coordination(0)
    assert np.allclose(n[0], [30 / 40, 100 / 40]) and np.allclose(n[1], [12 / 30, 52 / 30]) and np.all(np.isnan(n[2]))
    assert np.allclose(v.coordination(1)[0], [10 / 80, 10 / 80])     # ordered pairs: every pair is there for both its sites already
    # g(c) is Rdf.g on the same numbers, bit for bit: the cross class as it stands, the class of one group with half the counts (the
    # RDF counts an unordered pair once, P_c = N (N - 1) / 2)
    rdf = I.Rdf(samples=4, dropped=0, invalid=0, inv_volume_sum=0.04, interval=10, r_max=2.0, dr=1.0, classes=np.array([[0, 1], [1, 1]], dtype=np.int32),
                num_sites=np.array([10, 20]), pairs_per_sample=np.array([200, 190]), counts=np.array([[30, 70], [5, 0]], dtype=np.int64))
    assert np.array_equal(v.g(0), rdf.g()[0]) and np.array_equal(v.g(1), rdf.g()[1]) and np.array_equal(v.g(0), G[0])
    assert np.array_equal(v.coordination(1)[0], rdf.coordination()[1]) and np.array_equal(v.coordination(0)[0], rdf.coordination()[0])
    # an ideal gas: the expected count of every bin and row, as a table, gives 1
    nbins, r_max, na, nb, vol = 16, 1.2, 300, 500, 64.0
    e = np.sqrt(RR.edges2(r_max, nbins))
    visits = [7, 6, 5]
    ideal = np.array([na * nb * k / vol * 4 * np.pi / 3 * (e[1:] ** 3 - e[:-1] ** 3) for k in visits])
    gas = _hand_made([np.rint(ideal * 1e6).astype(np.int64)], visits, vol, r_max, [(0, 1)], [na, nb])
    assert np.allclose(gas.G_d(0) / 1e6, 1.0, rtol=1e-5, atol=0)


def test_from_words_splits_head_and_hist():
    I = _I()
    H = I.H
    lay, counts = H.VanHoveDistinctLayout(), H.VanHoveDistinctCounts(5, 1, 2, 3)
    lay.interval, lay.num_lags, lay.origin_every, lay.nbins, lay.num_groups, lay.num_classes, lay.num_rows = 10, 2, 1, 4, 2, 2, 3
    lay.head_words, lay.hist_words, lay.words, lay.r_max, lay.dr = 6, 24, 30, 1.0, 0.25
    lay.num_sites[0], lay.num_sites[1] = 3, 4
    lay.classes[0][0], lay.classes[0][1], lay.classes[1][0], lay.classes[1][1] = 0, 1, 1, 1
    lay.pairs_per_sample[0], lay.pairs_per_sample[1] = 12, 12
    words = np.arange(30, dtype=np.int64)
    v = I.vanhove_distinct_from_words(words, lay, counts)
    assert (v.samples, v.dropped, v.invalid, v.origin_floor, v.interval, v.origin_every) == (5, 1, 2, 3, 10, 1)
    assert np.array_equal(v.head, words[:6].reshape(3, 2)) and np.array_equal(v.hist, words[6:].reshape(2, 3, 4))
    assert np.array_equal(v.classes, [[0, 1], [1, 1]]) and list(v.num_sites) == [3, 4] and list(v.pairs_per_sample) == [12, 12]
    assert np.array_equal(v.visits, [0, 2, 4])


def test_write_vanhove_distinct_round_trips_through_loadtxt():
    hist = [[[30, 70, 11], [12, 40, 9], [0, 0, 0]], [[10, 0, 2], [4, 2, 1], [0, 0, 0]]]
    v = _hand_made(hist, [4, 3, 0], 100.0, 1.5, [(0, 1), (1, 1)], [10, 20])
    for c in (0, 1):
        out = io.StringIO()
        R.write_vanhove_distinct(out, v, 0.001, c=c)
        text = out.getvalue()
        head = text.splitlines()[:3]
        assert head[0] == '#"Samples"\t4\t"Dropped"\t1\t"Invalid"\t3\t"OriginFloor"\t2'
        assert head[1] == '#"Visits"\t4\t3\t0'
        tag = "0-1" if c == 0 else "1-1"
        assert head[2] == '#"r (nm)"\t"G_d[%s](0.0 ps)"\t"G_d[%s](0.01 ps)"\t"G_d[%s](0.02 ps)"' % (tag, tag, tag)
        back = np.loadtxt(io.StringIO(text))
        assert back.shape == (3, 4)
        assert np.array_equal(back[:, 0], v.r) and np.array_equal(back[:, 1:], v.G_d(c).T, equal_nan=True)
        plain = io.StringIO()
        R.write_vanhove_distinct(plain, v, 0.001, c=c, header=False)
        assert plain.getvalue() == "\n".join(text.splitlines()[3:]) + "\n"


# ------------------------------------------------------------------------------------------ the test hooks and the digest of the host tables
def test_hooks_are_known_and_checked():
    H = _I().H
    plan, keep = _plan()
    try:
        tune = lambda key, value: H.lib.vvhip_debug_tune(plan, key, value)
        for key, good, bad in ((b"vhd_hist_copies", (1, 4), (0, 2, 8)), (b"vhd_items_target", (1, 2, 4096), (0, -1)), (b"vhd_lds", (0, 1), (-1, 2))):
            for value in good:
                assert tune(key, value) == H.OK, (key, value)
            for value in bad:
                assert tune(key, value) == H.ERR_INVALID, (key, value)
    finally:
        H.lib.vvhip_plan_destroy(plan)


def test_recorder_digest_answers_for_vanhove_distinct():
    H = _I().H
    H.lib.vvhip_debug_recorder_digest.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64)]
    plan, keep = _plan(box=(3.0, 3.2, 3.4))
    try:
        def digest(name=b"vanhove_distinct"):
            out = C.c_uint64(1)
            assert H.lib.vvhip_debug_recorder_digest(plan, name, C.byref(out)) == H.OK
            return out.value

        assert digest() == 0                                         # nothing described
        _describe(plan)
        first = digest()
        assert first != 0 and digest(b"rdf") == 0 and digest(b"vanhove") == 0
        _describe(plan)
        assert digest() == first
        _describe(plan, num_groups=2, classes=[(0, 1)])
        assert digest() not in (0, first)                            # the work list is part of it
        assert H.lib.vvhip_debug_tune(plan, b"vhd_items_target", 1) == H.OK
        _describe(plan)
        assert digest() not in (0, first)                            # ... and follows the hook that shapes it
        assert H.lib.vvhip_vanhove_distinct_stop(plan) == H.OK and digest() == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)
