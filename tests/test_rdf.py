"""Device-side radial distribution functions (include/vvhip.h: vvhip_rdf_*), the host half, no GPU: tests/rdf_reference.py against a
plain Python double loop, the edges, the symmetry of the histogram, the layout of an unbound plan, every refusal of the start in its
documented order, the struct sizes, Rdf.g() in closed form, the text writer read back."""
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
import rdf_reference as RR      # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S = pkg.systems
R = pkg.reporters

ENTRY_POINTS = ("vvhip_rdf_start", "vvhip_rdf_sample", "vvhip_rdf_read", "vvhip_rdf_stop", "vvhip_rdf_info")
# the (r_max, nbins) of tests/test_gpu_rdf.py (1.55 and 1.24: half the shortest edge of its boxes) and of tools/probes/rdf_cost.py
GPU_BINS = [(1.55, 1), (1.55, 8), (1.55, 64), (1.55, 8192), (1.24, 1), (1.24, 8192), (0.7, 64), (0.5, 4), (0.4, 1), (1.0, 8), (2.0, 64),
            (0.6, 32), (0.6, 64), (0.6, 128), (0.6, 300), (1.5, 300), (3.1, 300)]


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


def _describe(plan, interval=10, nbins=64, num_groups=1, classes=((0, 0),), exclude=0, group=None, max_samples=1000, r_max=0.5, num_classes=None,
              null_classes=False):
    """vvhip_rdf_start on an unbound plan: (return code, error text); a description that passes the checks in front of the bind is kept."""
    H = _I().H
    grp = None if group is None else np.ascontiguousarray(group, dtype=np.int8)
    cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1, 2)
    desc = H.RdfDesc(interval, nbins, num_groups, len(cls) if num_classes is None else num_classes, exclude, 0, None if grp is None else grp.ctypes.data,
                     None if null_classes else cls.ctypes.data, max_samples, r_max)
    rc = H.lib.vvhip_rdf_start(plan, C.byref(desc))
    return rc, H.lib.vvhip_last_error(plan).decode()


def _info(plan):
    H = _I().H
    lay = H.RdfLayout()
    assert H.lib.vvhip_rdf_info(plan, C.byref(lay)) == H.OK
    return lay


def test_rdf_entry_points_and_struct_sizes():
    H = _I().H
    for name in ENTRY_POINTS:
        assert name in H.EXPORTS and hasattr(H.lib, name)
    header = open(os.path.join(ROOT, "include", "vvhip.h")).read()
    for name in ENTRY_POINTS:
        assert "int %s(" % name in header
    assert C.sizeof(H.RdfDesc) == 56 and C.sizeof(H.RdfCounts) == 32 and C.sizeof(H.RdfLayout) == 656


# ------------------------------------------------------------------------------------------ the reference against a plain loop
def _loop(x, box, groups, classes, r_max, nbins, mol_id):
    """The statement, one scalar at a time (Python floats are float64; round() is round-half-even)."""
    dr = r_max / nbins
    e = [(k * dr) * (k * dr) for k in range(nbins + 1)]
    table, invalid = np.zeros((len(classes), nbins), dtype=np.int64), 0
    n = len(x)
    for c, (ga, gb) in enumerate(classes):
        for i in range(n):
            if groups[i] != ga:
                continue
            for j in range(n):
                if groups[j] != gb or (ga == gb and not i < j) or (mol_id is not None and mol_id[i] == mol_id[j]):
                    continue
                d = []
                for a in range(3):
                    t = x[i][a] - x[j][a]
                    q = t * (1.0 / box[a])
                    if math.isnan(q):
                        d.append(float("nan"))
                        continue
                    t = t - box[a] * float(round(q))
                    d.append(t)
                r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                if math.isnan(r2):
                    invalid += 1
                    continue
                for b in range(nbins):
                    if e[b] <= r2 < e[b + 1]:
                        table[c, b] += 1
    return table, invalid


@pytest.mark.parametrize("exclude", [False, True], ids=["all-pairs", "exclude-same-molecule"])
@pytest.mark.parametrize("r_max,nbins", [(1.0, 8), (0.9, 5), (1.25, 1)])
def test_reference_equals_a_plain_loop(exclude, r_max, nbins):
    rng = np.random.default_rng(11)
    n = 40
    box = np.array([2.5, 3.0, 2.75])
    x = rng.uniform(-4.0, 7.0, size=(n, 3))                          # unwrapped: several images
    x[5] = x[4] + np.array([0.25, 0.0, 0.0])                         # a pair exactly on an edge of (1.0, 8)
    x[9] = x[8]                                                      # distance 0
    x[17, 1] = np.nan
    groups = rng.integers(-1, 3, size=n).astype(np.int8)
    groups[[4, 5, 8, 9]] = [0, 1, 0, 0]
    mol_id = np.sort(rng.integers(0, 12, size=n))
    classes = [(0, 1), (0, 0), (2, 2), (1, 0)]
    table, invalid = RR.rdf_reference(x, box, groups, classes, r_max, nbins, mol_id if exclude else None)
    want, want_invalid = _loop(x.tolist(), box.tolist(), groups.tolist(), classes, r_max, nbins, mol_id.tolist() if exclude else None)
    assert invalid == want_invalid and np.array_equal(table, want) and table.sum() > 0
    if not exclude:
        assert invalid > 0
    assert np.array_equal(table[0], table[3])                        # (a, b) and (b, a): the same histogram


@pytest.mark.parametrize("r_max,nbins", GPU_BINS)
def test_edges_strictly_increase(r_max, nbins):
    e = RR.edges2(r_max, nbins)
    assert e[0] == 0.0 and e.shape == (nbins + 1,) and np.all(np.diff(e) > 0)
    assert np.array_equal(e, _I().rdf_edges(r_max, nbins))


@pytest.mark.parametrize("cfg,scale", [("C1", 1.0), ("C3", 0.1), ("C5", 0.25)])
def test_edges_strictly_increase_at_half_the_box_of_the_gpu_tests(cfg, scale):
    half = float(min(S.make_config(cfg, scale=scale).box)) / 2
    for nbins in (1, 8, 64, 8192):
        e = RR.edges2(half, nbins)
        assert e[0] == 0.0 and np.all(np.diff(e) > 0)


def test_histogram_is_symmetric_bit_for_bit():
    rng = np.random.default_rng(3)
    box = np.array([3.1, 2.9, 3.3])
    a, b = rng.uniform(-10, 10, size=(301, 3)), rng.uniform(-10, 10, size=(257, 3))
    for r_max, nbins in [(1.45, 64), (1.45, 8192), (0.3, 7)]:
        hab, _ = RR.histogram(a, b, box, r_max, nbins)
        hba, _ = RR.histogram(b, a, box, r_max, nbins)
        assert np.array_equal(hab, hba) and hab.sum() > 0
    # ... because r2 itself is: the arithmetic is odd in d
    assert np.array_equal(RR.r2_block(a, b, box), RR.r2_block(b, a, box).T)


# ------------------------------------------------------------------------------------------ the layout of an unbound plan
def test_layout_of_an_unbound_plan():
    H = _I().H
    spec = _spec()
    n = spec.num_atoms
    plan, keep = _plan(box=(3.0, 3.2, 3.4))
    try:
        lay = _info(plan)
        assert (lay.active, lay.words, lay.nbins) == (0, 0, 0)
        groups = (np.arange(n) % 3).astype(np.int8) - 1               # -1, 0, 1
        classes = [(0, 1), (0, 0), (1, 1)]
        rc, text = _describe(plan, interval=7, nbins=300, num_groups=2, classes=classes, group=groups, r_max=1.5, exclude=1, max_samples=123)
        assert rc == H.ERR_INVALID and "vvhip_bind has not been called" in text
        lay = _info(plan)
        n0, n1 = int(np.count_nonzero(groups == 0)), int(np.count_nonzero(groups == 1))
        assert (lay.active, lay.interval, lay.nbins, lay.num_groups, lay.num_classes, lay.exclude_same_molecule, lay.max_samples) == (0, 7, 300, 2, 3, 1, 123)
        assert list(lay.num_sites[:3]) == [n0, n1, 0]
        assert [tuple(lay.classes[c]) for c in range(3)] == classes
        assert list(lay.pairs_per_sample[:4]) == [n0 * n1, n0 * (n0 - 1) // 2, n1 * (n1 - 1) // 2, 0]
        assert list(lay.pairs_per_sample[:3]) == list(RR.pairs_per_sample(groups, classes))
        assert lay.dr == 1.5 / 300 and lay.r_max == 1.5 and lay.words == 3 * 300
        stride = (n0 + n1 + 15) // 16 * 16
        assert lay.scratch_bytes == 3 * stride * 8 and lay.tile >= 64 and lay.tile % 64 == 0
        # a small workload: per i-tile the j-sites in runs of 64, a class of one group with itself from the i-tile's first site on
        runs = lambda na, nb, same: sum(-(-(nb - (i0 if same else 0)) // 64) for i0 in range(0, na, lay.tile))
        assert lay.num_items == runs(n0, n1, False) + runs(n0, n0, True) + runs(n1, n1, True)
        assert H.lib.vvhip_rdf_stop(plan) == H.OK and _info(plan).words == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)


def test_start_refuses_in_the_documented_order():
    H = _I().H
    n = _spec().num_atoms
    plan, keep = _plan(box=(2.0, 2.0, 2.0))
    try:
        assert H.lib.vvhip_rdf_start(plan, None) == H.ERR_INVALID and "null description" in H.lib.vvhip_last_error(plan).decode()
        bad_group = np.zeros(n, dtype=np.int8)
        bad_group[3] = 2
        # every description carries all the later faults too: the first one in the documented order is the one reported
        later = dict(r_max=-1.0, nbins=0, num_groups=17, num_classes=33, null_classes=True, max_samples=0)
        order = [("interval", dict(interval=0), "interval must be >= 1"),
                 ("r_max", dict(r_max=float("inf")), "r_max must be finite and > 0"),
                 ("nbins", dict(nbins=8193), "nbins must be in [1, 8192]"),
                 ("num_groups", dict(num_groups=0), "num_groups must be in [1, 16]"),
                 ("num_classes", dict(num_classes=0), "num_classes must be in [1, 32]"),
                 ("classes", dict(null_classes=True), "classes must not be NULL"),
                 ("max_samples", dict(max_samples=0), "max_samples must be >= 1")]
        names = [k for k, _, _ in order]
        for pos, (name, fault, text) in enumerate(order):
            kw = {k: v for k, v in later.items() if k in names[pos + 1:] or (k == "null_classes" and "classes" in names[pos + 1:])}
            kw.update(fault)
            rc, err = _describe(plan, **kw)
            assert rc == H.ERR_INVALID and text in err, (name, err)
        assert _describe(plan, r_max=0.0)[1].count("r_max must be finite and > 0") == 1
        assert _describe(plan, r_max=float("nan"))[0] == H.ERR_INVALID
        # a group entry, then a class entry, then the overflow, then the box, then the shard, then the bind
        rc, err = _describe(plan, num_groups=2, group=bad_group, classes=[(0, 5)], max_samples=1 << 62, r_max=1.5)
        assert rc == H.ERR_INVALID and "group[3] = 2 is outside [-1, num_groups = 2)" in err
        rc, err = _describe(plan, num_groups=2, classes=[(0, 1), (0, 5)], max_samples=1 << 62, r_max=1.5)
        assert rc == H.ERR_INVALID and "classes[1][1] = 5 is outside [0, num_groups = 2)" in err
        rc, err = _describe(plan, max_samples=1 << 62, r_max=1.5)
        assert rc == H.ERR_INVALID and "reaches 2^62" in err
        pairs = n * (n - 1) // 2
        assert _describe(plan, max_samples=(1 << 62) // pairs + 1, r_max=1.5)[1].count("reaches 2^62") == 1
        rc, err = _describe(plan, max_samples=((1 << 62) - 1) // pairs, r_max=1.5)
        assert rc == H.ERR_INVALID and "above half the shortest edge of the box" in err
        assert _info(plan).words == 0                                # nothing of a refused description is kept
        rc, err = _describe(plan, r_max=1.0)                         # exactly min(L) / 2 passes
        assert rc == H.ERR_INVALID and "vvhip_bind has not been called" in err and _info(plan).words == 64
        assert H.lib.vvhip_rdf_sample(plan) == H.ERR_INVALID and H.lib.vvhip_rdf_read(plan, None, 0, None, 0) == H.ERR_INVALID
    finally:
        H.lib.vvhip_plan_destroy(plan)
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


# ------------------------------------------------------------------------------------------ g(r), the coordination number, the writer
def _hand_made(counts, r_max, classes, num_sites, samples, inv_volume_sum):
    I = _I()
    counts = np.asarray(counts, dtype=np.int64)
    classes = np.asarray(classes, dtype=np.int32).reshape(-1, 2)
    num_sites = np.asarray(num_sites, dtype=np.int64)
    pps = np.array([num_sites[a] * (num_sites[a] - 1) // 2 if a == b else num_sites[a] * num_sites[b] for a, b in classes], dtype=np.int64)
    return I.Rdf(samples=samples, dropped=0, invalid=0, inv_volume_sum=inv_volume_sum, interval=1, r_max=r_max, dr=r_max / counts.shape[1],
                 classes=classes, num_sites=num_sites, pairs_per_sample=pps, counts=counts)


def test_g_in_closed_form():
    # two bins of width 1: shells 4 pi / 3 and 4 pi / 3 * 7; 10 x 20 sites, 4 samples in a volume of 100
    rdf = _hand_made([[30, 70], [5, 0]], 2.0, [(0, 1), (1, 1)], [10, 20], 4, 4 / 100.0)
    assert np.array_equal(rdf.edges, [0.0, 1.0, 2.0]) and np.array_equal(rdf.r, [0.5, 1.5])
    g = rdf.g()
    shell = 4 * np.pi / 3 * np.array([1.0, 7.0])
    assert np.allclose(g[0], np.array([30, 70]) / (200 * shell * 0.04), rtol=1e-15)
    assert np.allclose(g[1], np.array([5, 0]) / (190 * shell * 0.04), rtol=1e-15)
    n = rdf.coordination()
    assert np.allclose(n[0], [30 / 40, 100 / 40]) and np.allclose(n[1], [2 * 5 / 80, 2 * 5 / 80])
    # an ideal gas: the expected count of every bin, as a table, gives exactly 1
    nbins, r_max, na, nb, samples, vol = 16, 1.2, 300, 500, 7, 64.0
    e = np.sqrt(RR.edges2(r_max, nbins))
    ideal = na * nb * samples / vol * 4 * np.pi / 3 * (e[1:] ** 3 - e[:-1] ** 3)
    scale = 1e6                                                      # (integers: scale the pair density up until rounding is below 1e-6)
    rdf = _hand_made([np.rint(ideal * scale).astype(np.int64)], r_max, [(0, 1)], [na, nb], samples, samples / vol)
    assert np.allclose(rdf.g()[0] / scale, 1.0, rtol=1e-5, atol=0)
    empty = _hand_made([[0, 0]], 2.0, [(0, 0)], [1], 0, 0.0)
    assert np.all(np.isnan(empty.g())) and np.all(np.isnan(empty.coordination()))


def test_write_rdf_round_trips():
    rdf = _hand_made([[30, 70, 11], [5, 0, 2]], 1.5, [(0, 1), (1, 1)], [10, 20], 4, 4 / 100.0)
    out = io.StringIO()
    R.write_rdf(out, rdf)
    text = out.getvalue()
    assert text.startswith('#"Samples"\t4\t"Dropped"\t0\t"Invalid"\t0\t"InvVolumeSum"\t0.04\n#"r (nm)"\t"count[0-1]"\t"g[0-1]"\t"n[0-1]"\t"count[1-1]"')
    back = np.loadtxt(io.StringIO(text))
    assert back.shape == (3, 7)
    g, n = rdf.g(), rdf.coordination()
    assert np.array_equal(back[:, 0], rdf.r) and np.array_equal(back[:, 1], rdf.counts[0]) and np.array_equal(back[:, 4], rdf.counts[1])
    assert np.array_equal(back[:, 2], g[0]) and np.array_equal(back[:, 5], g[1]) and np.array_equal(back[:, 3], n[0]) and np.array_equal(back[:, 6], n[1])
