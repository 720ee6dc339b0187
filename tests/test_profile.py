"""Device-side profiles (include/vvhip.h: vvhip_profile_*), host side (no GPU): the NumPy statement of the arithmetic against a plain
Python loop, the fixed point and the default limits of an unbound plan, every refusal of the start in its documented order, the text
writer read back, and the sum over shards."""
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
import profile_reference as PR      # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S = pkg.systems
R = pkg.reporters

ENTRY_POINTS = ("vvhip_profile_start", "vvhip_profile_read", "vvhip_profile_stop", "vvhip_profile_info")


def _I():
    return importlib.import_module("openmm-velocityverlet_amd.integrator")


_SPEC = {}


def _spec():
    if "s" not in _SPEC:
        _SPEC["s"] = S.make_config("C3", scale=0.05)
    return _SPEC["s"]


def _plan(shard=None):
    I = _I()
    it = I.VVIntegrator(333.0, 10.0, 1.0, 40.0, 0.001)
    plan, _, keep = I.create_plan(_spec(), it, "mixed", shard)
    return plan, keep


def _describe(plan, interval=10, axis=2, nbins=64, mask=1, num_groups=1, group=None, max_samples=1000, limit=(0, 0, 0, 0)):
    """vvhip_profile_start on an unbound plan: (return code, error text); a description that passes the argument checks is kept."""
    H = _I().H
    grp = None if group is None else np.ascontiguousarray(group, dtype=np.int8)
    desc = H.ProfileDesc(interval, axis, nbins, mask, num_groups, 0, None if grp is None else grp.ctypes.data, max_samples, (C.c_double * 4)(*limit))
    rc = H.lib.vvhip_profile_start(plan, C.byref(desc))
    return rc, H.lib.vvhip_last_error(plan).decode()


def _info(plan):
    H = _I().H
    lay = H.ProfileLayout()
    assert H.lib.vvhip_profile_info(plan, C.byref(lay)) == H.OK
    return lay


def test_profile_entry_points_are_exported():
    H = _I().H
    for name in ENTRY_POINTS:
        assert name in H.EXPORTS, name
    assert C.sizeof(H.ProfileDesc) == 72 and C.sizeof(H.ProfileCounts) == 24 and C.sizeof(H.ProfileLayout) == 136
    assert (H.PROFILE_COUNT, H.PROFILE_CHARGE, H.PROFILE_MASS, H.PROFILE_MOMENTUM, H.PROFILE_KINETIC) == (1, 2, 4, 8, 16)


# ------------------------------------------------------------------------------------------ the reference against a plain loop
class _Desc:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _loop(x, v, q, m, g, box, desc, frac):
    """profile_reference, one particle and one Python float operation at a time."""
    row_of, rows = PR.rows_of_mask(desc.mask)
    table = np.zeros((desc.num_groups, rows, desc.nbins), dtype=np.int64)
    out = 0
    inv_l = 1.0 / float(box[desc.axis])
    for i in range(len(x)):
        if g[i] < 0:
            continue
        t = float(x[i][desc.axis]) * inv_l
        u = t - math.floor(t)
        b = min(int(u * float(desc.nbins)), desc.nbins - 1)
        mi, vx, vy, vz = float(m[i]), float(v[i][0]), float(v[i][1]), float(v[i][2])
        terms = []                                                  # (row, value, quantity)
        if desc.mask & PR.CHARGE:
            terms.append((row_of[1], float(q[i]), 1))
        if desc.mask & PR.MASS:
            terms.append((row_of[2], mi, 2))
        if desc.mask & PR.MOMENTUM:
            terms += [(row_of[3], mi * vx, 3), (row_of[3] + 1, mi * vy, 3), (row_of[3] + 2, mi * vz, 3)]
        if desc.mask & PR.KINETIC:
            terms.append((row_of[4], mi * ((vx * vx + vy * vy) + vz * vz), 4))
        if any(not (abs(value) < desc.limit[quantity]) for _, value, quantity in terms):
            out += 1
            continue
        table[g[i], 0, b] += 1
        for row, value, quantity in terms:
            table[g[i], row, b] += round(value * 2.0 ** frac[quantity])        # (Python's round: half to even)
    return table, out


@pytest.mark.parametrize("mask", [1, 3, 31, 8 | 16, 4 | 8])
@pytest.mark.parametrize("axis,nbins", [(2, 64), (0, 1), (1, 63), (2, 1000)])
def test_reference_equals_a_plain_loop(mask, axis, nbins):
    rng = np.random.default_rng(100 * mask + nbins)
    n = 200
    box = np.array([3.1, 2.7, 6.3])
    length = box[axis]
    x = rng.uniform(-2.0, 9.0, (n, 3))
    edges = np.arange(nbins + 1) * (length / nbins)
    k = min(40, nbins + 1)
    x[:k, axis] = edges[np.linspace(0, nbins, k).astype(int)]      # exactly on bin edges, 0 and L included
    x[40, axis] = -1e-20                                            # u = 1.0: the last bin by the clamp
    x[41, axis] = 400 * length + 0.37 * length                      # 400 box lengths out
    x[42, axis] = -0.5 * length
    x[43, axis] = np.nextafter(length, 0.0)
    x[44, axis] = -400 * length - 1e-9
    v = rng.normal(0.0, 0.6, (n, 3))
    q = rng.choice([-0.8, 0.8, 0.0, 1.5, -2.25], n)
    m = rng.choice([0.0, 0.4, 1.008, 12.011, 35.45, 126.9], n)
    g = rng.integers(-1, 3, n)
    v[50] = [np.nan, 0.0, 0.0]                                      # out of range where a velocity quantity is on
    v[51] = [40.0, 0.0, 0.0]
    v[52] = [0.0, 0.5, 1.5]                                         # m v = 0.25 and 0.75: ties of the coarse fixed point below, to even
    m[51], m[52] = 126.9, 0.5
    frac = [0, 20, 17, 1, 5]
    desc = _Desc(axis=axis, nbins=nbins, mask=mask, num_groups=3, limit=[1.0, 16.0, 128.0, 128.0 * 8, 128.0 * 64])
    want, want_out = _loop(x, v, q, m, g, box, desc, frac)
    got, got_out = PR.profile_reference(x, v, q, m, g, box, desc, frac)
    assert got.dtype == np.int64 and np.array_equal(got, want) and got_out == want_out
    assert got[:, 0].sum() == np.count_nonzero(g >= 0) - want_out
    if mask & (PR.MOMENTUM | PR.KINETIC):
        assert want_out >= (g[50] >= 0) + (g[51] >= 0)
    # the edge cases land where the definition says
    b = PR.bins(x[:, axis], length, nbins)
    assert b[40] == nbins - 1 and b[0] == 0                         # (-1e-20: u = 1.0, clamped; c = 0: bin 0)
    assert 0 <= b.min() and b.max() <= nbins - 1
    groups_none, _ = PR.profile_reference(x, v, q, m, None, box, _Desc(**{**desc.__dict__, "num_groups": 1}), frac)
    assert groups_none.shape[0] == 1


# ------------------------------------------------------------------------------------------ the fixed point of an unbound plan
def _ceil_log2(n):
    return max(0, (int(n) - 1).bit_length())


def _pow2_above(x):
    return 2.0 ** (math.frexp(x)[1])


def test_layout_without_a_recorder_is_empty():
    H = _I().H
    plan, _ = _plan()
    try:
        lay = _info(plan)
        assert (lay.active, lay.interval, lay.nbins, lay.rows, lay.words, lay.num_particles) == (0, 0, 0, 0, 0, 0)
        assert list(lay.row_of) == [-1] * 5
        assert H.lib.vvhip_profile_info(plan, None) == H.ERR_INVALID
        assert H.lib.vvhip_profile_stop(plan) == H.OK               # nothing to stop
    finally:
        H.lib.vvhip_plan_destroy(plan)


@pytest.mark.parametrize("mask,max_samples", [(1, 1000), (3, 1 << 20), (31, 30), (8 | 4, 4096), (16, 1)])
def test_fraction_bits_and_default_limits_of_an_unbound_plan(mask, max_samples):
    H = _I().H
    spec = _spec()
    n = spec.num_atoms
    masses = np.asarray(spec.masses, dtype=np.float64)
    plan, _ = _plan()
    try:
        rc, err = _describe(plan, interval=7, axis=1, nbins=100, mask=mask, num_groups=1, max_samples=max_samples)
        assert rc == H.ERR_INVALID and "vvhip_bind" in err         # an unbound plan cannot record, but answers for the layout
        lay = _info(plan)
        row_of, rows = PR.rows_of_mask(mask)
        assert (lay.active, lay.interval, lay.axis, lay.nbins, lay.mask, lay.num_groups) == (0, 7, 1, 100, mask | 1, 1)
        assert (lay.num_particles, lay.rows, lay.words, lay.max_samples, lay.start_step) == (n, rows, rows * 100, max_samples, 0)
        assert list(lay.row_of) == row_of
        mass_limit = _pow2_above(masses.max())
        assert mass_limit > masses.max() >= mass_limit / 2
        limits = [1.0, 16.0, mass_limit, mass_limit * 64, mass_limit * 4096]
        assert list(lay.limit) == limits
        head = 62 - _ceil_log2(n + 1) - _ceil_log2(max_samples + 1)
        assert lay.frac_bits[0] == 0
        for q in range(1, 5):
            assert lay.frac_bits[q] == min(40, head - int(math.log2(limits[q]))), (q, lay.frac_bits[q])
            if mask & (1 << q):
                # no word can overflow: n particles x max_samples samples x limit x 2^f stays below 2^63
                assert n * max_samples * limits[q] * 2.0 ** lay.frac_bits[q] <= 2.0 ** 62
        assert H.lib.vvhip_profile_stop(plan) == H.OK               # ... and forgets it
        assert _info(plan).words == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)


def test_given_limits_groups_and_shards():
    H = _I().H
    spec = _spec()
    n = spec.num_atoms
    masses = np.asarray(spec.masses, dtype=np.float64)
    mol = np.asarray(spec.mol_id)
    cut = int(np.nonzero(mol == mol[n // 2])[0].min())
    group = np.full(n, -1, dtype=np.int8)
    light = masses < np.median(masses[masses > 0])
    group[light] = 0
    group[::3] = 2                                                  # (group 1 stays empty)
    group[::7] = -1
    recorded = group >= 0
    for shard in (None, (0, cut), (cut, n)):
        plan, _ = _plan(shard)
        try:
            rc, err = _describe(plan, mask=31, num_groups=3, group=group, max_samples=100, limit=(3.0, 0, 1000.0, 8.0))
            assert rc == H.ERR_INVALID and "vvhip_bind" in err
            lay = _info(plan)
            lo, hi = shard or (0, n)
            assert lay.num_particles == np.count_nonzero(recorded[lo:hi]) and (lay.rows, lay.words) == (7, 3 * 7 * 64)
            # a given limit is rounded up to a power of two; the defaults follow the recorded particles of the WHOLE System, and so does
            # the fixed point: every shard scales its terms alike
            mass_limit = _pow2_above(masses[recorded].max())
            assert list(lay.limit) == [1.0, 4.0, mass_limit, 1024.0, 8.0]
            head = 62 - _ceil_log2(np.count_nonzero(recorded) + 1) - _ceil_log2(101)
            assert list(lay.frac_bits) == [0] + [min(40, head - int(math.log2(x))) for x in list(lay.limit)[1:]]
        finally:
            H.lib.vvhip_plan_destroy(plan)


# ------------------------------------------------------------------------------------------ refusals
# in the documented order: each case is wrong in its own argument AND in every argument behind it, and is refused for its own
ORDER = [("interval", dict(interval=0)), ("axis", dict(axis=3)), ("nbins", dict(nbins=0)), ("mask", dict(mask=32 | 1)),
         ("num_groups", dict(num_groups=17)), ("max_samples", dict(max_samples=0)), ("limit", dict(limit=(0, -1.0, 0, 0)))]


@pytest.mark.parametrize("k", range(len(ORDER)), ids=[name for name, _ in ORDER])
def test_profile_start_refuses_in_the_documented_order(k):
    H = _I().H
    plan, _ = _plan()
    try:
        kw = {}
        for _, bad in ORDER[k:]:
            kw.update(bad)
        rc, err = _describe(plan, **kw)
        assert rc == H.ERR_INVALID and err.startswith("profile: " + ORDER[k][0]), err
        assert "vvhip_bind" not in err
        assert _info(plan).words == 0                               # nothing is kept of it
    finally:
        H.lib.vvhip_plan_destroy(plan)


@pytest.mark.parametrize("kw,why", [
    (dict(interval=-3), "interval"), (dict(axis=-1), "axis"), (dict(nbins=65537), "nbins"), (dict(nbins=-1), "nbins"), (dict(mask=-1), "mask"),
    (dict(num_groups=0), "num_groups"), (dict(max_samples=-5), "max_samples"), (dict(limit=(float("nan"), 0, 0, 0)), "limit[0]"),
    (dict(limit=(0, 0, float("inf"), 0)), "limit[2]"), (dict(limit=(0, 0, 0, -2.0)), "limit[3]")])
def test_profile_start_validates_its_arguments(kw, why):
    H = _I().H
    plan, _ = _plan()
    try:
        rc, err = _describe(plan, **kw)
        assert rc == H.ERR_INVALID and err.startswith("profile: ") and why in err, err
        assert "vvhip_bind" not in err and _info(plan).words == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)


def test_group_entries_fraction_bits_and_the_unbound_plan():
    H = _I().H
    n = _spec().num_atoms
    plan, _ = _plan()
    try:
        group = np.zeros(n, dtype=np.int8)
        group[5] = 2
        rc, err = _describe(plan, num_groups=2, group=group)
        assert rc == H.ERR_INVALID and "group[5] = 2" in err and "num_groups" in err and "vvhip_bind" not in err
        group[5] = -2
        rc, err = _describe(plan, num_groups=2, group=group)
        assert rc == H.ERR_INVALID and "group[5] = -2" in err
        # behind the arguments: a quantity that would keep fewer than 8 fraction bits, named
        rc, err = _describe(plan, mask=1 | 16, max_samples=1 << 40)
        assert rc == H.ERR_INVALID and "kinetic" in err and "fraction bits" in err and "vvhip_bind" not in err
        rc, err = _describe(plan, mask=1 | 2 | 8, max_samples=1 << 20, limit=(0, 0, 2.0 ** 30, 0))
        assert rc == H.ERR_INVALID and "momentum" in err and "charge" not in err
        assert _info(plan).words == 0
        # the count alone has no fraction to lose
        rc, err = _describe(plan, mask=1, max_samples=1 << 40)
        assert rc == H.ERR_INVALID and "vvhip_bind" in err
        # the rest of the surface on an unbound plan
        counts = H.ProfileCounts()
        assert H.lib.vvhip_profile_read(plan, None, 0, C.byref(counts), 0) == H.ERR_INVALID
        assert H.lib.vvhip_profile_start(None, None) == H.ERR_INVALID
        assert H.lib.vvhip_profile_start(plan, None) == H.ERR_INVALID and "null description" in H.lib.vvhip_last_error(plan).decode()
        assert H.lib.vvhip_debug_recover(plan) == H.ERR_INVALID
    finally:
        H.lib.vvhip_plan_destroy(plan)


# ------------------------------------------------------------------------------------------ Profile, the writer, the sum over shards
def _fake_profile(rng, mask=31, groups=2, nbins=17, samples=12):
    I, H = _I(), _I().H
    row_of, rows = PR.rows_of_mask(mask)
    lay = H.ProfileLayout()
    lay.axis, lay.nbins, lay.mask, lay.num_groups, lay.rows, lay.words = 2, nbins, mask, groups, rows, groups * rows * nbins
    for q in range(5):
        lay.row_of[q], lay.frac_bits[q] = row_of[q], (0, 20, 17, 11, 5)[q]
    words = rng.integers(-10 ** 9, 10 ** 9, lay.words)
    words.reshape(groups, rows, nbins)[:, 0] = rng.integers(0, 50, (groups, nbins))
    if row_of[2] >= 0:
        m = words.reshape(groups, rows, nbins)[:, row_of[2]]
        m[:] = np.abs(m)
        m[0, 3] = 0                                                 # a bin without mass
    return I.profile_from_words(words, lay, H.ProfileCounts(samples, 1, 2), [3.0, 4.0, 8.5]), words.reshape(groups, rows, nbins)


def test_profile_views_and_densities():
    p, words = _fake_profile(np.random.default_rng(3))
    assert (p.samples, p.dropped, p.out_of_range) == (12, 1, 2) and p.words.dtype == np.int64 and np.array_equal(p.words, words)
    assert p.edges.shape == (18,) and p.edges[0] == 0.0 and p.edges[-1] == 8.5 and np.array_equal(p.centres, 0.5 * (p.edges[:-1] + p.edges[1:]))
    assert np.array_equal(p.count, words[:, 0].astype(np.float64))
    assert np.array_equal(p.charge, words[:, 1] * 2.0 ** -20) and np.array_equal(p.mass, words[:, 2] * 2.0 ** -17)
    assert p.momentum.shape == (2, 3, 17) and np.array_equal(p.momentum, words[:, 3:6] * 2.0 ** -11)
    assert np.array_equal(p.kinetic, words[:, 6] * 2.0 ** -5)
    vol = 3.0 * 4.0 * 8.5 / 17
    assert np.array_equal(p.number_density(), p.count / (vol * 12)) and np.array_equal(p.charge_density(), p.charge / (vol * 12))
    vel = p.velocity()
    assert vel.shape == (2, 3, 17) and np.all(vel[0, :, 3] == 0.0) and np.array_equal(vel[1], p.momentum[1] / p.mass[1][None, :])
    q, _ = _fake_profile(np.random.default_rng(4), mask=1)
    assert q.charge is None and q.momentum is None and q.words.shape == (2, 1, 17)
    with pytest.raises(ValueError):
        q.charge_density()
    with pytest.raises(ValueError):
        q.velocity()


@pytest.mark.parametrize("mask", [1, 3, 31, 1 | 4 | 8])
def test_write_profile_round_trips_through_loadtxt(tmp_path, mask):
    p, _ = _fake_profile(np.random.default_rng(5 + mask), mask=mask)
    path = str(tmp_path / "profile.txt")
    R.write_profile(path, p)
    lines = open(path).read().splitlines()
    assert lines[0] == '#"Samples"\t12\t"Dropped"\t1\t"OutOfRange"\t2' and lines[1].startswith('#"z (nm)"\t"count[0]"')
    a = np.loadtxt(path, delimiter="\t", ndmin=2)
    cols = R.profile_columns(p)
    assert a.shape == (17, len(cols)) and len(cols) == 1 + 2 * PR.rows_of_mask(mask)[1]
    assert lines[1].count("\t") == len(cols) - 1
    for j, (name, values) in enumerate(cols):
        assert np.array_equal(a[:, j], values), name               # repr round-trips the bits
    assert np.array_equal(a[:, 0], p.centres) and np.array_equal(a[:, 1], p.count[0])
    # appended without a header: a second block of the same shape; an open stream works too
    R.write_profile(path, p, append=True, header=False)
    assert np.array_equal(np.loadtxt(path, delimiter="\t", ndmin=2), np.concatenate([a, a]))
    s = io.StringIO()
    R.write_profile(s, p)
    assert s.getvalue().splitlines() == lines


def test_profile_sum_adds_the_words_as_integers():
    D = importlib.import_module("openmm-velocityverlet_amd.distributed")
    a, wa = _fake_profile(np.random.default_rng(8))
    b, wb = _fake_profile(np.random.default_rng(9))
    big = 2 ** 61 + 12345                                           # beyond float64's integers: the sum must not pass through floats
    a.words[1, 6, 2], b.words[1, 6, 2] = big, -big + 7
    t = D.profile_sum([a, b])
    assert t.words.dtype == np.int64 and np.array_equal(t.words, a.words + b.words) and t.words[1, 6, 2] == 7
    assert (t.samples, t.dropped, t.out_of_range) == (12, 1, 4)
    assert np.array_equal(t.count, (a.words + b.words)[:, 0].astype(np.float64)) and np.array_equal(t.charge, (a.words + b.words)[:, 1] * 2.0 ** -20)
    assert np.array_equal(D.profile_sum([a]).words, a.words)
    c, _ = _fake_profile(np.random.default_rng(10), samples=11)
    with pytest.raises(ValueError):
        D.profile_sum([a, c])
    d, _ = _fake_profile(np.random.default_rng(10), nbins=16)
    with pytest.raises(ValueError):
        D.profile_sum([a, d])
