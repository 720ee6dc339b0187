"""Device-side mean-squared displacements (include/vvhip.h: vvhip_msd_*), the host half, no GPU: tests/msd_reference.py against a plain
Python loop, uniform motion in closed form, the pair count per lag against its closed form, the layout, fixed point and default limit of an
unbound plan (sharded and whole), every refusal of the start in its documented order, the struct sizes, the text writer read back,
distributed.msd_sum."""
import ctypes as C
import importlib
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msd_reference as MR      # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S = pkg.systems
R = pkg.reporters

ENTRY_POINTS = ("vvhip_msd_start", "vvhip_msd_read", "vvhip_msd_stop", "vvhip_msd_info")


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


def _describe(plan, interval=10, num_lags=8, origin_every=1, mode=0, num_groups=1, group=None, max_samples=1000, limit=0.0):
    """vvhip_msd_start on an unbound plan: (return code, error text); a description that passes the checks in front of the bind is kept."""
    H = _I().H
    grp = None if group is None else np.ascontiguousarray(group, dtype=np.int8)
    desc = H.MsdDesc(interval, num_lags, origin_every, mode, num_groups, 0, None if grp is None else grp.ctypes.data, max_samples, limit)
    rc = H.lib.vvhip_msd_start(plan, C.byref(desc))
    return rc, H.lib.vvhip_last_error(plan).decode()


def _info(plan):
    H = _I().H
    lay = H.MsdLayout()
    assert H.lib.vvhip_msd_info(plan, C.byref(lay)) == H.OK
    return lay


def test_msd_entry_points_and_struct_sizes():
    H = _I().H
    for name in ENTRY_POINTS:
        assert name in H.EXPORTS and hasattr(H.lib, name)
    header = open(os.path.join(ROOT, "include", "vvhip.h")).read()
    for name in ENTRY_POINTS:
        assert "int %s(" % name in header
    assert C.sizeof(H.MsdDesc) == 48 and C.sizeof(H.MsdCounts) == 32 and C.sizeof(H.MsdLayout) == 80


# ------------------------------------------------------------------------------------------ the reference against a plain loop
def _loop(x, masses, mol_id, groups, molecules, num_groups, num_lags, every, frac, limit, floor):
    """The statement, one scalar at a time.  x: [J][n][3] nested floats."""
    n = len(x[0])
    units = []                                                       # (group, members)
    if molecules:
        for m in sorted(set(mol_id)):
            mem = [i for i in range(n) if mol_id[i] == m and masses[i] > 0]
            if mem and (groups is None or groups[mem[0]] >= 0):
                units.append((0 if groups is None else groups[mem[0]], mem))
    else:
        units = [(0 if groups is None else groups[i], [i]) for i in range(n) if groups is None or groups[i] >= 0]

    def centre(frame, mem):
        if not molecules:
            return [float(frame[mem[0]][a]) for a in range(3)]
        s, total = [0.0, 0.0, 0.0], 0.0
        for i in mem:
            for a in range(3):
                s[a] = s[a] + masses[i] * float(frame[i][a])
            total = total + masses[i]
        return [s[a] / total for a in range(3)]

    table, out = np.zeros((num_groups, num_lags, 4), dtype=np.int64), 0
    c = [[centre(frame, mem) for _, mem in units] for frame in x]
    for j in range(len(x)):
        for o in range(j):
            if o % every or o < floor or j - o > num_lags:
                continue
            for u, (g, _) in enumerate(units):
                d = [c[j][u][a] - c[o][u][a] for a in range(3)]
                if not all(abs(v) < limit for v in d):
                    out += 1
                    continue
                table[g, j - o - 1, 0] += 1
                for a in range(3):
                    table[g, j - o - 1, 1 + a] += int(np.rint(d[a] * d[a] * 2.0 ** frac))
    return table, out


@pytest.mark.parametrize("molecules", [False, True], ids=["particles", "molecules"])
@pytest.mark.parametrize("num_lags,every,floor", [(5, 1, 0), (5, 2, 0), (6, 3, 4), (4, 4, 0)])
def test_reference_equals_a_plain_loop(molecules, num_lags, every, floor):
    rng = np.random.default_rng(5)
    n, J = 23, 11
    mol_id = np.sort(rng.integers(0, 7, size=n))
    masses = rng.uniform(1.0, 30.0, size=n)
    masses[rng.choice(n, size=4, replace=False)] = 0.0               # massless particles take no part in a centre of mass
    per_mol = rng.integers(-1, 2, size=7)
    groups = per_mol[mol_id].astype(np.int8)
    x = np.cumsum(rng.normal(0, 0.3, size=(J, n, 3)), axis=0)
    x[7, 5, 1] = np.nan
    limit, frac = 1.0, 30
    c = [MR.unit_positions(f, masses, mol_id, groups, molecules) for f in x]
    table, out = MR.msd_reference(np.array([p for p, _ in c]), c[0][1], 2, num_lags, every, frac, limit, floor)
    want, want_out = _loop(x.tolist(), masses.tolist(), mol_id.tolist(), groups.tolist(), molecules, 2, num_lags, every, frac, limit, floor)
    assert out == want_out > 0 and np.array_equal(table, want) and table[:, :, 0].sum() > 0


def test_mixed_groups_inside_a_molecule_are_refused_by_the_reference():
    with pytest.raises(ValueError):
        MR.molecule_units([1.0, 1.0], [0, 0], [0, 1])
    assert [(m, g, list(mem)) for m, g, mem in MR.molecule_units([1.0, 0.0, 2.0], [0, 0, 1], [1, -1, 0])] == [(0, 1, [0]), (1, 0, [2])]


# ------------------------------------------------------------------------------------------ uniform motion and the pair count
@pytest.mark.parametrize("num_lags,every", [(8, 1), (8, 3), (8, 8), (6, 2)])
def test_uniform_motion_in_closed_form(num_lags, every):
    """x = x0 + v t with v tau dyadic: every displacement is exact in float64, so a row's words are pairs * rint(|v_a tau|^2 2^F)."""
    rng = np.random.default_rng(2)
    U, J, frac = 13, 25, 24
    v = np.array([3.0, -5.0, 0.5]) * 2.0 ** -6
    x0 = rng.integers(-2 ** 20, 2 ** 20, size=(U, 3)).astype(np.float64) * 2.0 ** -12      # on the same dyadic grid: every sum is exact
    c = x0[None] + np.arange(J)[:, None, None] * v[None, None, :]
    table, out = MR.msd_reference(c, np.zeros(U, dtype=int), 1, num_lags, every, frac, 64.0)
    per_unit = MR.pair_counts(J, every, num_lags)
    assert out == 0 and np.array_equal(table[0, :, 0], U * per_unit)
    for l in range(num_lags):
        for a in range(3):
            assert table[0, l, 1 + a] == U * per_unit[l] * int(np.rint((v[a] * (l + 1)) ** 2 * 2.0 ** frac))


@pytest.mark.parametrize("num_lags,every", [(8, 1), (8, 2), (8, 8), (8, 3), (7, 5), (1, 1)])
@pytest.mark.parametrize("J", [0, 1, 2, 9, 30])
def test_pair_count_per_lag_in_closed_form(num_lags, every, J):
    """(8, 2), (8, 8): num_origins * E == num_lags -- the slot that is overwritten is read in the same sample; (8, 3), (7, 5): E does not
    divide num_lags."""
    got = np.zeros(num_lags, dtype=np.int64)
    for _, o, row in MR.pairs(J, every, num_lags):
        assert o % every == 0
        got[row] += 1
    assert np.array_equal(got, MR.pair_counts(J, every, num_lags))
    # the ring holds what the pairs need: the origin of a pair is the newest holder of its slot
    R_ = MR.num_origins(num_lags, every)
    for j, o, _ in MR.pairs(J, every, num_lags):
        newer = [k for k in range(o // every + 1, (j - 1) // every + 1) if k % R_ == (o // every) % R_]
        assert not newer


# ------------------------------------------------------------------------------------------ the layout of an unbound plan
def test_layout_without_a_recorder_is_empty():
    H = _I().H
    plan, keep = _plan()
    try:
        lay = _info(plan)
        assert (lay.active, lay.words, lay.num_units, lay.ring_bytes) == (0, 0, 0, 0)
        assert H.lib.vvhip_msd_stop(plan) == H.OK
    finally:
        H.lib.vvhip_plan_destroy(plan)


@pytest.mark.parametrize("mode", [0, 1], ids=["particles", "molecules"])
@pytest.mark.parametrize("max_samples,every,limit", [(1000, 1, 0.0), (1 << 20, 4, 0.0), (4000, 3, 2.0 ** -10), (4000, 3, 3.0)])
def test_layout_fraction_bits_and_limit_of_an_unbound_plan(mode, max_samples, every, limit):
    H = _I().H
    spec = _spec()
    n = spec.num_atoms
    masses, mol = np.asarray(spec.masses, dtype=np.float64), np.asarray(spec.mol_id)
    units_whole = len(MR.molecule_units(masses, mol)) if mode else n
    cut = int(np.nonzero(mol == mol[n // 2])[0].min())              # a molecule boundary
    for shard in (None, (0, cut), (cut, n)):
        plan, keep = _plan(shard)
        try:
            rc, err = _describe(plan, 10, 8, every, mode, 1, None, max_samples, limit)
            assert rc == H.ERR_INVALID and "vvhip_bind" in err      # an unbound plan cannot record, but answers for the layout
            lay = _info(plan)
            b, e = shard or (0, n)
            units_here = len([1 for _, _, mem in MR.molecule_units(masses, mol) if b <= mem[0] < e]) if mode else e - b
            assert (lay.active, lay.interval, lay.num_lags, lay.origin_every, lay.mode, lay.num_groups) == (0, 10, 8, every, mode, 1)
            assert lay.num_units == units_here and lay.num_origins == MR.num_origins(8, every) and lay.words == 8 * 4
            assert lay.limit == MR.applied_limit(limit) and lay.max_samples == max_samples
            assert lay.frac_bits == MR.frac_bits(units_whole, max_samples, every, limit)      # of the WHOLE System on every shard
            assert lay.ring_bytes == lay.num_origins * 3 * ((units_here + 15) // 16 * 16) * 8
        finally:
            H.lib.vvhip_plan_destroy(plan)
    assert MR.applied_limit(0.0) == 64.0 and MR.applied_limit(3.0) == 4.0 and MR.applied_limit(2.0 ** -10) == 2.0 ** -10
    assert MR.frac_bits(1000, 1000, 1, 0.0) == 62 - 10 - 10 - 12


# ------------------------------------------------------------------------------------------ the refusals, in their order
def test_msd_start_refuses_in_the_documented_order():
    """Everything wrong at once, then one thing put right at a time: the error names the next one."""
    import barostat_cases as K
    I = _I()
    H = I.H
    spec = K.synthetic()                                             # (molecules whose particles alternate in index, massless ones among them)
    n = spec.num_atoms
    mol, masses = np.asarray(spec.mol_id), np.asarray(spec.masses)
    mixed = (np.arange(n) // 4 % 2).astype(np.int8)
    assert mol[1] == mol[5] and masses[1] > 0 and masses[5] > 0 and mixed[1] != mixed[5]      # one molecule, two groups
    assert mol[2] == mol[6] and masses[2] > 0 and masses[6] > 0                                 # the shard (0, 3) holds one of the two
    bad_entry = mixed.copy()
    bad_entry[3] = 5
    it = I.VVIntegrator(300.0, 10.0, 1.0, 40.0, 0.001)
    it.setUseCOMTempGroup(False)
    plan, _, keep = I.create_plan(spec, it, "mixed", (0, 3))        # a shard that cuts a molecule
    try:
        kw = dict(interval=0, num_lags=5000, origin_every=0, mode=7, num_groups=17, group=bad_entry, max_samples=0, limit=-1.0)
        steps = [("interval", dict(interval=10)), ("num_lags", dict(num_lags=4096)), ("origin_every", dict(origin_every=1)), ("mode", dict(mode=1)),
                 ("num_groups", dict(num_groups=2)), ("max_samples", dict(max_samples=1 << 61)), ("limit", dict(limit=0.0)),
                 ("group[3]", dict(group=mixed)), ("different groups", dict(group=None)), ("fraction bits", dict(max_samples=1000)),
                 ("num_origins", dict(origin_every=4)), ("cuts a molecule", None)]
        for text, fix in steps:
            rc, err = _describe(plan, **kw)
            assert rc == (H.ERR_UNSUPPORTED if fix is None else H.ERR_INVALID) and text in err, (text, rc, err)
            assert _info(plan).words == 0                            # nothing of a refused description is kept
            if fix:
                kw.update(fix)
        # particle mode does not mind the cut; the unbound plan is the next refusal, and keeps the description
        kw.update(mode=0)
        rc, err = _describe(plan, **kw)
        assert rc == H.ERR_INVALID and "vvhip_bind" in err
        assert _info(plan).words == 2 * 4096 * 4 and _info(plan).num_origins == 1024 and _info(plan).active == 0
        # the rest of the surface on an unbound plan
        assert H.lib.vvhip_msd_read(plan, None, 0, None, 0) == H.ERR_INVALID
        assert H.lib.vvhip_msd_start(plan, None) == H.ERR_INVALID and "null description" in H.lib.vvhip_last_error(plan).decode()
        assert H.lib.vvhip_msd_stop(plan) == H.OK and _info(plan).words == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)


# ------------------------------------------------------------------------------------------ the Python views, the writer, the sum
def _fake(rng, groups=2, lags=9, frac=30, interval=10, empty_last=True):
    I = _I()
    words = np.zeros((groups, lags, 4), dtype=np.int64)
    words[:, :, 0] = rng.integers(1, 500, size=(groups, lags))
    words[:, :, 1:] = rng.integers(0, 2 ** 45, size=(groups, lags, 3))
    if empty_last:
        words[:, -1, :] = 0
    return I.Msd(samples=40, dropped=1, out_of_range=3, origin_floor=2, interval=interval, origin_every=2, frac_bits=frac, molecules=False, words=words)


def test_msd_views_and_the_diffusion_coefficient():
    rng = np.random.default_rng(3)
    m = _fake(rng)
    assert np.array_equal(m.lag_steps, np.arange(1, 10) * 10) and np.array_equal(m.pairs, m.words[:, :, 0])
    assert m.msd.shape == (2, 9, 3) and np.all(np.isnan(m.msd[:, -1])) and np.all(np.isnan(m.total[:, -1]))
    assert np.array_equal(m.msd[:, :-1], m.words[:, :-1, 1:] * 2.0 ** -30 / m.words[:, :-1, :1])
    assert np.array_equal(m.total[:, :-1], m.msd[:, :-1].sum(axis=2))
    # straight lines: <dx_a^2> = 2 D_a t
    I = _I()
    dt, d_axis = 0.002, np.array([[0.5, 1.0, 1.5], [2.0, 2.0, 8.0]])
    words = np.zeros((2, 6, 4), dtype=np.int64)
    words[:, :, 0] = 1 << 4
    t = np.arange(1, 7) * 10 * dt
    words[:, :, 1:] = np.rint(2 * d_axis[:, None, :] * t[None, :, None] * 2.0 ** 34).astype(np.int64)
    line = I.Msd(samples=7, dropped=0, out_of_range=0, origin_floor=0, interval=10, origin_every=1, frac_bits=30, molecules=True, words=words)
    assert np.allclose(line.diffusion(dt, 0, 5), d_axis.mean(axis=1), rtol=1e-9, atol=0)
    assert np.allclose(line.diffusion(dt, 1, 4, axes=(2,)), d_axis[:, 2], rtol=1e-9, atol=0)
    assert np.allclose(line.diffusion(dt, 0, 5, axes=(0, 1)), d_axis[:, :2].mean(axis=1), rtol=1e-9, atol=0)
    with pytest.raises(ValueError):
        line.diffusion(dt, 2, 2)


def test_write_msd_round_trips_through_loadtxt():
    m = _fake(np.random.default_rng(4))
    out = io.StringIO()
    R.write_msd(out, m, 0.001)
    text = out.getvalue()
    head = text.splitlines()[:2]
    assert head[0] == '#"Samples"\t40\t"Dropped"\t1\t"OutOfRange"\t3\t"OriginFloor"\t2'
    assert head[1].startswith('#"lag (ps)"\t"pairs[0]"\t"msd[0] (nm^2)"\t"msd_x[0] (nm^2)"') and head[1].count("\t") == 10
    back = np.loadtxt(io.StringIO(text))
    assert back.shape == (9, 11)
    assert np.array_equal(back[:, 0], m.lag_steps * 0.001)
    for g in range(2):
        assert np.array_equal(back[:, 1 + 5 * g], m.pairs[g].astype(np.float64))
        assert np.array_equal(back[:, 2 + 5 * g], m.total[g], equal_nan=True)
        assert np.array_equal(back[:, 3 + 5 * g: 6 + 5 * g], m.msd[g], equal_nan=True)
    plain = io.StringIO()
    R.write_msd(plain, m, 0.001, header=False)
    assert plain.getvalue() == "\n".join(text.splitlines()[2:]) + "\n"


def test_msd_sum_adds_the_words_as_integers():
    import dataclasses
    D = pkg.distributed
    rng = np.random.default_rng(6)
    a, b = _fake(rng, empty_last=False), _fake(rng, empty_last=False)
    a.words[0, 0, 1] = 2 ** 62 - 5                                   # beyond float64's integers: the sum is an integer sum
    b.words[0, 0, 1] = 3
    s = D.msd_sum([a, b])
    assert s.words.dtype == np.int64 and np.array_equal(s.words, a.words + b.words) and s.words[0, 0, 1] == 2 ** 62 - 2
    assert (s.samples, s.dropped, s.out_of_range, s.origin_floor) == (40, 1, 6, 2)
    for other in (dataclasses.replace(b, frac_bits=29), dataclasses.replace(b, samples=39), dataclasses.replace(b, words=b.words[:, :-1]),
                  dataclasses.replace(b, origin_every=1), dataclasses.replace(b, molecules=True)):
        with pytest.raises(ValueError):
            D.msd_sum([a, other])
