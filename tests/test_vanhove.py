"""Device-side self van Hove functions (include/vvhip.h: vvhip_vanhove_*), the host half, no GPU: tests/vanhove_reference.py against a
plain Python loop, the invariant below + hist + beyond == pairs, the pair count per lag, uniform motion in closed form (an exact edge and the
zero displacement among it), the two-word r^4, the layout and the three exponents of an unbound plan, every refusal of the start in its
documented order, the struct sizes, the Python views against their formulas, the text writer read back, distributed.vanhove_sum, the
digest of the host tables."""
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
import msd_reference as MR          # noqa: E402
import vanhove_reference as VR      # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S = pkg.systems
R = pkg.reporters

ENTRY_POINTS = ("vvhip_vanhove_start", "vvhip_vanhove_read", "vvhip_vanhove_stop", "vvhip_vanhove_info")
EDGES = np.array([0.0, 0.25, 0.5, 1.0, 2.0])


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


def _describe(plan, interval=10, num_lags=8, origin_every=1, mode=0, num_groups=1, group=None, max_samples=1000, limit=0.0, edges=EDGES,
              num_bins=None):
    """vvhip_vanhove_start on an unbound plan: (return code, error text); a description that passes the checks in front of the bind is kept."""
    H = _I().H
    grp = None if group is None else np.ascontiguousarray(group, dtype=np.int8)
    e = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
    nb = (len(e) - 1 if e is not None else 0) if num_bins is None else num_bins
    desc = H.VanHoveDesc(interval, num_lags, origin_every, mode, num_groups, nb, None if grp is None else grp.ctypes.data,
                         None if e is None else e.ctypes.data, max_samples, limit)
    rc = H.lib.vvhip_vanhove_start(plan, C.byref(desc))
    return rc, H.lib.vvhip_last_error(plan).decode()


def _info(plan):
    H = _I().H
    lay = H.VanHoveLayout()
    assert H.lib.vvhip_vanhove_info(plan, C.byref(lay)) == H.OK
    return lay


def test_vanhove_entry_points_and_struct_sizes():
    H = _I().H
    for name in ENTRY_POINTS:
        assert name in H.EXPORTS and hasattr(H.lib, name)
    header = open(os.path.join(ROOT, "include", "vvhip.h")).read()
    for name in ENTRY_POINTS:
        assert "int %s(" % name in header
    assert C.sizeof(H.VanHoveDesc) == 56 and C.sizeof(H.VanHoveCounts) == 32 and C.sizeof(H.VanHoveLayout) == 104
    assert H.VANHOVE_MAX_WORDS == VR.MAX_WORDS and "#define VVHIP_VANHOVE_MAX_WORDS (1ll << 22)" in header


# ------------------------------------------------------------------------------------------ the reference against a plain loop
def _loop(x, masses, mol_id, groups, molecules, num_groups, num_lags, every, edges, exps, limit, floor):
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

    frac2, fh, d = exps
    e2 = [float(e) * float(e) for e in edges]
    B = len(e2) - 1
    head, hist, out = np.zeros((num_groups, num_lags, 6), dtype=np.int64), np.zeros((num_groups, num_lags, B), dtype=np.int64), 0
    c = [[centre(frame, mem) for _, mem in units] for frame in x]
    for j in range(len(x)):
        for o in range(j):
            if o % every or o < floor or j - o > num_lags:
                continue
            row = j - o - 1
            for u, (g, _) in enumerate(units):
                dl = [c[j][u][a] - c[o][u][a] for a in range(3)]
                if not all(abs(v) < limit for v in dl):
                    out += 1
                    continue
                r2 = (dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]
                head[g, row, 0] += 1
                if r2 < e2[0]:
                    head[g, row, 1] += 1
                elif r2 >= e2[B]:
                    head[g, row, 2] += 1
                else:
                    for b in range(B):
                        if e2[b] <= r2 < e2[b + 1]:
                            hist[g, row, b] += 1
                head[g, row, 3] += int(np.rint(r2 * 2.0 ** frac2))
                x4 = (r2 * r2) * 2.0 ** fh
                hi = float(np.floor(x4))
                head[g, row, 4] += int(hi)
                head[g, row, 5] += int(np.rint((x4 - hi) * 2.0 ** d))
    return head, hist, out


@pytest.mark.parametrize("molecules", [False, True], ids=["particles", "molecules"])
@pytest.mark.parametrize("num_lags,every,floor", [(1, 1, 0), (7, 3, 0), (8, 4, 0), (7, 3, 4)])
def test_reference_equals_a_plain_loop(molecules, num_lags, every, floor):
    rng = np.random.default_rng(5)
    n, J = 23, 13
    mol_id = np.sort(rng.integers(0, 7, size=n))
    masses = rng.uniform(1.0, 30.0, size=n)
    masses[rng.choice(n, size=4, replace=False)] = 0.0               # massless particles take no part in a centre of mass
    per_mol = rng.integers(-1, 2, size=7)
    groups = per_mol[mol_id].astype(np.int8)
    x = np.cumsum(rng.normal(0, 0.12, size=(J, n, 3)), axis=0)
    x[7, int(np.nonzero((groups >= 0) & (masses > 0))[0][0]), 1] = np.nan      # a recorded particle: its pairs with sample 7 are out of range
    limit, exps = 1.0, (30, 28, 40)
    edges = np.array([0.15, 0.2, 0.3, 0.4, 0.8])                    # edges[0] > 0: `below` is populated; limit sqrt(3) > 0.8: `beyond` can be
    c = [VR.unit_positions(f, masses, mol_id, groups, molecules) for f in x]
    head, hist, out = VR.vanhove_reference(np.array([p for p, _ in c]), c[0][1], 2, num_lags, every, edges, exps, limit, floor)
    want_head, want_hist, want_out = _loop(x.tolist(), masses.tolist(), mol_id.tolist(), groups.tolist(), molecules, 2, num_lags, every,
                                           edges.tolist(), exps, limit, floor)
    assert out == want_out > 0 and np.array_equal(head, want_head) and np.array_equal(hist, want_hist)
    assert head[:, :, 0].sum() > 0 and hist.sum() > 0 and head[:, :, 1].sum() > 0
    # the invariant, and the pair count per lag of the units that are never out of range
    assert np.array_equal(head[:, :, 1] + hist.sum(axis=2) + head[:, :, 2], head[:, :, 0])


@pytest.mark.parametrize("num_lags,every", [(1, 1), (7, 3), (8, 4)])
def test_invariant_and_pair_counts_per_lag(num_lags, every):
    rng = np.random.default_rng(8)
    U, J = 17, 19
    g = np.arange(U) % 3
    c = np.cumsum(rng.normal(0, 0.2, size=(J, U, 3)), axis=0)
    head, hist, out = VR.vanhove_reference(c, g, 3, num_lags, every, _I().vanhove_edges(0.45, 6, 0.25), (30, 20, 40), 16.0)
    assert out == 0
    assert np.array_equal(head[:, :, 1] + hist.sum(axis=2) + head[:, :, 2], head[:, :, 0])
    per_unit = MR.pair_counts(J, every, num_lags)
    for k in range(3):
        assert np.array_equal(head[k, :, 0], np.count_nonzero(g == k) * per_unit)
    assert head[:, :, 1].sum() > 0 and head[:, :, 2].sum() > 0


# ------------------------------------------------------------------------------------------ uniform motion
@pytest.mark.parametrize("v,edges", [((0.5, 0.0, 0.0), [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5]),      # |v| (l + 1) IS an edge: the upper bin
                                     ((0.375, -0.25, 0.125), np.linspace(0.0, 4.0, 33)),
                                     ((0.0, 0.0, 0.0), [0.0, 0.5, 1.0])],                                         # no displacement, edges[0] = 0: bin 0
                         ids=["on-an-edge", "generic", "at-rest"])
@pytest.mark.parametrize("num_lags,every", [(8, 1), (8, 4), (7, 3)])
def test_uniform_motion_in_closed_form(v, edges, num_lags, every):
    """x = x0 + v t on a dyadic grid: every displacement is exact, row l holds all its pairs in the one bin that contains |v| (l + 1)."""
    rng = np.random.default_rng(2)
    U, J, exps = 13, 25, (24, 20, 40)
    v, edges = np.array(v), np.asarray(edges, dtype=np.float64)
    x0 = rng.integers(-2 ** 20, 2 ** 20, size=(U, 3)).astype(np.float64) * 2.0 ** -12
    c = x0[None] + np.arange(J)[:, None, None] * v[None, None, :]
    head, hist, out = VR.vanhove_reference(c, np.zeros(U, dtype=int), 1, num_lags, every, edges, exps, 16.0)
    per_unit = MR.pair_counts(J, every, num_lags)
    assert out == 0 and np.array_equal(head[0, :, 0], U * per_unit) and not head[0, :, 1:3].any()
    for l in range(num_lags):
        r2 = float(np.dot(v, v)) * (l + 1) ** 2                      # exact
        b = [k for k in range(len(edges) - 1) if edges[k] ** 2 <= r2 < edges[k + 1] ** 2]
        assert len(b) == 1
        want = np.zeros(len(edges) - 1, dtype=np.int64)
        want[b[0]] = U * per_unit[l]
        assert np.array_equal(hist[0, l], want)
        assert head[0, l, 3] == U * per_unit[l] * int(np.rint(r2 * 2.0 ** 24))
        assert VR.r4_value(head[0, l, 4], head[0, l, 5], 20, 40) == U * per_unit[l] * r2 * r2
    if v[0] == 0.5:
        assert hist[0, 0, 1] == U * per_unit[0] and hist[0, 0, 0] == 0            # r = 0.5 exactly, an edge at 0.5: the upper bin
    if not v.any():
        assert hist[0, :, 0].sum() == U * per_unit.sum()


def test_two_word_r4_reconstructs_the_product():
    """Per term the two words give r2 * r2 to 2^-(fh + d): hi is exact, lo is the fraction rounded to d bits."""
    rng = np.random.default_rng(9)
    for limit, fh, d in ((16.0, 20, 40), (1.0, 40, 52), (64.0, 2, 30), (0.25, 40, 10)):
        top = 9.0 * limit ** 4
        r4 = np.concatenate([10.0 ** rng.uniform(-12, np.log10(top), size=4000), [1e-12, top * (1 - 2.0 ** -52), 0.0]])
        r2 = np.sqrt(r4)
        r2 = r2[r2 * r2 < top]
        hi, lo = VR.r4_words(r2, fh, d)
        assert np.all(hi >= 0) and np.all(lo >= 0) and np.all(lo <= 2 ** d) and np.all(hi < 2.0 ** (4 * np.log2(limit) + 4 + fh))
        # in exact arithmetic: (hi + lo 2^-d) 2^-fh against r2 * r2
        from fractions import Fraction
        for k in rng.choice(len(r2), size=200, replace=False):
            exact = Fraction(float(r2[k] * r2[k]))
            got = (Fraction(int(hi[k])) + Fraction(int(lo[k]), 2 ** d)) / 2 ** fh
            assert abs(got - exact) <= Fraction(1, 2 ** (fh + d))


# ------------------------------------------------------------------------------------------ the layout of an unbound plan
def test_layout_without_a_recorder_is_empty():
    H = _I().H
    plan, keep = _plan()
    try:
        lay = _info(plan)
        assert (lay.active, lay.words, lay.num_units, lay.ring_bytes, lay.num_bins, lay.head_words, lay.hist_words) == (0, 0, 0, 0, 0, 0, 0)
        assert H.lib.vvhip_vanhove_stop(plan) == H.OK
    finally:
        H.lib.vvhip_plan_destroy(plan)


@pytest.mark.parametrize("mode", [0, 1], ids=["particles", "molecules"])
@pytest.mark.parametrize("max_samples,every,limit", [(1000, 1, 0.0), (1 << 20, 4, 0.0), (4000, 3, 2.0 ** -10), (4000, 3, 3.0), (1 << 30, 1, 1.0)])
def test_layout_exponents_and_limit_of_an_unbound_plan(mode, max_samples, every, limit):
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
            assert lay.num_units == units_here and lay.num_origins == MR.num_origins(8, every) and lay.num_bins == 4
            assert (lay.head_words, lay.hist_words, lay.words) == (8 * 6, 8 * 4, 8 * 10)
            assert lay.limit == VR.applied_limit(limit) and lay.max_samples == max_samples
            assert (lay.frac2_bits, lay.r4_hi_bits, lay.r4_lo_bits) == VR.exponents(units_whole, max_samples, every, limit)      # of the WHOLE System on every shard
            assert lay.ring_bytes == lay.num_origins * 3 * ((units_here + 15) // 16 * 16) * 8
        finally:
            H.lib.vvhip_plan_destroy(plan)
    assert VR.applied_limit(0.0) == 16.0 and VR.applied_limit(3.0) == 4.0 and VR.applied_limit(2.0 ** -10) == 2.0 ** -10
    assert VR.exponents(1000, 1000, 1, 0.0) == (62 - 20 - 8 - 2, 62 - 20 - 16 - 4, 61 - 20)
    assert VR.exponents(3, 3, 1, 2.0 ** -10) == (40, 40, 52)


# ------------------------------------------------------------------------------------------ the refusals, in their order
def test_vanhove_start_refuses_in_the_documented_order():
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
    wide = np.linspace(0.0, 2.0, 1025)
    cu = MR.ceil_log2(len(MR.molecule_units(masses, mol)) + 1)
    try:
        kw = dict(interval=0, num_lags=5000, origin_every=0, mode=7, num_groups=17, group=bad_entry, max_samples=0, limit=-1.0,
                  edges=np.array([0.5, np.inf, 0.25]), num_bins=0)
        steps = [("interval", dict(interval=10)), ("num_lags", dict(num_lags=4096)), ("origin_every", dict(origin_every=1)), ("mode", dict(mode=1)),
                 ("num_groups", dict(num_groups=2)), ("max_samples", dict(max_samples=1 << 61)), ("limit", dict(limit=0.0)),
                 ("group[3]", dict(group=mixed)),
                 ("num_bins", dict(num_bins=1025)), ("num_bins", dict(num_bins=2, edges=None)), ("edges is null", dict(edges=np.array([0.5, np.inf, 0.25]))),
                 ("edges[1]", dict(edges=np.array([-0.5, 0.5, 0.25]))), ("edges[0]", dict(edges=np.array([0.5, 0.5, 0.25]))),
                 ("ascend", dict(edges=np.array([0.25, 0.5, 0.5]))), ("ascend", dict(edges=wide, num_bins=1024)),
                 ("different groups", dict(group=None)),
                 ("frac2_bits", dict(max_samples=(1 << (43 - cu)) - 1)),      # cu + co = 43 at the limit of 16 nm: frac2 = 52 - 43 >= 8, fh = 42 - 43 < 0
                 ("r4_hi_bits", dict(max_samples=1000)),
                 ("words", dict(num_bins=4, edges=EDGES)),           # 2 * 4096 * (6 + 1024) words
                 ("num_origins", dict(origin_every=4)), ("cuts a molecule", None)]
        for text, fix in steps:
            rc, err = _describe(plan, **kw)
            assert rc == (H.ERR_UNSUPPORTED if fix is None else H.ERR_INVALID) and text in err, (text, rc, err)
            assert _info(plan).words == 0                            # nothing of a refused description is kept
            if fix:
                kw.update(fix)
        assert str(2 * 4096 * (6 + 1024)) in _describe(plan, **dict(kw, num_bins=1024, edges=wide))[1]      # the cap's refusal carries the count
        # particle mode does not mind the cut; the unbound plan is the next refusal, and keeps the description
        kw.update(mode=0)
        rc, err = _describe(plan, **kw)
        assert rc == H.ERR_INVALID and "vvhip_bind" in err
        lay = _info(plan)
        assert lay.words == 2 * 4096 * 10 and lay.num_origins == 1024 and lay.active == 0
        # the rest of the surface on an unbound plan
        assert H.lib.vvhip_vanhove_read(plan, None, 0, None, 0) == H.ERR_INVALID
        assert H.lib.vvhip_vanhove_start(plan, None) == H.ERR_INVALID and "null description" in H.lib.vvhip_last_error(plan).decode()
        assert H.lib.vvhip_vanhove_stop(plan) == H.OK and _info(plan).words == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)


# ------------------------------------------------------------------------------------------ the Python views, the writer, the sum
def _fake(rng, groups=2, lags=9, bins=5, interval=10, empty_last=True, exps=(30, 20, 40)):
    I = _I()
    hist = rng.integers(0, 200, size=(groups, lags, bins)).astype(np.int64)
    head = np.zeros((groups, lags, 6), dtype=np.int64)
    head[:, :, 1] = rng.integers(0, 20, size=(groups, lags))
    head[:, :, 2] = rng.integers(0, 20, size=(groups, lags))
    head[:, :, 0] = head[:, :, 1] + head[:, :, 2] + hist.sum(axis=2)
    head[:, :, 3] = rng.integers(1, 2 ** 45, size=(groups, lags))
    head[:, :, 4] = rng.integers(1, 2 ** 40, size=(groups, lags))
    head[:, :, 5] = rng.integers(0, 2 ** 50, size=(groups, lags))
    if empty_last:
        head[:, -1, :] = 0
        hist[:, -1, :] = 0
    return I.VanHove(samples=40, dropped=1, out_of_range=3, origin_floor=2, interval=interval, origin_every=2, frac2_bits=exps[0],
                     r4_hi_bits=exps[1], r4_lo_bits=exps[2], molecules=False, edges=np.array([0.125, 0.25, 0.5, 1.0, 2.0, 4.0])[: bins + 1],
                     head=head, hist=hist)


def test_vanhove_views_against_their_formulas():
    rng = np.random.default_rng(3)
    m = _fake(rng)
    e = m.edges
    n = m.head[:, :-1, 0].astype(np.float64)
    assert np.array_equal(m.lag_steps, np.arange(1, 10) * 10) and np.array_equal(m.pairs, m.head[:, :, 0])
    for view in (m.P, m.G_s):
        assert view.shape == (2, 9, 5) and np.all(np.isnan(view[:, -1]))
    for view in (m.msd, m.r4, m.alpha2, m.Fs(3.0)[0], m.Fs(3.0)[1], m.overlap(0.5)):
        assert view.shape == (2, 9) and np.all(np.isnan(view[:, -1]))
    P = m.hist[:, :-1] / n[:, :, None]
    assert np.allclose(m.P[:, :-1], P, rtol=1e-12, atol=0)
    assert np.allclose(m.G_s[:, :-1], P / (4.0 / 3.0 * np.pi * (e[1:] ** 3 - e[:-1] ** 3)), rtol=1e-12, atol=0)
    msd = m.head[:, :-1, 3] / 2.0 ** 30 / n
    r4 = (m.head[:, :-1, 4] + m.head[:, :-1, 5] / 2.0 ** 40) / 2.0 ** 20 / n
    assert np.allclose(m.msd[:, :-1], msd, rtol=1e-12, atol=0) and np.allclose(m.r4[:, :-1], r4, rtol=1e-12, atol=0)
    assert np.allclose(m.alpha2[:, :-1], 3.0 * r4 / (5.0 * msd ** 2) - 1.0, rtol=1e-12, atol=0)
    k = 3.0
    mid = 0.5 * (e[1:] + e[:-1])
    F, lost = m.Fs(k)
    assert np.allclose(F[:, :-1], (P * np.sin(k * mid) / (k * mid)).sum(axis=2), rtol=1e-12, atol=0)
    assert np.allclose(lost[:, :-1], (m.head[:, :-1, 1] + m.head[:, :-1, 2]) / n, rtol=1e-12, atol=0)
    assert np.allclose(m.Fs(0.0)[0][:, :-1], P.sum(axis=2), rtol=1e-12, atol=0)
    assert np.allclose(m.overlap(0.5)[:, :-1], (m.head[:, :-1, 1] + m.hist[:, :-1, :2].sum(axis=2)) / n, rtol=1e-12, atol=0)
    assert np.allclose(m.overlap(e[0])[:, :-1], m.head[:, :-1, 1] / n, rtol=1e-12, atol=0)
    assert np.allclose(m.overlap(e[-1])[:, :-1], (n - m.head[:, :-1, 2]) / n, rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        m.overlap(0.3)                                               # not an edge: the histogram cannot split a bin


def test_relaxation_time_interpolates_between_rows():
    I = _I()
    lags = 6
    # one bin around r = 1 whose probability falls by row: Fs(k) = P sinc(k), everything else beyond
    want = np.array([0.9, 0.7, 0.5, 0.3, 0.2, 0.1])
    hist = np.rint(want * 1000).astype(np.int64).reshape(1, lags, 1)
    head = np.zeros((1, lags, 6), dtype=np.int64)
    head[0, :, 0] = 1000
    head[0, :, 2] = 1000 - hist[0, :, 0]
    m = I.VanHove(samples=7, dropped=0, out_of_range=0, origin_floor=0, interval=10, origin_every=1, frac2_bits=30, r4_hi_bits=20, r4_lo_bits=40,
                  molecules=True, edges=np.array([0.75, 1.25]), head=head, hist=hist)
    k = 1e-9                                                         # sinc -> 1: Fs is P itself
    t = m.relaxation_time(k, level=0.4, dt=0.5)
    assert t.shape == (1,) and np.isclose(t[0], (30 + 10 * (0.5 - 0.4) / (0.5 - 0.3)) * 0.5, rtol=1e-9)
    assert np.isclose(m.relaxation_time(k, level=0.95)[0], 10 * (1.0 - 0.95) / (1.0 - 0.9), rtol=1e-9)      # between the zero lag and row 0
    assert np.isnan(m.relaxation_time(k, level=0.05)[0])
    assert np.isclose(m.relaxation_time(k)[0], 30 + 10 * (0.5 - np.exp(-1)) / 0.2, rtol=1e-9)


def test_vanhove_edges_uniform_and_logarithmic():
    I = _I()
    u = I.vanhove_edges(2.0, 8)
    assert np.array_equal(u, np.arange(9) * 0.25)
    g = I.vanhove_edges(4.0, 128, 0.001)
    assert g.shape == (129,) and g[0] == 0.001 and g[-1] == 4.0 and np.all(np.diff(g) > 0)
    assert np.allclose(g[1:] / g[:-1], (4.0 / 0.001) ** (1 / 128), rtol=1e-12)
    with pytest.raises(ValueError):
        I.vanhove_edges(1.0, 8, 0.0)


def test_write_vanhove_round_trips_through_loadtxt():
    m = _fake(np.random.default_rng(4), bins=3)
    out = io.StringIO()
    R.write_vanhove(out, m, 0.001)
    text = out.getvalue()
    head = text.splitlines()[:3]
    assert head[0] == '#"Samples"\t40\t"Dropped"\t1\t"OutOfRange"\t3\t"OriginFloor"\t2'
    assert head[1] == '#"Edges (nm)"\t0.125\t0.25\t0.5\t1.0'
    per = 6 + 3
    assert head[2].startswith('#"lag (ps)"\t"pairs[0]"\t"below[0]"\t"beyond[0]"\t"msd[0] (nm^2)"\t"r4[0] (nm^4)"\t"alpha2[0]"\t"P[0][0]"') and head[2].count("\t") == 2 * per
    back = np.loadtxt(io.StringIO(text))
    assert back.shape == (9, 1 + 2 * per)
    assert np.array_equal(back[:, 0], m.lag_steps * 0.001)
    for g in range(2):
        col = 1 + per * g
        assert np.array_equal(back[:, col], m.pairs[g].astype(np.float64)) and np.array_equal(back[:, col + 1], m.below[g].astype(np.float64))
        assert np.array_equal(back[:, col + 2], m.beyond[g].astype(np.float64))
        assert np.array_equal(back[:, col + 3], m.msd[g], equal_nan=True) and np.array_equal(back[:, col + 4], m.r4[g], equal_nan=True)
        assert np.array_equal(back[:, col + 5], m.alpha2[g], equal_nan=True)
        assert np.array_equal(back[:, col + 6: col + 9], m.P[g], equal_nan=True)
    plain = io.StringIO()
    R.write_vanhove(plain, m, 0.001, header=False)
    assert plain.getvalue() == "\n".join(text.splitlines()[3:]) + "\n"


def test_vanhove_sum_adds_the_words_as_integers():
    import dataclasses
    D = pkg.distributed
    rng = np.random.default_rng(6)
    a, b = _fake(rng, empty_last=False), _fake(rng, empty_last=False)
    a.head[0, 0, 3] = 2 ** 62 - 5                                    # beyond float64's integers: the sum is an integer sum
    b.head[0, 0, 3] = 3
    s = D.vanhove_sum([a, b])
    assert s.head.dtype == np.int64 and s.hist.dtype == np.int64
    assert np.array_equal(s.head, a.head + b.head) and np.array_equal(s.hist, a.hist + b.hist) and s.head[0, 0, 3] == 2 ** 62 - 2
    assert (s.samples, s.dropped, s.out_of_range, s.origin_floor) == (40, 1, 6, 2)
    for other in (dataclasses.replace(b, frac2_bits=29), dataclasses.replace(b, r4_hi_bits=19), dataclasses.replace(b, r4_lo_bits=39),
                  dataclasses.replace(b, samples=39), dataclasses.replace(b, head=b.head[:, :-1], hist=b.hist[:, :-1]),
                  dataclasses.replace(b, hist=b.hist[:, :, :-1], edges=b.edges[:-1]), dataclasses.replace(b, edges=b.edges * 2),
                  dataclasses.replace(b, origin_every=1), dataclasses.replace(b, molecules=True)):
        with pytest.raises(ValueError):
            D.vanhove_sum([a, other])


# ------------------------------------------------------------------------------------------ the digest of the host tables
def test_recorder_digest_answers_for_vanhove():
    H = _I().H
    H.lib.vvhip_debug_recorder_digest.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64)]
    plan, keep = _plan()
    try:
        def digest(name=b"vanhove"):
            out = C.c_uint64(1)
            assert H.lib.vvhip_debug_recorder_digest(plan, name, C.byref(out)) == H.OK
            return out.value

        assert digest() == 0                                         # nothing described
        _describe(plan, edges=EDGES)
        first = digest()
        assert first != 0 and digest(b"msd") == 0
        _describe(plan, edges=EDGES)
        assert digest() == first
        _describe(plan, edges=EDGES * 2)
        assert digest() not in (0, first)                            # e2 is part of it
        _describe(plan, edges=EDGES, mode=1)
        assert digest() not in (0, first)
        assert H.lib.vvhip_vanhove_stop(plan) == H.OK and digest() == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)
