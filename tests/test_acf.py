"""Device-side velocity and orientation autocorrelations (include/vvhip.h: vvhip_acf_*), the host half, no GPU: tests/acf_reference.py
against a brute-force float64 evaluation, the exact cases (a constant dyadic vector, a rotation by 90 degrees per sample, the pair counts in
closed form, the floor, a restart, max_samples, a bad vector at either end), the unit vectors' condition | |u|^2 - 1 | <= 2^-49 and the
host build of csrc/vv_layout.h's acf_inverse_norm by a digest, the Python views (Green-Kubo, spectrum, P1, P2, relaxation time), the text
writer, distributed.acf_sum, the layout of an unbound plan and every refusal of the start in its documented order."""
import ctypes as C
import importlib
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import acf_reference as AR      # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S = pkg.systems
R = pkg.reporters

ENTRY_POINTS = ("vvhip_acf_start", "vvhip_acf_read", "vvhip_acf_stop", "vvhip_acf_info")


def _I():
    return importlib.import_module("openmm-velocityverlet_amd.integrator")


def _describe(plan, interval=10, num_lags=8, origin_every=1, mode=0, num_groups=1, group=None, pairs=None, max_samples=1000, limit=0.0, num_pairs=None):
    """vvhip_acf_start on an unbound plan: (return code, error text); a description that passes the checks in front of the bind is kept."""
    H = _I().H
    grp = None if group is None else np.ascontiguousarray(group, dtype=np.int8)
    pr = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    desc = H.AcfDesc(interval, num_lags, origin_every, mode, num_groups, (0 if pr is None else len(pr)) if num_pairs is None else num_pairs,
                     None if grp is None else grp.ctypes.data, None if pr is None else pr.ctypes.data, max_samples, limit)
    rc = H.lib.vvhip_acf_start(plan, C.byref(desc))
    return rc, H.lib.vvhip_last_error(plan).decode()


def _info(plan):
    H = _I().H
    lay = H.AcfLayout()
    assert H.lib.vvhip_acf_info(plan, C.byref(lay)) == H.OK
    return lay


def test_acf_entry_points_and_struct_sizes():
    H = _I().H
    for name in ENTRY_POINTS:
        assert name in H.EXPORTS and hasattr(H.lib, name)
    assert (C.sizeof(H.AcfDesc), C.sizeof(H.AcfCounts), C.sizeof(H.AcfLayout)) == (56, 32, 80)
    assert (H.ACF_VELOCITY_PARTICLES, H.ACF_VELOCITY_MOLECULES, H.ACF_ORIENTATION) == (AR.VELOCITY, AR.MOLECULES, AR.ORIENTATION) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "vvhip.h")).read()
    for name in ("vvhip_acf_desc", "vvhip_acf_counts", "vvhip_acf_layout", "VVHIP_ACF_VELOCITY_PARTICLES 0", "VVHIP_ACF_VELOCITY_MOLECULES 1",
                 "VVHIP_ACF_ORIENTATION 2"):
        assert name in hdr


# ------------------------------------------------------------------------------------------ the reference against a brute-force evaluation
def _random_vectors(rng, J, U, mode):
    a = rng.standard_normal((J, U, 3))
    if mode == AR.ORIENTATION:
        return np.array([AR.unit_vectors(x * 0.1) for x in a])
    return a * 0.5


@pytest.mark.parametrize("mode", [AR.VELOCITY, AR.ORIENTATION], ids=["velocity", "orientation"])
@pytest.mark.parametrize("num_lags,every,floor", [(8, 3, 0), (8, 1, 0), (8, 8, 5), (1, 1, 0), (5, 2, 3)])
def test_reference_equals_a_brute_force_evaluation(mode, num_lags, every, floor):
    """A plain float64 loop over samples, origins, units: the pair counts are equal, and every sum is within the fixed point's resolution
    -- half a unit of 2^-F per term from the rounding -- plus the float64 sum's own error."""
    rng = np.random.default_rng(5 + num_lags + every)
    J, U, G, F = 19, 23, 3, 30
    a = _random_vectors(rng, J, U, mode)
    g = rng.integers(0, G, size=U)
    table, out = AR.acf_reference(a, g, G, num_lags, every, F, mode, floor)
    W = AR.row_words(mode)
    assert table.shape == (G, num_lags, W) and table.dtype == np.int64 and out == 0
    count, sums = np.zeros((G, num_lags)), np.zeros((G, num_lags, W - 1))
    for j in range(J):
        for o in range(0, j + 1, every):
            if o < floor or j - o >= num_lags:
                continue
            for u in range(U):
                p = a[o, u] * a[j, u]
                count[g[u], j - o] += 1
                sums[g[u], j - o, :3] += p
                if W == 5:
                    sums[g[u], j - o, 3] += p.sum() ** 2
    assert np.array_equal(table[:, :, 0], count.astype(np.int64)) and count.sum() > 0
    err = np.abs(table[:, :, 1:] * 2.0 ** -F - sums)
    assert np.all(err <= (0.5 * 2.0 ** -F + 2.0 ** -48) * np.maximum(count, 1)[:, :, None]), err.max()


def test_molecule_vectors_are_the_sequential_mass_weighted_sum():
    rng = np.random.default_rng(3)
    masses = np.array([12.0, 1.0, 0.0, 16.0, 1.0, 1.0, 0.4, 14.0])
    mol = np.array([0, 0, 0, 1, 1, 1, 1, 2])
    v = rng.standard_normal((8, 3))
    a, g = AR.unit_vectors_of_sample(AR.MOLECULES, 64.0, v=v, masses=masses, mol_id=mol)
    assert a.shape == (3, 3) and list(g) == [0, 0, 0]
    s = 0.0 + 16.0 * v[3]
    s = s + 1.0 * v[4]
    s = s + 1.0 * v[5]
    s = s + 0.4 * v[6]
    M = ((16.0 + 1.0) + 1.0) + 0.4
    assert np.array_equal(a[1], s / M) and np.array_equal(a[2], (14.0 * v[7]) / 14.0)


# ------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("num_lags,every", [(8, 3), (8, 1), (8, 8), (1, 1)])
def test_constant_dyadic_vector_is_exact(num_lags, every):
    J, U, F = 21, 5, 40
    v = np.array([0.75, -1.5, 0.015625])
    a = np.broadcast_to(v, (J, U, 3))
    table, out = AR.acf_reference(a, np.zeros(U, dtype=int), 1, num_lags, every, F, AR.VELOCITY)
    pairs = U * AR.pair_counts(J, every, num_lags)
    assert out == 0 and np.array_equal(table[0, :, 0], pairs) and pairs[0] > 0
    for k in range(3):
        assert np.array_equal(table[0, :, 1 + k], pairs * int(v[k] * v[k] * 2 ** F))


def test_rotation_by_a_quarter_turn_per_sample_is_exact():
    """d = 4 (cos, sin, 0) of j quarter turns: the sequence gives y = 1/4 exactly, so P1 = 1, 0, -1, 0, ... and P2 = 1, -1/2, 1, ..."""
    I = _I()
    J, U, F, L = 24, 3, 40, 8
    quarter = np.array([[4.0, 0, 0], [0, 4.0, 0], [-4.0, 0, 0], [0, -4.0, 0]])
    a = np.array([np.broadcast_to(AR.unit_vectors(quarter[j % 4][None])[0], (U, 3)) for j in range(J)])
    assert np.array_equal(np.abs(a).sum(axis=2), np.ones((J, U)))
    table, out = AR.acf_reference(a, np.zeros(U, dtype=int), 1, L, 1, F, AR.ORIENTATION)
    acf = I.Autocorrelations(samples=J, dropped=0, out_of_range=out, origin_floor=0, interval=1, origin_every=1, frac_bits=F, mode="orientation", words=table)
    assert np.array_equal(acf.P1(0), np.array([1.0, 0, -1, 0] * 2)) and np.array_equal(acf.P2(0), np.array([1.0, -0.5] * 4))
    assert np.array_equal(acf.squares[0], acf.pairs[0] * np.array([1.0, 0] * 4))


@pytest.mark.parametrize("num_lags,every", [(8, 3), (8, 1), (8, 8), (1, 1), (5, 2)])
@pytest.mark.parametrize("J", [0, 1, 2, 7, 30])
def test_pair_count_per_lag_in_closed_form(num_lags, every, J):
    want = np.zeros(num_lags, dtype=np.int64)
    for _, _, row in AR.pairs_of(J, every, num_lags):
        want[row] += 1
    assert np.array_equal(AR.pair_counts(J, every, num_lags), want)
    # every origin is used at most num_lags samples long: the ring of ceil(num_lags / E) slots holds them all
    for j, o, _ in AR.pairs_of(J, every, num_lags):
        assert o % every == 0 and j - o < num_lags and (j // every - o // every) < -(-num_lags // every)


def test_floor_restart_and_max_samples():
    rng = np.random.default_rng(11)
    J, U, F = 15, 4, 30
    a, g = rng.standard_normal((J, U, 3)), np.zeros(U, dtype=int)
    # a floor kills the origins below it from the sample on at which it stands, the table so far is kept
    floors = [0] * 5 + [5] * 4 + [9] * 6
    table, _ = AR.acf_reference(a, g, 1, 8, 1, F, AR.VELOCITY, floors)
    want = AR.acf_reference(a[:5], g, 1, 8, 1, F, AR.VELOCITY)[0] + AR.acf_reference(a[5:9], g, 1, 8, 1, F, AR.VELOCITY)[0] + \
        AR.acf_reference(a[9:], g, 1, 8, 1, F, AR.VELOCITY)[0]
    assert np.array_equal(table, want) and table[0, :, 0].sum() < U * AR.pair_counts(J, 1, 8).sum()
    # with E = 2 a floor at an odd ordinal leaves the next even one as the first origin
    assert [p for p in AR.pairs_of(6, 2, 8, [0, 0, 0, 3, 3, 3])] == [(0, 0, 0), (1, 0, 1), (2, 0, 2), (2, 2, 0), (4, 4, 0), (5, 4, 1)]
    # past max_samples a sample adds nothing; a restart (reset) is the reference over the later samples alone
    capped, _ = AR.acf_reference(a, g, 1, 8, 3, F, AR.VELOCITY, max_samples=5)
    assert np.array_equal(capped, AR.acf_reference(a[:5], g, 1, 8, 3, F, AR.VELOCITY)[0])
    assert np.array_equal(AR.acf_reference(a[5:], g, 1, 8, 3, F, AR.VELOCITY)[0][0, :, 0], U * AR.pair_counts(10, 3, 8))


def test_a_bad_vector_at_either_end_leaves_the_pair_out():
    rng = np.random.default_rng(13)
    J, U, F, limit = 9, 6, 30, 0.25
    v = rng.uniform(-0.2, 0.2, size=(J, U, 3))
    v[3, 2, 1] = 0.25                                                # at the limit: bad
    v[6, 4, 0] = np.nan
    a = np.array([AR.unit_vectors_of_sample(AR.VELOCITY, limit, v=x)[0] for x in v])
    assert np.all(np.isnan(a[3, 2])) and np.all(np.isnan(a[6, 4])) and np.count_nonzero(np.isnan(a[:, :, 0])) == 2
    table, out = AR.acf_reference(a, np.zeros(U, dtype=int), 1, 4, 1, F, AR.VELOCITY)
    # sample 3 of unit 2 is an end of the pairs (3, o <= 3) and (j >= 3, 3): 4 + 4 - 1; sample 6 of unit 4: 4 + 3 - 1
    assert out == 7 + 6 and table[0, :, 0].sum() == U * AR.pair_counts(J, 1, 4).sum() - out
    clean = np.where(np.isnan(a), 0.0, a)
    assert np.array_equal(table[0, :, 1:], AR.acf_reference(clean, np.zeros(U, dtype=int), 1, 4, 1, F, AR.VELOCITY)[0][0, :, 1:])
    # orientation: n2 outside [2^-40, 2^40) or NaN
    d = np.array([[2.0 ** -20, 0, 0], [2.0 ** -21, 0, 0], [2.0 ** 19.5, 0, 0], [2.0 ** 20, 0, 0], [np.nan, 1, 1], [0, 0, 0], [1, 2, 2]])
    u = AR.unit_vectors(d)
    assert list(np.isnan(u[:, 0])) == [False, True, False, True, True, True, False] and np.array_equal(u[6], np.array([1, 2, 2]) * AR.inverse_norm(np.array([9.0]))[0])


# ------------------------------------------------------------------------------------------ the unit vectors
def _condition_vectors():
    rng = np.random.default_rng(2024)
    d = rng.standard_normal((200000, 3))
    d = d / np.sqrt((d * d).sum(axis=1))[:, None] * np.exp2(rng.uniform(-19.0, 19.0, size=200000))[:, None]
    return d


def test_unit_vectors_meet_the_condition():
    """| |u|^2 - 1 | <= 2^-49 over 2e5 random directions with lengths spread over 2^-19 .. 2^19 nm.  |u|^2 is evaluated in extended
    precision (64-bit mantissa: the evaluation's own error is below 2^-61), or exactly in rationals where the platform has none."""
    d = _condition_vectors()
    u = AR.unit_vectors(d)
    assert not np.isnan(u).any()
    n = np.sqrt((d * d).sum(axis=1))
    assert n.min() < 2.0 ** -18 and n.max() > 2.0 ** 18
    if np.finfo(np.longdouble).nmant >= 63:
        ul = u.astype(np.longdouble)
        err = float(np.abs((ul * ul).sum(axis=1) - 1).max())
    else:
        from fractions import Fraction
        err = max(abs(float(sum(Fraction(float(c)) ** 2 for c in v) - 1)) for v in u)
    assert err <= AR.UNIT_BOUND, err
    # the reciprocal norm itself: within 2^-51 of the float64 division
    n2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert np.abs(AR.inverse_norm(n2) * np.sqrt(n2) - 1).max() < 2.0 ** -51


def _mix(k):
    with np.errstate(over="ignore"):
        z = (k + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_build_of_the_inverse_norm_equals_numpy(tmp_path):
    """tests/cpp/acf_unit_check.cpp compiles vv_layout.h's acf_inverse_norm without contraction, under the address and undefined-behaviour
    sanitizers, and prints a digest of the unit vectors' bits over a fixed vector list; NumPy forms the same digest from the reference."""
    exe = str(tmp_path / "acf_unit_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "openmm-velocityverlet_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "acf_unit_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout.split()
    i = np.arange(1 << 18, dtype=np.uint64)
    s = (_mix(np.uint64(4) * i + np.uint64(3)) % np.uint64(39)).astype(np.int64) - 19
    d = np.stack([((_mix(np.uint64(4) * i + np.uint64(a)) >> np.uint64(11)).astype(np.int64) - (1 << 52)).astype(np.float64) * 2.0 ** -52 * np.exp2(s.astype(np.float64))
                  for a in range(3)], axis=1)
    n2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    keep = (n2 >= AR.N2_MIN) & (n2 < AR.N2_MAX)
    u = np.ascontiguousarray(d[keep] * AR.inverse_norm(n2[keep])[:, None])
    assert np.array_equal(u, AR.unit_vectors(d[keep])) and (1 << 18) - 1024 < keep.sum() < (1 << 18)      # (a few of the shortest fall below 2^-40 nm^2: skipped on both sides)
    with np.errstate(over="ignore"):
        terms = ((i[keep] + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.ascontiguousarray(u[:, 0]).view(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F) +
                 np.ascontiguousarray(u[:, 1]).view(np.uint64) * np.uint64(0x165667B19E3779F9) + np.ascontiguousarray(u[:, 2]).view(np.uint64) * np.uint64(0x27D4EB2F165667C5))
        digest = int(np.add.reduce(terms, dtype=np.uint64))
    assert int(out[0]) == int(keep.sum())
    assert int(out[1], 16) == digest


# ------------------------------------------------------------------------------------------ the Python views, the writer, the sum
def _table_of(curves, pairs, frac, squares=None):
    """words [G, L, 4 | 5] whose C(g) is curves[g] (all of it in the x component) with `pairs` pairs per row."""
    curves = np.atleast_2d(curves)
    words = np.zeros(curves.shape + (4 if squares is None else 5,), dtype=np.int64)
    words[:, :, 0] = pairs
    words[:, :, 1] = np.rint(curves * pairs * 2.0 ** frac).astype(np.int64)
    if squares is not None:
        words[:, :, 4] = np.rint(np.atleast_2d(squares) * pairs * 2.0 ** frac).astype(np.int64)
    return words


def _acf(words, mode="velocity", frac=40, interval=2):
    return _I().Autocorrelations(samples=40, dropped=1, out_of_range=3, origin_floor=2, interval=interval, origin_every=2, frac_bits=frac, mode=mode, words=words)


def test_green_kubo_of_an_exponential_and_the_spectrum_of_a_cosine():
    L, interval, dt, tau, A = 400, 2, 0.001, 0.05, 0.3
    t = np.arange(L) * interval * dt
    acf = _acf(_table_of([A * np.exp(-t / tau), A * np.cos(2 * np.pi * 25.0 * t)], 1000, 40), interval=interval)
    assert np.array_equal(acf.lag_steps, np.arange(L) * interval) and acf.pairs.shape == (2, L) and acf.sums.shape == (2, L, 3)
    assert np.allclose(acf.C(0), A * np.exp(-t / tau), rtol=0, atol=2.0 ** -39) and np.allclose(acf.normalized(0), np.exp(-t / tau), atol=1e-9)
    # the trapezoid of A exp(-t / tau) / 3 over [0, T]: A tau (1 - exp(-T / tau)) / 3 up to h^2 / (12 tau^2)
    h = interval * dt
    exact = A * tau * (1 - np.exp(-t[-1] / tau)) / 3
    assert abs(acf.diffusion_green_kubo(0, dt) - exact) <= exact * h * h / (12 * tau * tau) * 1.01 + 1e-12
    half = acf.diffusion_green_kubo(0, dt, upto=100)
    assert abs(half - A * tau * (1 - np.exp(-t[100] / tau)) / 3) <= exact * 2e-4 and half < acf.diffusion_green_kubo(0, dt)
    # the cosine of 25 THz peaks at 25 THz, with and without the window
    for window in ("hann", None):
        f, s = acf.spectrum(1, dt, window=window)
        assert f.shape == s.shape == (L,) and f[0] == 0 and abs(f[1] - 1 / (2 * L * h)) < 1e-12
        assert abs(f[int(np.argmax(s))] - 25.0) <= f[1]
    with pytest.raises(ValueError):
        acf.spectrum(1, dt, window="boxcar")
    with pytest.raises(ValueError):
        acf.P1(0)
    with pytest.raises(ValueError, match="P2 belongs"):
        acf.P2(0)
    with pytest.raises(ValueError):
        acf.squares


def test_orientation_views_and_the_relaxation_time():
    L, interval, tau = 50, 5, 40.0
    t = np.arange(L) * interval
    p1 = np.exp(-t / tau)
    sq = (2 * np.exp(-3 * t / tau) + 1) / 3                          # P2 = exp(-3 t / tau)
    acf = _acf(_table_of([p1], 640, 40, squares=[sq]), mode="orientation", interval=interval)
    assert np.allclose(acf.P1(0), p1, atol=1e-10) and np.allclose(acf.P2(0), np.exp(-3 * t / tau), atol=1e-10)
    assert abs(acf.relaxation_time(0, 1) - tau) < 0.02 * tau and abs(acf.relaxation_time(0, 2, dt=0.5) - tau / 6) < 0.02 * tau
    with pytest.raises(ValueError):
        acf.relaxation_time(0, 3)
    with pytest.raises(ValueError):
        acf.diffusion_green_kubo(0, 0.001)
    empty = _acf(np.zeros((1, 4, 5), dtype=np.int64), mode="orientation")
    assert np.isnan(empty.P1(0)).all() and np.isnan(empty.P2(0)).all()


@pytest.mark.parametrize("mode", ["velocity", "orientation"])
def test_write_acf_round_trips_through_loadtxt(mode):
    rng = np.random.default_rng(7)
    words = np.zeros((2, 6, 5 if mode == "orientation" else 4), dtype=np.int64)
    words[:, :, 0] = rng.integers(1, 500, size=(2, 6))
    words[:, :, 1:] = rng.integers(-2 ** 40, 2 ** 40, size=words[:, :, 1:].shape)
    words[1, -1] = 0
    acf = _acf(words, mode=mode, frac=30, interval=10)
    buf = io.StringIO()
    R.write_acf(buf, acf, 0.002)
    lines = buf.getvalue().splitlines()
    assert lines[0] == '#"Samples"\t40\t"Dropped"\t1\t"OutOfRange"\t3\t"OriginFloor"\t2' and lines[1].startswith('#"lag (ps)"')
    back = np.loadtxt(io.StringIO(buf.getvalue()), ndmin=2)
    cols = R.acf_columns(acf, 0.002)
    assert back.shape == (6, len(cols)) and back[0, 0] == 0.0 and back[1, 0] == 10 * 0.002
    for k, (_, v) in enumerate(cols):
        assert np.array_equal(back[:, k], v, equal_nan=True)


def test_acf_sum_adds_the_words_as_integers():
    import dataclasses
    D = importlib.import_module("openmm-velocityverlet_amd.distributed")
    rng = np.random.default_rng(9)
    parts = [_acf(rng.integers(-2 ** 50, 2 ** 50, size=(2, 5, 4)).astype(np.int64)) for _ in range(3)]
    total = D.acf_sum(parts)
    assert np.array_equal(total.words, parts[0].words + parts[1].words + parts[2].words) and total.out_of_range == 9 and total.samples == 40
    with pytest.raises(ValueError):
        D.acf_sum([parts[0], dataclasses.replace(parts[1], samples=41)])


# ------------------------------------------------------------------------------------------ the layout of an unbound plan, the refusals
def test_layout_of_an_unbound_plan():
    I = _I()
    H = I.H
    spec = S.make_config("C3", scale=0.05)
    n = spec.num_atoms
    plan, _, keep = I.create_plan(spec, I.VVIntegrator(333.0, 10.0, 1.0, 40.0, 0.001), "mixed", None)
    try:
        lay = _info(plan)
        assert (lay.active, lay.words, lay.num_units, lay.row_words) == (0, 0, 0, 0)
        rc, err = _describe(plan, num_lags=8, origin_every=3, max_samples=1000, limit=3.0)
        assert rc == H.ERR_INVALID and "vvhip_bind" in err         # an unbound plan cannot record, but answers for the layout
        lay = _info(plan)
        assert (lay.active, lay.num_units, lay.num_origins, lay.row_words, lay.words, lay.limit) == (0, n, 3, 4, 8 * 4, 4.0)
        assert lay.frac_bits == AR.frac_bits(n, 1000, 3, AR.VELOCITY, 3.0) and lay.ring_bytes == 3 * 3 * ((n + 15) // 16 * 16) * 8
        pairs = np.asarray(spec.drude_pairs, dtype=np.int32)[:, :2]
        grp = (np.arange(len(pairs)) % 3 - 1).astype(np.int8)
        rc, err = _describe(plan, mode=2, num_groups=2, group=grp, pairs=pairs, max_samples=1 << 20)
        assert rc == H.ERR_INVALID and "vvhip_bind" in err
        lay = _info(plan)
        units = int(np.count_nonzero(grp >= 0))
        assert (lay.mode, lay.num_units, lay.row_words, lay.words, lay.limit) == (2, units, 5, 2 * 8 * 5, 1.0)
        assert lay.frac_bits == AR.frac_bits(units, 1 << 20, 1, AR.ORIENTATION) == min(40, 62 - AR.MR.ceil_log2(units + 1) - 21)
        assert H.lib.vvhip_acf_stop(plan) == H.OK and _info(plan).words == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)


def test_acf_start_refuses_in_the_documented_order():
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
        kw = dict(interval=0, num_lags=5000, origin_every=0, mode=7, num_groups=17, group=bad_entry, max_samples=0, limit=-1.0, pairs=[[1, 5]])
        steps = [("interval", dict(interval=10)), ("num_lags", dict(num_lags=4096)), ("origin_every", dict(origin_every=1)), ("mode", dict(mode=1)),
                 ("num_groups", dict(num_groups=2)), ("max_samples", dict(max_samples=1 << 61)), ("limit", dict(limit=0.0)),
                 ("orientation mode only", dict(pairs=None)), ("group[3]", dict(group=mixed)), ("different groups", dict(group=None)),
                 ("fraction bits", dict(max_samples=1000)), ("num_origins", dict(origin_every=4)), ("cuts a molecule", None)]
        for text, fix in steps:
            rc, err = _describe(plan, **kw)
            assert rc == (H.ERR_UNSUPPORTED if fix is None else H.ERR_INVALID) and text in err, (text, rc, err)
            assert _info(plan).words == 0                            # nothing of a refused description is kept
            if fix:
                kw.update(fix)
        # orientation mode: its own refusals, then the pair the shard cuts
        kw.update(mode=2, limit=1.0, pairs=[[1, 5], [2, 2], [0, n], [1, 2], [2, 6]], group=np.array([0, 1, 0, 7, 0], dtype=np.int8))
        assert mol[1] != mol[2]
        steps = [("limit must be 0", dict(limit=0.0)), ("group[3]", dict(group=None)), ("pair 1", dict(pairs=[[1, 5], [0, n], [1, 2], [2, 6]])),
                 ("outside the System", dict(pairs=[[1, 5], [1, 2], [2, 6]])), ("joins molecules", dict(pairs=[[1, 5], [2, 6]])), ("cuts a recorded pair", None)]
        for text, fix in steps:
            rc, err = _describe(plan, **kw)
            assert rc == (H.ERR_UNSUPPORTED if fix is None else H.ERR_INVALID) and text in err, (text, rc, err)
            assert _info(plan).words == 0
            if fix:
                kw.update(fix)
        rc, err = _describe(plan, **dict(kw, pairs=None, num_pairs=2))
        assert rc == H.ERR_INVALID and "needs pairs" in err
        # particle mode does not mind the cut; the unbound plan is the next refusal, and keeps the description
        kw.update(mode=0, pairs=None)
        rc, err = _describe(plan, **kw)
        assert rc == H.ERR_INVALID and "vvhip_bind" in err
        assert _info(plan).words == 2 * 4096 * 4 and _info(plan).num_origins == 1024 and _info(plan).active == 0 and _info(plan).num_units == 3
        # the rest of the surface on an unbound plan
        assert H.lib.vvhip_acf_read(plan, None, 0, None, 0) == H.ERR_INVALID
        assert H.lib.vvhip_acf_start(plan, None) == H.ERR_INVALID and "null description" in H.lib.vvhip_last_error(plan).decode()
        assert H.lib.vvhip_acf_stop(plan) == H.OK and _info(plan).words == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)
