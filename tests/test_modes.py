"""Device-side density modes (include/vvhip.h: vvhip_modes_*), the host half, no GPU: the phasor of tests/modes_reference.py against long
double, the host build of csrc/vv_layout.h's phasor against the same NumPy by a digest, the exact lattice case, the wrap cases against
Python integers, the ideal gas, the ABI on an unbound plan (struct sizes, every refusal in the documented order, the kept description,
num_lags = 0, the table cap), the DensityModes views, modes_in_shells and the text writer."""
import ctypes as C
import importlib
import io
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import modes_reference as MR      # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S = pkg.systems
R = pkg.reporters

ENTRY_POINTS = ("vvhip_modes_start", "vvhip_modes_read", "vvhip_modes_stop", "vvhip_modes_info")


def _I():
    return importlib.import_module("openmm-velocityverlet_amd.integrator")


# ------------------------------------------------------------------------------------------ the phasor
def _edges():
    """Every quadrant and octant edge (and the sixteenths between) with -1, 0, +1."""
    return np.array([((e << 28) + d) % (1 << 32) for e in range(16) for d in (-1, 0, 1)], dtype=np.uint64)


def test_phasor_is_within_the_derived_bound_of_long_double():
    """2^22 random phases plus the edges.  The truth: cos and sin in long double of the exactly reduced argument (the quadrant and the
    signed offset are integers; pi in long double), selected by the quadrant.  Bound: 2^-51 absolute, derived from the rounding steps
    (the product r C, z, six Horner steps on terms that shrink by z <= 0.62 each, the last two adds: below 4 x 2^-53)."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("long double is no wider than double on this machine")
    rng = np.random.default_rng(20261020)
    phi = np.concatenate([rng.integers(0, 1 << 32, size=1 << 22, dtype=np.uint64), _edges()])
    co, si = MR.phasor(phi)
    t = (phi + np.uint64(1 << 29)) & MR.MASK
    q = (t >> np.uint64(30)).astype(np.int64)
    r = (t & np.uint64((1 << 30) - 1)).astype(np.int64) - (1 << 29)
    pi = np.arctan(np.longdouble(1)) * 4
    x = r.astype(np.longdouble) * (pi / np.longdouble(2.0 ** 31))
    cs, sn = np.cos(x), np.sin(x)
    want_c = np.choose(q, [cs, -sn, -cs, sn])
    want_s = np.choose(q, [sn, cs, -sn, -cs])
    worst = float(max(np.abs(co.astype(np.longdouble) - want_c).max(), np.abs(si.astype(np.longdouble) - want_s).max()))
    assert worst <= 2.0 ** -51, "worst absolute error %.3f x 2^-53" % (worst * 2.0 ** 53)
    assert np.abs(co * co + si * si - 1.0).max() < 2.0 ** -50


def _digest(phi):
    co, si = MR.phasor(phi)
    with np.errstate(over="ignore"):
        terms = ((phi + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + co.view(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F) +
                 si.view(np.uint64) * np.uint64(0x165667B19E3779F9))
        return int(np.add.reduce(terms, dtype=np.uint64))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_build_of_the_phasor_equals_numpy(tmp_path):
    """tests/cpp/phasor_check.cpp compiles vv_layout.h's phasor_turns without contraction and prints a digest of the (cos, sin) bits over a
    fixed phase list; NumPy forms the same digest from the reference's phasor."""
    exe = str(tmp_path / "phasor_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "openmm-velocityverlet_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "phasor_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout.split()
    state, mask = 88172645463325252, (1 << 64) - 1
    phi = []
    for _ in range(1 << 20):
        state ^= (state << 13) & mask
        state ^= state >> 7
        state ^= (state << 17) & mask
        phi.append(state >> 32)
    phi = np.concatenate([np.array(phi, dtype=np.uint64), _edges()])
    assert int(out[0]) == phi.size
    assert int(out[1], 16) == _digest(phi)


# ------------------------------------------------------------------------------------------ exact cases
def test_simple_cubic_lattice_is_exact():
    """8 x 8 x 8 sites at dyadic fractions of the box, w = 1: a mode whose components are all multiples of 8 has A = 512 2^30 and B = 0
    exactly; every other mode has A = B = 0 exactly -- the phases come in pairs half a turn apart and the quadrant select negates
    exactly."""
    X, box = lattice_positions(), np.array(LATTICE_BOX)
    frac = np.stack(np.meshgrid(np.arange(8) / 8.0, np.arange(8) / 8.0, np.arange(8) / 8.0, indexing="ij"), axis=-1).reshape(-1, 3)
    assert np.array_equal(MR.turns(X, 1.0 / box), (frac * 2.0 ** 32).astype(np.uint64))      # (the box edges are powers of two: nothing rounds)
    A, B, bad = MR.sample_sums(X, box, np.ones(512), None, 1, LATTICE_MODES, 30)
    bragg = np.all(LATTICE_MODES % 8 == 0, axis=1)
    assert bad == 0 and bragg.sum() == 5 and (~bragg).sum() == 9
    assert np.array_equal(A[0], np.where(bragg, 512 << 30, 0)) and not B.any()


LATTICE_BOX = (2.0, 4.0, 0.5)
LATTICE_MODES = np.array([(0, 0, 0), (8, 0, 0), (0, -8, 16), (8, 8, 8), (4088, -4088, 8), (1, 0, 0), (3, 5, -7), (4, 4, 4), (0, 0, 12), (4095, -4095, 1),
                          (7, 8, 8), (2, 2, 2), (-1, -1, -1), (8, 8, 9)])


def lattice_positions():
    """8 x 8 x 8 sites at i / 8 of LATTICE_BOX, shifted by whole boxes (unwrapped positions): float64 [512, 3]."""
    i = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3)
    return (i / 8.0 + (i.sum(axis=1) % 5 - 2)[:, None]) * np.array(LATTICE_BOX)


def _turn_by_hand(x, inv_l):
    t = x * inv_l
    u = t - math.floor(t)
    return int(math.floor(u * 4294967296.0)) & 0xFFFFFFFF


WRAP_BOX = (2.5, 3.1, 4.7)


def wrap_positions():
    """Components -1e-20, exactly L, L (1 - 2^-53), +-5 L + x, one per row, on every axis."""
    rows = []
    for a, L in enumerate(WRAP_BOX):
        for v in (-1e-20, L, L * (1.0 - 2.0 ** -53), 5.0 * L + 0.3, -5.0 * L + 0.3, 0.0, -0.0, L / 3.0, -L / 3.0):
            x = [0.1, 0.2, 0.3]
            x[a] = v
            rows.append(x)
    return np.array(rows, dtype=np.float64)


WRAP_MODES = np.array([(4095, 4095, 4095), (-4095, -4095, -4095), (4095, -4095, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 2, -3), (0, 0, 0)])


def test_wrap_cases_equal_python_integers():
    X, box = wrap_positions(), np.array(WRAP_BOX)
    inv_L = 1.0 / box
    T = MR.turns(X, inv_L)
    by_hand = np.array([[_turn_by_hand(float(X[i, a]), float(inv_L[a])) for a in range(3)] for i in range(len(X))], dtype=np.uint64)
    assert np.array_equal(T, by_hand)
    assert T[0, 0] == 0                                               # -1e-20: u = 1.0 becomes 2^32 and wraps to 0
    assert T[1, 0] == 0                                               # exactly L
    assert T[2, 0] in (0, (1 << 32) - 1)                              # L (1 - 2^-53): whatever the product rounds to, not out of range
    phi = MR.phases(WRAP_MODES, T)
    for i in range(len(X)):
        for k, n in enumerate(WRAP_MODES):
            assert int(phi[i, k]) == sum(int(n[a]) * int(T[i, a]) for a in range(3)) % (1 << 32)
    # +-5 L + x is x's phase up to the rounding of the product: within 2^-20 turns here (|t| ~ 5: 3 bits above u's)
    d = (T[3, 0].astype(np.int64) - T[4, 0].astype(np.int64)) % (1 << 32)
    assert min(d, (1 << 32) - d) < 1 << 12


def test_ideal_gas_structure_factor_is_one():
    """Fixed seed: 4 096 (mode, sample) cells of |rho|^2 / N for N = 2 000 uniform sites.  Each cell is exponentially distributed with
    mean and standard deviation 1 (up to 1 / N), so the mean of 4 096 is within 5 / sqrt(4096) of 1."""
    rng = np.random.default_rng(7)
    box = np.array([4.0, 4.5, 5.0])
    N, K, J = 2000, 64, 64
    modes = _I().modes_in_shells(box, 12.0, max_per_shell=2, seed=1)[:K]
    assert len(modes) == K
    cells = []
    for _ in range(J):
        X = rng.uniform(-2.0, 2.0, size=(N, 3)) * box
        A, B, bad = MR.sample_sums(X, box, np.ones(N), None, 1, modes, 30)
        a, b = A[0].astype(np.float64) * 2.0 ** -30, B[0].astype(np.float64) * 2.0 ** -30
        cells.append((a * a + b * b) / N)
    cells = np.concatenate(cells)
    assert cells.size == 4096 and abs(cells.mean() - 1.0) <= 5.0 / math.sqrt(4096.0), cells.mean()
    assert abs(cells.std() - 1.0) < 0.15


def test_correlate_against_a_plain_loop():
    """The ring and the table of the reference against the statement, one scalar at a time."""
    rng = np.random.default_rng(3)
    G, K, J, F = 2, 3, 11, 28
    sums = [(rng.integers(-2 ** 33, 2 ** 33, size=(G, K)), rng.integers(-2 ** 33, 2 ** 33, size=(G, K)), 1 if j in (4, 6) else 0) for j in range(J)]
    boxes = rng.uniform(2.0, 3.0, size=(J, 3))
    for num_lags, E in [(0, 1), (5, 2), (4, 1), (4, 4)]:
        floors = [0] * 8 + [7] * 3
        got = MR.correlate(sums, boxes, G, K, num_lags, E, F, floors)
        count = [0] * (num_lags + 1)
        cell = np.zeros((num_lags + 1, G, G, K))
        for j, (A, B, bad) in enumerate(sums):
            if bad:
                continue
            for l in range(num_lags + 1):
                o = j - l
                if l and (o < 0 or o % E or o < floors[j] or sums[o][2]):
                    continue
                count[l] += 1
                for g in range(G):
                    for h in range(G):
                        for k in range(K):
                            cell[l, g, h, k] += (float(sums[o][0][g, k]) * 2.0 ** -F) * (float(A[h, k]) * 2.0 ** -F) + \
                                                (float(sums[o][1][g, k]) * 2.0 ** -F) * (float(B[h, k]) * 2.0 ** -F)
        assert list(got["words"][:, 0]) == count
        assert np.array_equal(got["words"][:, 1:], cell.reshape(num_lags + 1, -1).view(np.int64))
        assert (got["out_of_range"], got["invalid_samples"]) == (2, 2)
    clean = [(A, B, 0) for A, B, _ in sums]
    assert np.array_equal(MR.correlate(clean, boxes, G, K, 5, 2, F)["words"][:, 0], MR.lag_counts(J, 2, 5))


# ------------------------------------------------------------------------------------------ the ABI on an unbound plan
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


ONE_MODE = np.array([[1, 0, 0]], dtype=np.int32)


def _describe(plan, interval=10, num_lags=8, origin_every=1, num_groups=1, weight="ones", group=None, modes=ONE_MODE, num_modes=None, max_samples=1000,
              limit_position=0.0):
    """vvhip_modes_start on an unbound plan: (return code, error text); a description that passes the checks in front of the bind is kept."""
    H = _I().H
    n = _spec().num_atoms
    w = np.ones(n) if isinstance(weight, str) else (None if weight is None else np.ascontiguousarray(weight, dtype=np.float64))
    grp = None if group is None else np.ascontiguousarray(group, dtype=np.int8)
    m = None if modes is None else np.ascontiguousarray(modes, dtype=np.int32).reshape(-1, 3)
    K = num_modes if num_modes is not None else (1 if m is None else m.shape[0])
    desc = H.ModesDesc(interval, num_lags, origin_every, num_groups, K, None if w is None else w.ctypes.data, None if grp is None else grp.ctypes.data,
                       None if m is None else m.ctypes.data, max_samples, limit_position)
    rc = H.lib.vvhip_modes_start(plan, C.byref(desc))
    return rc, H.lib.vvhip_last_error(plan).decode()


def _info(plan):
    H = _I().H
    lay = H.ModesLayout()
    assert H.lib.vvhip_modes_info(plan, C.byref(lay)) == H.OK
    return lay


def test_modes_entry_points_and_struct_sizes():
    H = _I().H
    for name in ENTRY_POINTS:
        assert name in H.EXPORTS and hasattr(H.lib, name)
    header = open(os.path.join(ROOT, "include", "vvhip.h")).read()
    for name in ENTRY_POINTS:
        assert "int %s(" % name in header
    assert C.sizeof(H.ModesDesc) == 64 and C.sizeof(H.ModesCounts) == 64 and C.sizeof(H.ModesLayout) == 144


def test_kept_description_of_an_unbound_plan():
    H = _I().H
    n = _spec().num_atoms
    plan, keep = _plan()
    try:
        lay = _info(plan)
        assert (lay.active, lay.words, lay.num_modes) == (0, 0, 0)
        third = (np.arange(n) % 3).astype(np.int8) - 1                # -1, 0, 1
        modes = np.array([(0, 0, 0), (1, 2, 3), (-1, -2, -3), (4095, -4095, 1), (7, 0, 0)], dtype=np.int32)
        for group, G, wscale, num_lags, E, limit in [(None, 1, 1.0, 9, 4, 0.0), (third, 2, 0.3, 0, 1, 100.0), (third, 2, 2.0 ** -30, 7, 7, 0.0), (None, 1, 0.0, 1, 1, 2.0),
                                                     (None, 1, 2.0 ** 22 - 1, 3, 2, 0.0)]:
            w = wscale * np.linspace(-1.0, 0.5, n)
            w[0] = -wscale
            rc, text = _describe(plan, interval=7, num_lags=num_lags, origin_every=E, num_groups=G, weight=w, group=group, modes=modes, max_samples=123,
                                 limit_position=limit)
            assert rc == H.ERR_INVALID and "vvhip_bind has not been called" in text, text
            lay = _info(plan)
            sites = [n] if group is None else [int(np.count_nonzero(group == g)) for g in range(G)]
            W = MR.weight_bound(w, group)
            R_ = -(-num_lags // E) if num_lags else 0
            assert (lay.active, lay.interval, lay.num_lags, lay.origin_every, lay.num_groups, lay.num_modes, lay.max_samples) == (0, 7, num_lags, E, G, 5, 123)
            assert (lay.num_particles, lay.num_origins, lay.weight_bound, lay.frac_bits) == (sum(sites), R_, W, MR.frac_bits(W))
            assert list(lay.group_sites)[:G] == sites and not any(list(lay.group_sites)[G:])
            assert lay.row_words == MR.row_words(G, 5) and lay.words == (num_lags + 1) * MR.row_words(G, 5)
            assert lay.ring_bytes == R_ * (G * 5 * 2 + 1) * 8 and lay.scratch_bytes == 3 * 4 * ((sum(sites) + 15) // 16 * 16)
            assert lay.limit_position == (64.0 if limit == 0 else 2.0 ** math.ceil(math.log2(limit)))
            assert lay.sites_per_thread in (1, 2, 4, 8) and 1 <= lay.k_tile <= 1024 and lay.block_threads == 256
            per_item = lay.sites_per_thread * lay.block_threads
            assert lay.num_items == sum(-(-s // per_item) for s in sites) * -(-5 // lay.k_tile)
        assert H.lib.vvhip_modes_stop(plan) == H.OK and _info(plan).words == 0
    finally:
        H.lib.vvhip_plan_destroy(plan)


def test_start_refuses_in_the_documented_order():
    H = _I().H
    n = _spec().num_atoms
    plan, keep = _plan()
    try:
        assert H.lib.vvhip_modes_start(plan, None) == H.ERR_INVALID and "null description" in H.lib.vvhip_last_error(plan).decode()
        bad_group = np.zeros(n, dtype=np.int8)
        bad_group[3] = 2
        bad_weight = np.ones(n)
        bad_weight[5] = np.inf
        bad_modes = np.array([(1, 0, 0), (0, 4096, 0)], dtype=np.int32)
        # every description carries all the later faults too: the first one in the documented order is the one reported
        later = dict(num_lags=-1, origin_every=0, num_groups=9, num_modes=0, max_samples=0, limit_position=-1.0, weight=None, modes=None)
        order = [("interval", dict(interval=0), "interval must be >= 1"),
                 ("num_lags", dict(num_lags=4097), "num_lags must be in [0, 4096]"),
                 ("origin_every", dict(num_lags=8, origin_every=9), "origin_every must be in [1, max(1, num_lags)]"),
                 ("num_groups", dict(num_groups=0), "num_groups must be in [1, 8]"),
                 ("num_modes", dict(num_modes=4097), "num_modes must be in [1, 4096]"),
                 ("max_samples", dict(max_samples=0), "max_samples must be >= 1"),
                 ("limit_position", dict(limit_position=float("inf")), "limit_position must be finite and >= 0"),
                 ("weight", dict(weight=None), "weight must not be NULL"),
                 ("modes", dict(modes=None, num_modes=1), "modes must not be NULL")]
        names = [k for k, _, _ in order]
        for pos, (name, fault, text) in enumerate(order):
            kw = {k: v for k, v in later.items() if k in names[pos + 1:]}
            kw.update(fault)
            rc, err = _describe(plan, **kw)
            assert rc == H.ERR_INVALID and text in err, (name, err)
        assert "origin_every must be in" in _describe(plan, num_lags=0, origin_every=2)[1]
        # a mode component, then a group entry, then a weight that is not finite, then the fixed point, then the table, then the bind
        big = 2.0 ** 23 * np.ones(n)
        rc, err = _describe(plan, num_groups=2, modes=bad_modes, group=bad_group, weight=bad_weight)
        assert rc == H.ERR_INVALID and "modes[1][1] = 4096 is outside [-4095, 4095]" in err
        assert "modes[0][2] = -4096 is outside" in _describe(plan, modes=np.array([(0, 0, -4096)]))[1]
        rc, err = _describe(plan, num_groups=2, group=bad_group, weight=bad_weight)
        assert rc == H.ERR_INVALID and "group[3] = 2 is outside [-1, num_groups = 2)" in err
        rc, err = _describe(plan, weight=bad_weight)
        assert rc == H.ERR_INVALID and "weight[5] is not finite" in err
        wide = np.zeros((4096, 3), dtype=np.int32)
        rc, err = _describe(plan, weight=big, num_groups=8, modes=wide, num_lags=255)
        assert rc == H.ERR_INVALID and "would keep 6 fraction bits (< 8)" in err
        assert _info(plan).words == 0                                # nothing of a refused description is kept
        rc, err = _describe(plan, weight=big / 4)                    # W = 2^22: F = 8, the last that passes
        assert "vvhip_bind has not been called" in err and _info(plan).frac_bits == 8
        assert "would keep 7 fraction bits" in _describe(plan, weight=big / 2)[1]
        # the table's cap of 2^26 words: 8 groups and 4096 modes are rows of 262 145 words
        rc, err = _describe(plan, num_groups=8, modes=wide, num_lags=255)
        assert rc == H.ERR_INVALID and "67109120 words" in err and "above 2^26" in err
        rc, err = _describe(plan, num_groups=8, modes=wide, num_lags=254, origin_every=254)
        assert "vvhip_bind has not been called" in err and _info(plan).words == 255 * 262145
        assert H.lib.vvhip_modes_read(plan, None, 0, None, 0) == H.ERR_INVALID
    finally:
        H.lib.vvhip_plan_destroy(plan)


def test_a_sharded_plan_is_refused():
    H = _I().H
    n = _spec().num_atoms
    mol = np.asarray(_spec().mol_id)
    cut = int(np.nonzero(mol == mol[n // 2])[0].min())                # a molecule boundary
    assert 0 < cut < n
    for shard in ((0, cut), (cut, n)):
        plan, keep = _plan(shard=shard)
        try:
            rc, err = _describe(plan, weight=2.0 ** 23 * np.ones(n))  # the fixed point goes first
            assert rc == H.ERR_INVALID and "fraction bits" in err
            rc, err = _describe(plan)
            assert rc == H.ERR_UNSUPPORTED and "shard" in err and "before the products" in err
            assert _info(plan).words == 0 and _info(plan).active == 0
        finally:
            H.lib.vvhip_plan_destroy(plan)


# ------------------------------------------------------------------------------------------ the views, the helper, the writer
def _hand_made(G, modes, num_lags, interval, count, mean, sites, samples, box_sum, invalid=0):
    """A DensityModes from MEANS [L + 1, G, G, K] of rho_g* rho_h: the table holds mean * count."""
    I = _I()
    count = np.asarray(count, dtype=np.int64)
    K = len(modes)
    words = np.zeros((num_lags + 1, MR.row_words(G, K)), dtype=np.int64)
    words[:, 0] = count
    words[:, 1:] = (np.asarray(mean, dtype=np.float64) * count[:, None, None, None]).reshape(num_lags + 1, -1).view(np.int64)
    return I.DensityModes(samples=samples, dropped=0, out_of_range=0, invalid_samples=invalid, origin_floor=0, box_sum=np.asarray(box_sum, dtype=np.float64),
                          interval=interval, origin_every=1, num_groups=G, frac_bits=30, group_sites=np.asarray(sites, dtype=np.int64),
                          modes=np.asarray(modes, dtype=np.int32), words=words)


def test_views_on_a_hand_made_table():
    modes = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (2, 0, 0)]
    G, L = 2, 4
    sites = [100, 400]
    tau = 20.0                                                        # steps
    t = np.arange(L + 1) * 5.0
    S0 = np.array([[[1.0, 2.0, 3.0, 4.0, 8.0], [0.5] * 5], [[0.5] * 5, [2.0, 2.0, 2.0, 1.0, 1.0]]])      # [g][h][k], already / sqrt(N_g N_h)
    norm = np.sqrt(np.outer(sites, sites))[:, :, None]
    mean = (S0 * norm)[None] * np.exp(-t / tau)[:, None, None, None]
    dm = _hand_made(G, modes, L, 5, [10, 9, 8, 7, 0], mean, sites, samples=12, box_sum=[20.0, 30.0, 40.0], invalid=2)
    assert dm.num_modes == 5 and list(dm.lag_steps) == [0, 5, 10, 15, 20] and list(dm.count) == [10, 9, 8, 7, 0]
    assert np.allclose(dm.mean_box, [2.0, 3.0, 4.0], rtol=0, atol=0)
    assert np.allclose(dm.S(0, 0), S0[0, 0], rtol=1e-15) and np.allclose(dm.S(1, 0), S0[1, 0], rtol=1e-15) and np.allclose(dm.S(1, 1), S0[1, 1], rtol=1e-15)
    F = dm.F(0, 0)
    assert F.shape == (5, 5) and np.all(np.isnan(F[4])) and np.allclose(F[:4], S0[0, 0][None] * np.exp(-t[:4] / tau)[:, None], rtol=1e-14)
    k = dm.k_magnitudes()
    assert np.allclose(k, 2 * np.pi * np.array([1 / 2.0, 1 / 3.0, 1 / 4.0, math.hypot(1 / 2.0, 1 / 3.0), 2 / 2.0]), rtol=1e-15)
    assert list(dm.shells()) == [0, 0, 0, 1, 2]
    ks, av = dm.shell_average(dm.S(0, 0))
    assert np.allclose(ks, [k[:3].mean(), k[3], k[4]], rtol=1e-15) and np.allclose(av, [2.0, 4.0, 8.0], rtol=1e-15)
    with pytest.raises(ValueError):
        dm.S(0, 2)
    # F / S = exp(-t / tau) sampled every 5 steps: 1 / e is reached at t = tau = 20, outside the rows with origins -> a steeper decay
    fast = (S0 * norm)[None] * np.exp(-t / 7.0)[:, None, None, None]
    dq = _hand_made(G, modes, L, 5, [10, 9, 8, 7, 6], fast, sites, samples=10, box_sum=[20.0, 30.0, 40.0])
    y = np.exp(-t / 7.0)
    want = 5.0 + 5.0 * (y[1] - math.exp(-1.0)) / (y[1] - y[2])        # between rows 1 and 2
    assert dq.relaxation_time(0, 0) == pytest.approx(want, rel=1e-12) and dq.relaxation_time(1, 2, dt=0.002) == pytest.approx(want * 0.002, rel=1e-12)
    slow = _hand_made(G, modes, L, 5, [10, 9, 8, 7, 6], (S0 * norm)[None] * np.exp(-t / 1e3)[:, None, None, None], sites, samples=10, box_sum=[20.0, 30.0, 40.0])
    assert math.isnan(slow.relaxation_time(0, 0))


def test_modes_in_shells():
    I = _I()
    box = (3.0, 3.0, 4.5)
    m = I.modes_in_shells(box, 9.0)
    assert m.dtype == np.int32 and m.ndim == 2 and m.shape[1] == 3 and len(m) > 20
    as_set = set(map(tuple, m.tolist()))
    assert len(as_set) == len(m) and (0, 0, 0) not in as_set
    assert all((-a, -b, -c) not in as_set for a, b, c in as_set)      # never both n and -n
    n2 = (m.astype(np.int64) ** 2).sum(axis=1)
    assert np.all(np.diff(n2) >= 0)                                   # sorted by |n|^2
    k = 2 * np.pi * np.sqrt(((m / np.array(box)) ** 2).sum(axis=1))
    assert k.max() <= 9.0
    # complete: every triple within k_max is there, itself or its negative
    top = 5
    for a in range(-top, top + 1):
        for b in range(-top, top + 1):
            for c in range(-top - 2, top + 3):
                inside = (a, b, c) != (0, 0, 0) and 2 * math.pi * math.sqrt((a / 3.0) ** 2 + (b / 3.0) ** 2 + (c / 4.5) ** 2) <= 9.0
                assert inside == ((a, b, c) in as_set or (-a, -b, -c) in as_set), (a, b, c)
    thin = I.modes_in_shells(box, 9.0, max_per_shell=3, seed=5)
    t2 = (thin.astype(np.int64) ** 2).sum(axis=1)
    assert set(map(tuple, thin.tolist())) <= as_set and np.all(np.diff(t2) >= 0) and np.bincount(t2).max() == 3
    assert set(np.unique(t2)) == set(np.unique(n2))
    assert np.array_equal(thin, I.modes_in_shells(box, 9.0, max_per_shell=3, seed=5))
    assert not np.array_equal(thin, I.modes_in_shells(box, 9.0, max_per_shell=3, seed=6))
    with pytest.raises(ValueError):
        I.modes_in_shells((3.0, 3.0, 3.0), 1e5)


def test_write_modes_round_trips():
    modes = [(1, 0, 0), (0, 1, 0), (1, 1, 1)]
    rng = np.random.default_rng(11)
    mean = rng.uniform(0.1, 3.0, size=(3, 1, 1, 3))
    dm = _hand_made(1, modes, 2, 4, [6, 5, 0], mean, [50], samples=6, box_sum=[12.0, 15.0, 18.0])
    buf = io.StringIO()
    R.write_modes(buf, dm, 0.002)
    text = buf.getvalue()
    lines = text.splitlines()
    assert lines[0].startswith('#"Samples"\t6\t"Dropped"\t0') and '"BoxSum"\t12.0\t15.0\t18.0' in lines[0]
    assert lines[1] == '#"nx"\t"ny"\t"nz"\t"k (1/nm)"\t"S[0-0]"\t"F[0-0](0.008 ps)"\t"F[0-0](0.016 ps)"'
    back = np.loadtxt(io.StringIO(text), ndmin=2)
    assert back.shape == (3, 7) and np.array_equal(back[:, :3], np.array(modes, dtype=float))
    assert np.array_equal(back[:, 3], dm.k_magnitudes()) and np.array_equal(back[:, 4], dm.S()) and np.array_equal(back[:, 5], dm.F()[1])
    assert np.all(np.isnan(back[:, 6]))
