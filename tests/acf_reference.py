"""The statement of the device-side autocorrelation recorder (include/vvhip.h: vvhip_acf_*) in NumPy, float64 without contraction: the
reciprocal norm of the unit vectors as the one sequence of +, -, * it is, the units' vectors of the three modes with NaN for a bad one,
the (sample, origin, row) pairs of a list of samples, the pair-count closed form, the fixed-point table and the out-of-range count.
Imported by tests/test_acf.py (against a plain loop) and tests/test_gpu_acf.py (against the device's table, fed with float64 frames)."""
import numpy as np

import msd_reference as MR

VELOCITY, MOLECULES, ORIENTATION = 0, 1, 2
DEFAULT_LIMIT = 64.0
N2_MIN, N2_MAX = 2.0 ** -40, 2.0 ** 40
UNIT_BOUND = 2.0 ** -49      # | |u|^2 - 1 | of every unit vector


def row_words(mode):
    return 5 if mode == ORIENTATION else 4


def applied_limit(mode, limit):
    if mode == ORIENTATION:
        return 1.0
    return MR.pow2_at_least(limit) if limit > 0 else DEFAULT_LIMIT


def frac_bits(units_whole_system, max_samples, origin_every, mode, limit=0.0):
    """F of the statement; `limit` as given to the recorder (0: the default)."""
    lim = applied_limit(mode, limit)
    return min(40, 62 - MR.ceil_log2(units_whole_system + 1) - MR.ceil_log2(-(-max_samples // origin_every) + 1) - 2 * int(np.log2(lim)))


def inverse_norm(n2):
    """y ~ n2^(-1/2) for normal positive n2, element-wise: csrc/vv_layout.h's acf_inverse_norm operation for operation.  With ex the
    exponent of n2 and e = ex - (ex & 1): m = n2 2^-e in [1, 4) by rewriting the exponent field; the chord of m^(-1/2) over [1, 2) or
    [2, 4) as the seed; four Newton steps, every * and - rounded on its own; then the exact scaling by 2^(-e/2)."""
    n2 = np.ascontiguousarray(n2, dtype=np.float64)
    bits = n2.view(np.uint64)
    e = ((bits >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
    odd = e & 1
    m = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | ((1023 + odd).astype(np.uint64) << np.uint64(52))).view(np.float64)
    h = (e - odd) // 2
    y = np.where(m < 2.0, 1.2929 - 0.2929 * m, 0.9142 - 0.10355 * m)
    hm = 0.5 * m
    for _ in range(4):
        y = y * (1.5 - hm * (y * y))
    return y * ((1023 - h).astype(np.uint64) << np.uint64(52)).view(np.float64)


def unit_vectors(d):
    """u float64 [n, 3] of d [n, 3]: d * y with n2 = (dx dx + dy dy) + dz dz; NaN rows where n2 is NaN or outside [2^-40, 2^40)."""
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    n2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    good = (n2 >= N2_MIN) & (n2 < N2_MAX)                             # (False for a NaN)
    y = inverse_norm(np.where(good, n2, 1.0))
    return np.where(good[:, None], d * y[:, None], np.nan)


def orientation_units(pairs, groups=None):
    """(heads, tails, g) of the recorded pairs (group >= 0) in the order given."""
    pairs = np.asarray(pairs, dtype=int).reshape(-1, 2)
    g = np.zeros(len(pairs), dtype=int) if groups is None else np.asarray(groups).astype(int)
    keep = g >= 0
    return pairs[keep, 0], pairs[keep, 1], g[keep]


def unit_vectors_of_sample(mode, limit, v=None, x=None, masses=None, mol_id=None, groups=None, pairs=None, units=None):
    """(a float64 [U, 3], g int [U]) of one sample, bad vectors NaN in all three components.  v, x: float64 [n, 3], the velocities and
    positions as a float64 frame holds them.  VELOCITY: the recorded particles' v.  MOLECULES: the centre-of-mass velocity by the
    SEQUENTIAL sum in ascending particle index (msd_reference.unit_positions with v for X).  ORIENTATION: unit_vectors of X_head -
    X_tail; `groups` has one entry per pair.  `limit`: as applied."""
    if mode == ORIENTATION:
        h, t, g = orientation_units(pairs, groups)
        x = np.asarray(x, dtype=np.float64)
        return unit_vectors(x[h] - x[t]), g
    a, g = MR.unit_positions(v, masses, mol_id, groups, mode == MOLECULES, units)
    good = np.all(np.abs(a) < limit, axis=1)                          # (False for a NaN)
    return np.where(good[:, None], a, np.nan), g


def pairs_of(num_samples, origin_every, num_lags, floor=0, max_samples=None):
    """[(j, origin ordinal, row)] of samples 0 .. num_samples - 1: at sample j every origin o = k E with floor_j <= o <= j and
    j - o < num_lags contributes to row j - o.  `floor`: one ordinal, or one per sample (the floor as it stood at that sample).  Samples
    at or past max_samples add nothing."""
    floors = np.broadcast_to(np.asarray(floor, dtype=np.int64), (num_samples,))
    out = []
    for j in range(num_samples if max_samples is None else min(num_samples, max_samples)):
        for o in range(0, j + 1, origin_every):
            if o >= floors[j] and j - o < num_lags:
                out.append((j, o, j - o))
    return out


def pair_counts(num_samples, origin_every, num_lags):
    """Closed form: pairs per row per unit after num_samples samples (floor 0).  Row l pairs sample j = k E + l with origin k E: the
    k >= 0 with k E + l <= num_samples - 1."""
    l = np.arange(num_lags)
    return np.maximum(0, (num_samples - 1 - l) // origin_every + 1).astype(np.int64) * (l <= num_samples - 1)


def acf_reference(a, g, num_groups, num_lags, origin_every, frac, mode, floor=0, max_samples=None):
    """(table int64 [num_groups, num_lags, row_words], out_of_range) of the samples a float64 [J, U, 3] (unit_vectors_of_sample of every
    sample, ordinal 0 first) with the units' groups g [U]."""
    a = np.asarray(a, dtype=np.float64)
    g = np.asarray(g, dtype=int)
    W = row_words(mode)
    table, out = np.zeros((num_groups, num_lags, W), dtype=np.int64), 0
    scale = 2.0 ** frac
    for j, o, row in pairs_of(len(a), origin_every, num_lags, floor, max_samples):
        ok = ~np.isnan(a[j, :, 0]) & ~np.isnan(a[o, :, 0])
        out += int(np.count_nonzero(~ok))
        p = np.where(ok[:, None], a[o] * a[j], 0.0)
        w = [np.rint(p[:, k] * scale) for k in range(3)]             # round-half-even, as llrint
        if W == 5:
            c = (p[:, 0] + p[:, 1]) + p[:, 2]
            w.append(np.rint(c * c * scale))
        for k in range(num_groups):
            take = ok & (g == k)
            table[k, row, 0] += int(np.count_nonzero(take))
            for q in range(W - 1):
                table[k, row, 1 + q] += int(w[q][take].astype(np.int64).sum())
    return table, out
