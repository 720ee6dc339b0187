"""The statement of the device-side self van Hove recorder (include/vvhip.h: vvhip_vanhove_*) in NumPy, float64 without contraction: the
(sample, origin, row) pairs and the units are the MSD recorder's (tests/msd_reference.py), the bins are decided by comparisons against the
squared edges, the moments are fixed-point integers with r2 r2 in two words.  Imported by tests/test_vanhove.py (against a plain loop) and
tests/test_gpu_vanhove.py (against the device's table, fed with float64 frames)."""
import numpy as np

from msd_reference import ceil_log2, molecule_units, num_origins, pair_counts, pairs, pow2_at_least, unit_positions      # noqa: F401

DEFAULT_LIMIT = 16.0
MAX_WORDS = 1 << 22
PAIRS, BELOW, BEYOND, R2, R4_HI, R4_LO, ROW = 0, 1, 2, 3, 4, 5, 6


def applied_limit(limit):
    return pow2_at_least(limit) if limit > 0 else DEFAULT_LIMIT


def exponents(units_whole_system, max_samples, origin_every, limit):
    """(frac2, fh, d) of the statement; `limit` as given to the recorder (0: the default)."""
    lg = int(np.log2(applied_limit(limit)))
    s = ceil_log2(units_whole_system + 1) + ceil_log2(-(-max_samples // origin_every) + 1)
    return min(40, 62 - s - 2 * lg - 2), min(40, 62 - s - 4 * lg - 4), min(52, 61 - s)


def squared_edges(edges):
    e = np.asarray(edges, dtype=np.float64)
    return e * e


def bins_of(r2, e2):
    """int [..]: b with e2[b] <= r2 < e2[b + 1] -- -1 below e2[0], len(e2) - 1 at or beyond the last edge -- by comparisons alone: the
    number of edges at or below r2, minus one."""
    return (np.asarray(r2)[..., None] >= e2).sum(axis=-1) - 1


def r4_words(r2, fh, d):
    """(hi, lo) int64 of r2 * r2: x = (r2 * r2) * 2^fh, hi = floor(x), lo = rint((x - hi) * 2^d); every step exact or correctly rounded."""
    x = (r2 * r2) * 2.0 ** fh
    hi = np.floor(x)
    return hi.astype(np.int64), np.rint((x - hi) * 2.0 ** d).astype(np.int64)


def r4_value(hi, lo, fh, d):
    return (np.asarray(hi, dtype=np.float64) + np.asarray(lo, dtype=np.float64) * 2.0 ** -d) * 2.0 ** -fh


def vanhove_reference(c, g, num_groups, num_lags, origin_every, edges, exps, limit, floor=0):
    """(head int64 [num_groups, num_lags, 6], hist int64 [num_groups, num_lags, bins], out_of_range) of the samples c float64 [J, U, 3]
    (unit_positions of every sample, ordinal 0 first) with the units' groups g [U].  `exps`: (frac2, fh, d); `limit`: as applied."""
    c = np.asarray(c, dtype=np.float64)
    g = np.asarray(g, dtype=int)
    e2 = squared_edges(edges)
    B = len(e2) - 1
    frac2, fh, d = exps
    head = np.zeros((num_groups, num_lags, ROW), dtype=np.int64)
    hist = np.zeros((num_groups, num_lags, B), dtype=np.int64)
    out = 0
    for j, o, row in pairs(len(c), origin_every, num_lags, floor):
        dl = c[j] - c[o]
        ok = np.all(np.abs(dl) < limit, axis=1)                    # (False for a NaN)
        out += int(np.count_nonzero(~ok))
        dl = np.where(ok[:, None], dl, 0.0)
        r2 = (dl[:, 0] * dl[:, 0] + dl[:, 1] * dl[:, 1]) + dl[:, 2] * dl[:, 2]
        b = bins_of(r2, e2)
        w2 = np.rint(r2 * 2.0 ** frac2).astype(np.int64)           # round-half-even, as llrint
        hi, lo = r4_words(r2, fh, d)
        for k in range(num_groups):
            take = ok & (g == k)
            head[k, row, PAIRS] += int(np.count_nonzero(take))
            head[k, row, BELOW] += int(np.count_nonzero(take & (b < 0)))
            head[k, row, BEYOND] += int(np.count_nonzero(take & (b >= B)))
            head[k, row, R2] += w2[take].sum()
            head[k, row, R4_HI] += hi[take].sum()
            head[k, row, R4_LO] += lo[take].sum()
            inside = take & (b >= 0) & (b < B)
            hist[k, row] += np.bincount(b[inside], minlength=B).astype(np.int64)
    return head, hist, out
