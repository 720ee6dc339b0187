"""The statement of the device-side MSD recorder (include/vvhip.h: vvhip_msd_*) in NumPy, float64 without contraction: units from
positions, the (sample, origin, row) pairs of a list of samples, the fixed-point table and the out-of-range count.  Imported by
tests/test_msd.py (against a plain loop) and tests/test_gpu_msd.py (against the device's table, fed with float64 frames)."""
import numpy as np

DEFAULT_LIMIT = 64.0


def ceil_log2(n):
    """Smallest k with 2^k >= n (n >= 1)."""
    return int(n - 1).bit_length()


def pow2_at_least(x):
    m, e = np.frexp(float(x))
    return float(x) if m == 0.5 else float(np.ldexp(1.0, e))


def applied_limit(limit):
    return pow2_at_least(limit) if limit > 0 else DEFAULT_LIMIT


def num_origins(num_lags, origin_every):
    return -(-num_lags // origin_every)


def frac_bits(units_whole_system, max_samples, origin_every, limit):
    """F of the statement; `limit` as given to the recorder (0: the default)."""
    lim = applied_limit(limit)
    return min(40, 62 - ceil_log2(units_whole_system + 1) - ceil_log2(-(-max_samples // origin_every) + 1) - 2 * int(np.log2(lim)))


def molecule_units(masses, mol_id, groups=None):
    """The molecule units of a System: [(molecule id, group, members ascending)] for every molecule with a massive particle whose group is
    >= 0, by ascending molecule id.  A molecule whose massive particles lie in different groups raises ValueError."""
    masses, mol_id = np.asarray(masses, dtype=np.float64), np.asarray(mol_id)
    out = []
    massive = np.nonzero(masses > 0)[0]
    order = massive[np.argsort(mol_id[massive], kind="stable")]      # by molecule, ascending particle index inside one
    starts = np.nonzero(np.diff(mol_id[order], prepend=-1))[0] if order.size else []
    for mem in np.split(order, starts[1:]) if order.size else []:
        m = mol_id[mem[0]]
        g = np.zeros(mem.size, dtype=int) if groups is None else np.asarray(groups)[mem].astype(int)
        if np.any(g != g[0]):
            raise ValueError(f"molecule {int(m)} has massive particles in different groups")
        if g[0] >= 0:
            out.append((int(m), int(g[0]), mem))
    return out


def unit_positions(x, masses=None, mol_id=None, groups=None, molecules=False, units=None):
    """(c float64 [U, 3], g int [U]) of one sample: x float64 [n, 3], the positions as a float64 frame holds them.  Particles: the
    recorded ones (group >= 0) in ascending index.  Molecules: the centre of mass by the SEQUENTIAL sum in ascending particle index,
    s = s + m_i * X_i, c = s / M with M summed in the same order -- vectorised across the molecules over the k-th member.  `units`:
    molecule_units of the same arguments, where the caller has them already."""
    x = np.asarray(x, dtype=np.float64)
    if not molecules:
        g = np.zeros(len(x), dtype=int) if groups is None else np.asarray(groups).astype(int)
        keep = g >= 0
        return x[keep].copy(), g[keep]
    units = molecule_units(masses, mol_id, groups) if units is None else units
    masses = np.asarray(masses, dtype=np.float64)
    count = np.array([len(mem) for _, _, mem in units])
    s, total = np.zeros((len(units), 3)), np.zeros(len(units))
    for k in range(int(count.max()) if len(units) else 0):
        has = np.nonzero(count > k)[0]
        i = np.array([units[u][2][k] for u in has])
        s[has] = s[has] + masses[i][:, None] * x[i]
        total[has] = total[has] + masses[i]
    return s / total[:, None], np.array([g for _, g, _ in units], dtype=int)


def pairs(num_samples, origin_every, num_lags, floor=0):
    """[(j, origin ordinal, row)] of samples 0 .. num_samples - 1: at sample j every origin k E with floor_j <= k E < j and
    j - k E <= num_lags contributes to row j - k E - 1.  `floor`: one ordinal, or one per sample (the floor as it stood at that sample)."""
    floors = np.broadcast_to(np.asarray(floor, dtype=np.int64), (num_samples,))
    out = []
    for j in range(num_samples):
        for o in range(0, j, origin_every):
            if o >= floors[j] and j - o <= num_lags:
                out.append((j, o, j - o - 1))
    return out


def pair_counts(num_samples, origin_every, num_lags):
    """Closed form: pairs per row per unit after num_samples samples (floor 0).  Row l pairs sample j = k E + l + 1 with origin k E:
    the k >= 0 with k E + l + 1 <= num_samples - 1."""
    l = np.arange(num_lags)
    return np.maximum(0, (num_samples - 2 - l) // origin_every + 1).astype(np.int64)


def msd_reference(c, g, num_groups, num_lags, origin_every, frac, limit, floor=0):
    """(table int64 [num_groups, num_lags, 4], out_of_range) of the samples c float64 [J, U, 3] (unit_positions of every sample, ordinal 0
    first) with the units' groups g [U].  `limit`: as applied (a power of two)."""
    c = np.asarray(c, dtype=np.float64)
    g = np.asarray(g, dtype=int)
    table, out = np.zeros((num_groups, num_lags, 4), dtype=np.int64), 0
    scale = 2.0 ** frac
    for j, o, row in pairs(len(c), origin_every, num_lags, floor):
        d = c[j] - c[o]
        ok = np.all(np.abs(d) < limit, axis=1)                     # (False for a NaN)
        out += int(np.count_nonzero(~ok))
        w = np.rint(d * d * scale)                                 # round-half-even, as llrint
        for k in range(num_groups):
            take = ok & (g == k)
            table[k, row, 0] += int(np.count_nonzero(take))
            table[k, row, 1:] += w[take].astype(np.int64).sum(axis=0)
    return table, out
