"""The statement of the device-side current recorder (include/vvhip.h: vvhip_current_*) in NumPy, float64 without contraction: the
fixed-point sums of a sample, the ring of origins, and the table whose cells are sequential float64 sums in ascending sample order.
Imported by tests/test_current.py (against a plain loop) and tests/test_gpu_current.py (against the device's table, fed with float64
frames)."""
import numpy as np

DEFAULT_LIMIT = 64.0


def ceil_log2(n):
    """Smallest k with 2^k >= n (n >= 1)."""
    return int(n - 1).bit_length()


def pow2_at_least(x):
    m, e = np.frexp(float(x))
    return float(x) if m == 0.5 else float(np.ldexp(1.0, e))


def pow2_above(x):
    """The smallest power of two above x > 0; 1 for x == 0."""
    _, e = np.frexp(float(x))
    return float(np.ldexp(1.0, e)) if x > 0 else 1.0


def applied_limit(limit):
    return pow2_at_least(limit) if limit > 0 else DEFAULT_LIMIT


def weight_bound(weights, groups=None):
    """W: the smallest power of two above max |w_i| over the recorded particles."""
    w = np.abs(np.asarray(weights, dtype=np.float64))
    if groups is not None:
        w = w[np.asarray(groups) >= 0]
    return pow2_above(w.max()) if w.size else 1.0


def frac_bits(num_recorded, W, limit):
    """Fp or Fv of the statement; `limit` as given to the recorder (0: the default)."""
    return min(40, 62 - ceil_log2(num_recorded + 1) - int(np.log2(W)) - int(np.log2(applied_limit(limit))))


def num_origins(num_lags, origin_every):
    return -(-num_lags // origin_every)


def num_classes(G):
    """(ND, NC)"""
    return G * (G + 1) // 2, G * G


def disp_class(g, h, G):
    """c(g, h), g <= h: (0,0) (0,1) .. (0,G-1) (1,1) .."""
    assert 0 <= g <= h < G
    return g * G - g * (g - 1) // 2 + (h - g)


def row_words(G):
    nd, nc = num_classes(G)
    return 1 + 3 * (nd + nc)


def molecule_weights(charges, masses, mol_id):
    """Q_m m_i / M_m with Q_m and M_m summed in ascending particle index, one scalar at a time; massless particles get 0."""
    q, m, mol = np.asarray(charges, dtype=np.float64), np.asarray(masses, dtype=np.float64), np.asarray(mol_id)
    Q, M = {}, {}
    for i in range(len(q)):
        Q[mol[i]] = Q.get(mol[i], 0.0) + q[i]
        M[mol[i]] = M.get(mol[i], 0.0) + m[i]
    return np.array([Q[mol[i]] * m[i] / M[mol[i]] if m[i] > 0 and M[mol[i]] > 0 else 0.0 for i in range(len(q))])


def sample_sums(x, v, weights, groups, G, Fp, Fv, limit_p, limit_v):
    """(S int64 [G, 6]: P_x P_y P_z U_x U_y U_z per group, out-of-range particles) of one sample: x, v float64 [n, 3] as a float64 frame
    holds them, the limits as applied."""
    x, v, w = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    g = np.zeros(len(x), dtype=int) if groups is None else np.asarray(groups).astype(int)
    rec = g >= 0
    ok = np.all(np.abs(x) < limit_p, axis=1) & np.all(np.abs(v) < limit_v, axis=1)      # (False for a NaN)
    bad = int(np.count_nonzero(rec & ~ok))
    S = np.zeros((G, 6), dtype=np.int64)
    take = rec & ok
    p = np.rint((w[take, None] * x[take]) * 2.0 ** Fp).astype(np.int64)                # round-half-even, as llrint
    u = np.rint((w[take, None] * v[take]) * 2.0 ** Fv).astype(np.int64)
    for k in range(G):
        sel = g[take] == k
        S[k, :3] = p[sel].sum(axis=0, dtype=np.int64)
        S[k, 3:] = u[sel].sum(axis=0, dtype=np.int64)
    return S, bad


def lag_counts(num_samples, origin_every, num_lags):
    """Closed form of count[0 .. num_lags] after num_samples valid samples with floor 0: row 0 every sample; row l >= 1 the k >= 0 with
    k E + l <= num_samples - 1 (tests/msd_reference.pair_counts, shifted by row 0)."""
    l = np.arange(1, num_lags + 1)
    rows = np.maximum(0, (num_samples - 1 - l) // origin_every + 1)
    return np.concatenate([[num_samples], rows]).astype(np.int64)


def correlate(sums, bad, G, num_lags, origin_every, Fp, Fv, floor=0, inv_volume=None):
    """The table of the samples' sums [J, G, 6] (ordinal 0 first) and out-of-range counts [J]:
    dict(words int64 [num_lags + 1, row_words], out_of_range, invalid_samples, inv_volume_sum).  `floor`: one ordinal, or one per sample
    (the floor as it stood at that sample); inv_volume: one 1 / V, or one per sample.  The ring is kept as the device keeps it."""
    sums = np.asarray(sums, dtype=np.int64)
    J = len(sums)
    floors = np.broadcast_to(np.asarray(floor, dtype=np.int64), (J,))
    inv_v = None if inv_volume is None else np.broadcast_to(np.asarray(inv_volume, dtype=np.float64), (J,))
    nd, nc = num_classes(G)
    R, E = num_origins(num_lags, origin_every), origin_every
    count = np.zeros(num_lags + 1, dtype=np.int64)
    disp, cur = np.zeros((num_lags + 1, nd, 3)), np.zeros((num_lags + 1, nc, 3))
    ring, hold = np.zeros((R, G, 6), dtype=np.int64), np.full(R, -1, dtype=np.int64)
    pairs = [(g, h) for g in range(G) for h in range(g, G)]
    dg, dh = np.array([g for g, _ in pairs]), np.array([h for _, h in pairs])
    cg, ch = np.repeat(np.arange(G), G), np.tile(np.arange(G), G)
    sp, sv = 2.0 ** -Fp, 2.0 ** -Fv
    out, invalid, ivs = 0, 0, 0.0
    for j in range(J):
        valid = bad[j] == 0
        out += int(bad[j])
        if valid:
            Jn = sums[j, :, 3:].astype(np.float64) * sv
            cur[0] = cur[0] + Jn[cg] * Jn[ch]
            count[0] += 1
            for s in range(R):
                o = hold[s]
                l = j - o
                if o < 0 or o < floors[j] or l < 1 or l > num_lags:
                    continue
                dP = (sums[j, :, :3] - ring[s, :, :3]).astype(np.float64) * sp
                Jo = ring[s, :, 3:].astype(np.float64) * sv
                disp[l] = disp[l] + dP[dg] * dP[dh]
                cur[l] = cur[l] + Jo[cg] * Jn[ch]
                count[l] += 1
            if inv_v is not None:
                ivs = ivs + float(inv_v[j])
        else:
            invalid += 1
        if j % E == 0:                                               # accumulation first, the store second
            s = (j // E) % R
            if valid:
                ring[s], hold[s] = sums[j], j
            else:
                hold[s] = -1
    words = np.zeros((num_lags + 1, 1 + 3 * (nd + nc)), dtype=np.int64)
    words[:, 0] = count
    words[:, 1:1 + 3 * nd] = disp.reshape(num_lags + 1, -1).view(np.int64)
    words[:, 1 + 3 * nd:] = cur.reshape(num_lags + 1, -1).view(np.int64)
    return dict(words=words, out_of_range=out, invalid_samples=invalid, inv_volume_sum=ivs)


def current_reference(xs, vs, weights, groups, G, num_lags, origin_every, Fp, Fv, limit_p, limit_v, floor=0, inv_volume=None):
    """correlate() over the samples xs, vs float64 [J, n, 3]; the limits as applied."""
    per = [sample_sums(x, v, weights, groups, G, Fp, Fv, limit_p, limit_v) for x, v in zip(xs, vs)]
    sums = np.array([s for s, _ in per], dtype=np.int64).reshape(len(per), G, 6)
    return correlate(sums, np.array([b for _, b in per], dtype=np.int64), G, num_lags, origin_every, Fp, Fv, floor, inv_volume)
