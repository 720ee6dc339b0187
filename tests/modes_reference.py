"""The definition of the density-mode recorder (include/vvhip.h: vvhip_modes_*) in NumPy and Python integers: turns, phase, phasor, terms,
sums, ring and table.  Only correctly rounded + - * on float64 and integer arithmetic occur, so this file states the device's words bit for
bit; tests/test_modes.py holds it to long double, to Python integers and to exact cases, tests/test_gpu_modes.py holds the device to it."""
import numpy as np

MASK = np.uint64(0xFFFFFFFF)
S = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04,
     2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10)
C = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05,
     -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11)
TURN = float(np.pi) * 2.0 ** -31      # the double nearest to pi 2^-31 (np.pi is the double nearest to pi, the scaling is exact)


def turns(X, inv_L):
    """uint64 (values below 2^32), the shape of X: T = (uint64) floor((t - floor(t)) 2^32) & 0xFFFFFFFF with t = X * inv_L."""
    t = np.asarray(X, dtype=np.float64) * np.asarray(inv_L, dtype=np.float64)
    u = t - np.floor(t)
    return np.floor(u * 4294967296.0).astype(np.uint64) & MASK


def phases(modes, T):
    """uint64 [N, K] (values below 2^32): (n_x T_x + n_y T_y + n_z T_z) mod 2^32 for modes int [K, 3] and turns [N, 3]."""
    n = (np.asarray(modes, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint64)      # two's complement, 32 bits
    T = np.asarray(T, dtype=np.uint64)
    phi = np.zeros((T.shape[0], n.shape[0]), dtype=np.uint64)
    for a in range(3):
        phi = (phi + ((T[:, a, None] * n[None, :, a]) & MASK)) & MASK           # (a product is below 2^64: nothing is lost mod 2^32)
    return phi


def phasor(phi):
    """(cos, sin) of 2 pi phi / 2^32 as the definition forms them; phi: unsigned integers below 2^32, any shape."""
    t = (np.asarray(phi, dtype=np.uint64) + np.uint64(1 << 29)) & MASK
    q = (t >> np.uint64(30)).astype(np.int64)
    r = (t & np.uint64((1 << 30) - 1)).astype(np.int64) - (1 << 29)
    x = r.astype(np.float64) * TURN
    z = x * x
    ps = S[5]
    for c in S[4::-1]:
        ps = c + z * ps
    pc = C[5]
    for c in C[4::-1]:
        pc = c + z * pc
    sn = x + (x * z) * ps
    cs = (1.0 - 0.5 * z) + (z * z) * pc
    odd = (q & 1) == 1
    co = np.where(odd, sn, cs)
    si = np.where(odd, cs, sn)
    co = np.where((q == 1) | (q == 2), -co, co)
    si = np.where(q >= 2, -si, si)
    return co, si


def weight_bound(weights, groups):
    """W: the smallest power of two above max |w| over the recorded particles, 1 if all are 0."""
    w = np.abs(np.asarray(weights, dtype=np.float64))
    if groups is not None:
        w = w[np.asarray(groups) >= 0]
    top = float(w.max()) if w.size else 0.0
    if top == 0.0:
        return 1.0
    m, e = np.frexp(top)
    return float(np.ldexp(1.0, int(e)))


def frac_bits(W):
    return 30 - int(np.log2(W))


def sample_sums(X, box, weights, groups, G, modes, F, limit=64.0, chunk=4096):
    """(A, B, bad): int64 [G, K] each and the number of recorded particles out of range (A, B are zeros then: the sample is invalid)."""
    X = np.asarray(X, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    grp = np.zeros(X.shape[0], dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    K = np.asarray(modes).reshape(-1, 3).shape[0]
    A, B = np.zeros((G, K), dtype=np.int64), np.zeros((G, K), dtype=np.int64)
    rec = grp >= 0
    bad = int(np.count_nonzero(rec & ~np.all(np.abs(X) < limit, axis=1)))      # (a NaN fails the compare)
    if bad:
        return A, B, bad
    inv_L = 1.0 / np.asarray(box, dtype=np.float64)
    scale = 2.0 ** F
    for g in range(G):
        at = np.nonzero(grp == g)[0]
        for lo in range(0, at.size, chunk):
            i = at[lo:lo + chunk]
            co, si = phasor(phases(modes, turns(X[i], inv_L)))
            A[g] += np.rint((w[i, None] * co) * scale).astype(np.int64).sum(axis=0)
            B[g] += np.rint((w[i, None] * si) * scale).astype(np.int64).sum(axis=0)
    return A, B, 0


def row_words(G, K):
    return 1 + G * G * K


def lag_counts(samples, every, num_lags):
    """int64 [num_lags + 1]: the origins behind every row after `samples` valid samples with no floor."""
    n = np.zeros(num_lags + 1, dtype=np.int64)
    n[0] = samples
    for j in range(samples):
        for l in range(1, num_lags + 1):
            if j - l >= 0 and (j - l) % every == 0:
                n[l] += 1
    return n


def correlate(sums, boxes, G, K, num_lags, every, F, floor=0):
    """The ring and the table over the samples' sums [(A, B, bad)] as the device keeps them.  floor: one value, or one per sample (the
    origin floor in force when the sample is taken).  Returns words int64 [num_lags + 1, 1 + G^2 K], out_of_range, invalid_samples, box_sum."""
    R = -(-num_lags // every) if num_lags else 0
    table = np.zeros((num_lags + 1, G, G, K), dtype=np.float64)
    count = np.zeros(num_lags + 1, dtype=np.int64)
    hold, ring = [-1] * R, [None] * R
    inv = 2.0 ** -F
    out_of_range = invalid = 0
    box_sum = np.zeros(3, dtype=np.float64)
    floors = [floor] * len(sums) if np.isscalar(floor) else list(floor)
    for j, (A, B, bad) in enumerate(sums):
        if bad == 0:
            a, b = A.astype(np.float64) * inv, B.astype(np.float64) * inv
            table[0] += a[:, None, :] * a[None, :, :] + b[:, None, :] * b[None, :, :]
            count[0] += 1
            for s in range(R):
                o = hold[s]
                if o < 0 or o < floors[j] or not 1 <= j - o <= num_lags:
                    continue
                ao, bo = ring[s][0].astype(np.float64) * inv, ring[s][1].astype(np.float64) * inv
                table[j - o] += ao[:, None, :] * a[None, :, :] + bo[:, None, :] * b[None, :, :]      # the origin is the first index
                count[j - o] += 1
            box_sum = box_sum + np.asarray(boxes[j], dtype=np.float64)
        else:
            out_of_range += bad
            invalid += 1
        if R and j % every == 0:
            slot = (j // every) % R
            hold[slot] = j if bad == 0 else -1
            if bad == 0:
                ring[slot] = (A.copy(), B.copy())
    words = np.zeros((num_lags + 1, row_words(G, K)), dtype=np.int64)
    words[:, 0] = count
    words[:, 1:] = table.reshape(num_lags + 1, -1).view(np.int64)
    return dict(words=words, out_of_range=out_of_range, invalid_samples=invalid, box_sum=box_sum)


def modes_reference(positions, boxes, weights, groups, G, modes, num_lags, every, F, limit=64.0, floor=0):
    """The whole recorder over float64 frames positions [samples, N, 3] with boxes [samples, 3]."""
    modes = np.asarray(modes).reshape(-1, 3)
    sums = [sample_sums(positions[j], boxes[j], weights, groups, G, modes, F, limit) for j in range(len(positions))]
    out = correlate(sums, boxes, G, modes.shape[0], num_lags, every, F, floor)
    out["sums"] = sums
    return out
