"""The statement of vvhip_set_velocities_to_temperature (include/vvhip.h) in NumPy: Philox4x32-10 in uint64 arithmetic, Box-Muller in
float64.  The result is a function of (seed, global particle index, masses, T, T_D) alone; tests/test_thermalize.py checks the generator
against known answers and that this reference meets the statistical bounds the GPU tests put on the device's draw."""
import numpy as np

R = 8.31446261815324e-3          # kJ/(mol K), as include/vvhip.h
TAG = 0x5654                     # counter word 3 of this stream (vv_kernel_fill_normals has 0x5656)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two 32-bit words; returns the four output words as uint64 arrays."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _LOW for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _32) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> _32) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def normals(g, seed):
    """n(g): [len(g), 3] standard normals of the particles with global indices g."""
    g = np.asarray(g, dtype=np.uint64)
    zero = np.zeros_like(g)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((g, zero, zero, zero + np.uint64(TAG)), (seed & 0xFFFFFFFF, seed >> 32))
    s = 2.0 ** -32
    u0, u1, u2, u3 = (w[0].astype(np.float64) + 1.0) * s, w[1].astype(np.float64) * s, (w[2].astype(np.float64) + 1.0) * s, w[3].astype(np.float64) * s
    r0, r1 = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    return np.stack([r0 * np.cos(2 * np.pi * u1), r0 * np.sin(2 * np.pi * u1), r1 * np.cos(2 * np.pi * u3)], axis=1)


def velocities(masses, drude_pairs, temperature, seed, drude_temperature=None):
    """float64 [N, 3] for the whole system (global index = row).  drude_temperature None: plain mode."""
    m = np.asarray(masses, dtype=np.float64)
    n = normals(np.arange(m.size), seed)
    v = np.zeros((m.size, 3))
    massive = m > 0
    v[massive] = np.sqrt(R * temperature / m[massive])[:, None] * n[massive]
    pairs = np.asarray(drude_pairs, dtype=np.int64).reshape(-1, 2)
    if drude_temperature is not None and len(pairs):
        d, p = pairs[:, 0], pairs[:, 1]
        both = (m[d] > 0) & (m[p] > 0)
        d, p = d[both], p[both]
        md, mp = m[d], m[p]
        M = md + mp
        mu = md * mp / M
        V = np.sqrt(R * temperature / M)[:, None] * n[p]
        w = np.sqrt(R * drude_temperature / mu)[:, None] * n[d]
        v[d] = V + (mp / M)[:, None] * w
        v[p] = V - (md / M)[:, None] * w
    return v


def split_pairs(masses, drude_pairs):
    """The (Drude, parent) pairs with both masses > 0: what the Drude-aware mode splits."""
    m = np.asarray(masses, dtype=np.float64)
    pairs = np.asarray(drude_pairs, dtype=np.int64).reshape(-1, 2)
    return pairs[(m[pairs[:, 0]] > 0) & (m[pairs[:, 1]] > 0)] if len(pairs) else pairs


def plain_temperature(masses, v):
    """sum m v^2 / (3 N_massive R)"""
    m = np.asarray(masses, dtype=np.float64)
    massive = m > 0
    return float(np.sum(m[massive, None] * v[massive] ** 2) / (3 * np.count_nonzero(massive) * R))


def drude_temperature(masses, drude_pairs, v):
    """sum mu |v_d - v_p|^2 / (3 N_pairs R) over the split pairs: the T_Drude of the Drude temperature report."""
    m = np.asarray(masses, dtype=np.float64)
    pairs = split_pairs(m, drude_pairs)
    d, p = pairs[:, 0], pairs[:, 1]
    mu = m[d] * m[p] / (m[d] + m[p])
    return float(np.sum(mu[:, None] * (v[d] - v[p]) ** 2) / (3 * len(pairs) * R))


def two_ke(masses, v):
    m = np.asarray(masses, dtype=np.float64)
    return float(np.sum(m[:, None] * v ** 2))


def correlation(a, b):
    a, b = np.ravel(a), np.ravel(b)
    return float(np.sum(a * b) / np.sqrt(np.sum(a * a) * np.sum(b * b)))
