"""The definition of a device-side profile (include/vvhip.h: vvhip_profile_*) in NumPy: what one sample adds to the table.

Everything is float64, one rounding per operation, no contraction.  For particle i with group g >= 0 and coordinate c along the axis

    t = c * inv_L  (inv_L = 1.0 / box[axis]),   u = t - floor(t),   b = min(int(u * nbins), nbins - 1)

(positions are unwrapped: this is the periodic wrap, and c = -1e-20 gives u = 1.0, the last bin by the clamp).  The rows of a group are
the enabled quantities in the order count, charge, mass, momentum x | y | z, kinetic, with the terms

    count 1     charge q     mass m     momentum m * v.x, m * v.y, m * v.z     kinetic m * ((v.x * v.x + v.y * v.y) + v.z * v.z)

and a term x is added as the integer rint(x * 2^frac_bits[quantity]), round-half-even (count: the integer 1).  A particle any of whose
enabled terms is NaN or has |x| >= limit[quantity] is left out of every row and counted in out_of_range instead.
"""
import numpy as np

COUNT, CHARGE, MASS, MOMENTUM, KINETIC = 1, 2, 4, 8, 16
QUANTITIES = ("count", "charge", "mass", "momentum", "kinetic")
ROWS_OF = (1, 1, 1, 3, 1)


def rows_of_mask(mask):
    """(first row of every quantity or -1, rows per group) for a mask; count is always on."""
    mask |= COUNT
    row_of, rows = [], 0
    for q in range(5):
        row_of.append(rows if mask & (1 << q) else -1)
        rows += ROWS_OF[q] if mask & (1 << q) else 0
    return row_of, rows


def bins(c, box_axis, nbins):
    """The bin of every coordinate (already summed in float64)."""
    t = np.asarray(c, dtype=np.float64) * (1.0 / np.float64(box_axis))
    u = t - np.floor(t)
    b = (u * np.float64(nbins)).astype(np.int64)
    return np.minimum(b, nbins - 1)


def profile_reference(positions, velocities, charges, masses, groups, box, desc, frac_bits):
    """One sample: (int64 table [num_groups, rows, nbins], out_of_range).
    positions, velocities: float64 [n, 3]; charges, masses: [n]; groups: int [n] (-1: not recorded) or None (everything in group 0);
    desc: anything with axis, nbins, mask, num_groups and limit[5] as applied (a vvhip_profile_layout); frac_bits: [5] by quantity."""
    x = np.asarray(positions, dtype=np.float64)
    v = np.asarray(velocities, dtype=np.float64)
    q = np.asarray(charges, dtype=np.float64)
    m = np.asarray(masses, dtype=np.float64)
    n = x.shape[0]
    g = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    mask = int(desc.mask) | COUNT
    nbins, num_groups, axis = int(desc.nbins), int(desc.num_groups), int(desc.axis)
    row_of, rows = rows_of_mask(mask)
    b = bins(x[:, axis], box[axis], nbins)
    terms = {}                                                      # row -> (values, quantity)
    if mask & CHARGE:
        terms[row_of[1]] = (q, 1)
    if mask & MASS:
        terms[row_of[2]] = (m, 2)
    if mask & MOMENTUM:
        for k in range(3):
            terms[row_of[3] + k] = (m * v[:, k], 3)
    if mask & KINETIC:
        terms[row_of[4]] = (m * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]), 4)
    recorded = g >= 0
    bad = np.zeros(n, dtype=bool)
    for values, quantity in terms.values():
        bad |= ~(np.abs(values) < np.float64(desc.limit[quantity]))     # (NaN compares false: out of range)
    keep = recorded & ~bad
    table = np.zeros((num_groups, rows, nbins), dtype=np.int64)
    np.add.at(table, (g[keep], 0, b[keep]), 1)
    for row, (values, quantity) in terms.items():
        with np.errstate(invalid="ignore"):
            words = np.rint(values[keep] * 2.0 ** int(frac_bits[quantity])).astype(np.int64)
        np.add.at(table, (g[keep], row, b[keep]), words)
    return table, int(np.count_nonzero(recorded & bad))
