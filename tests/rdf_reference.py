"""The definition of the device-side radial distribution functions (include/vvhip.h: vvhip_rdf_*) in NumPy, float64, operation for
operation: per axis d = X_i - X_j, n = rint(d * inv_L) (round-half-even), d = d - L * n, r2 = (dx dx + dy dy) + dz dz; squared edges
e(k) = ((double) k dr)^2 with dr = r_max / nbins; the bin b with e(b) <= r2 < e(b + 1) through searchsorted(e, r2, side="right") - 1; a
pair at or beyond e(nbins) adds nothing, a NaN r2 counts as invalid.  NumPy evaluates every line below as separate float64 operations
(no contraction).  Chunked over i so that 1 500 x 1 500 sites stay within a few MB per temporary."""
import numpy as np

CHUNK = 256


def edges2(r_max, nbins):
    """float64 [nbins + 1]: e(k) = ((double) k * dr) * ((double) k * dr), dr = r_max / nbins."""
    dr = np.float64(r_max) / np.float64(nbins)
    t = np.arange(int(nbins) + 1, dtype=np.float64) * dr
    return t * t


def r2_block(xa, xb, box):
    """float64 [len(xa), len(xb)]: the minimum-image squared distances as the header states them."""
    box = np.asarray(box, dtype=np.float64)
    inv = 1.0 / box
    sq = []
    for a in range(3):
        d = xa[:, None, a] - xb[None, :, a]
        n = np.rint(d * inv[a])
        d = d - box[a] * n
        sq.append(d * d)
    return (sq[0] + sq[1]) + sq[2]


def histogram(xa, xb, box, r_max, nbins, same=False, mol_a=None, mol_b=None):
    """(int64 [nbins], invalid) of the pairs (i in a, j in b); same=True: xa is xb and every unordered pair i < j counts once;
    mol_a / mol_b given: pairs with equal molecule are left out (counted nowhere)."""
    xa, xb = np.asarray(xa, dtype=np.float64).reshape(-1, 3), np.asarray(xb, dtype=np.float64).reshape(-1, 3)
    e = edges2(r_max, nbins)
    hist, invalid = np.zeros(int(nbins), dtype=np.int64), 0
    jj = np.arange(len(xb))
    with np.errstate(invalid="ignore"):
        for i0 in range(0, len(xa), CHUNK):
            i1 = min(len(xa), i0 + CHUNK)
            r2 = r2_block(xa[i0:i1], xb, box)
            keep = np.ones(r2.shape, dtype=bool)
            if same:
                keep &= np.arange(i0, i1)[:, None] < jj[None, :]
            if mol_a is not None:
                keep &= np.asarray(mol_a)[i0:i1, None] != np.asarray(mol_b)[None, :]
            v = r2[keep]
            nan = np.isnan(v)
            invalid += int(np.count_nonzero(nan))
            v = v[~nan]
            b = np.searchsorted(e, v, side="right") - 1
            b = b[b < nbins]                                         # r2 >= e(nbins): nothing
            hist += np.bincount(b, minlength=int(nbins)).astype(np.int64)
    return hist, invalid


def rdf_reference(x, box, groups, classes, r_max, nbins, mol_id=None):
    """(int64 [classes, nbins], invalid) of ONE sample: x [n, 3] float64 positions of every particle, groups [n] (-1: no site; None:
    everything in group 0), classes [(ga, gb)], mol_id [n] with the exclusion on (None: off).  Sites ascend by particle inside a group."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    g = np.zeros(len(x), dtype=np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    table, invalid = np.zeros((len(classes), int(nbins)), dtype=np.int64), 0
    for c, (ga, gb) in enumerate(classes):
        ia, ib = np.nonzero(g == ga)[0], np.nonzero(g == gb)[0]
        ma = None if mol_id is None else np.asarray(mol_id)[ia]
        mb = None if mol_id is None else np.asarray(mol_id)[ib]
        h, bad = histogram(x[ia], x[ib], box, r_max, nbins, same=(ga == gb), mol_a=ma, mol_b=mb)
        table[c] += h
        invalid += bad
    return table, invalid


def pairs_per_sample(groups, classes, n=None):
    """int64 [classes]: N_a N_b, or N_a (N_a - 1) / 2 for ga == gb."""
    g = np.zeros(int(n), dtype=np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    cnt = lambda k: int(np.count_nonzero(g == k))
    return np.array([cnt(a) * (cnt(a) - 1) // 2 if a == b else cnt(a) * cnt(b) for a, b in classes], dtype=np.int64)


def inv_volume_sum(boxes):
    """The sequential float64 sum s = s + 1.0 / ((Lx * Ly) * Lz) over the counted samples' boxes, in order."""
    s = np.float64(0.0)
    for b in boxes:
        b = np.asarray(b, dtype=np.float64)
        s = s + np.float64(1.0) / ((b[0] * b[1]) * b[2])
    return float(s)
