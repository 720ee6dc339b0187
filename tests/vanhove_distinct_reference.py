"""The statement of the device-side distinct van Hove recorder (include/vvhip.h: vvhip_vanhove_distinct_*) in NumPy, float64 without
contraction.  The pair arithmetic and the squared edges are the RDF's (tests/rdf_reference.py: r2_block, edges2) with the i-site taken
at the origin and the j-site now, d = X_j(now) - X_i(origin); the (sample, origin) pairs are the MSD's (tests/msd_reference.py: pairs) with
row l = j - origin and a row 0 of every sample against itself in front.  Imported by tests/test_vanhove_distinct.py (against a plain
loop) and tests/test_gpu_vanhove_distinct.py (against the device's table, fed with float64 frames)."""
import numpy as np

from msd_reference import num_origins, pairs      # noqa: F401
from rdf_reference import edges2, r2_block

MAX_WORDS = 1 << 22


def visits_of(num_samples, origin_every, num_lags, floor=0):
    """[(j, origin ordinal, row)] of samples 0 .. num_samples - 1 in the order the device visits the rows of one sample after another:
    (j, j, 0) for every sample, and (j, k E, j - k E) for every origin with floor_j <= k E < j and j - k E <= num_lags.  `floor`: one
    ordinal, or one per sample (the floor as it stood at that sample)."""
    out = [(j, j, 0) for j in range(num_samples)]
    out += [(j, o, row + 1) for j, o, row in pairs(num_samples, origin_every, num_lags, floor)]
    return sorted(out, key=lambda v: v[0])      # (stable: per sample row 0 first; a row gets at most one visit per sample)


def pairs_per_sample(groups, classes, n=None):
    """int64 [classes]: N_a N_b, or N_a (N_a - 1) for ga == gb (ordered pairs of two different sites)."""
    g = np.zeros(int(n), dtype=np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    cnt = lambda k: int(np.count_nonzero(g == k))
    return np.array([cnt(a) * (cnt(a) - 1) if a == b else cnt(a) * cnt(b) for a, b in classes], dtype=np.int64)


def histogram(x_origin, x_now, box, r_max, nbins, same=False, mol_a=None, mol_b=None):
    """(int64 [nbins], invalid) of the ordered pairs (i at the origin, j now); same=True: both are the sites of one group, and a site is
    not paired with its own earlier self; mol_a / mol_b given: pairs with equal molecule are left out (counted nowhere)."""
    xa, xb = np.asarray(x_origin, dtype=np.float64).reshape(-1, 3), np.asarray(x_now, dtype=np.float64).reshape(-1, 3)
    e = edges2(r_max, nbins)
    with np.errstate(invalid="ignore"):
        r2 = r2_block(xb, xa, box).T                               # [i, j]: d = X_j(now) - X_i(origin)
    keep = np.ones(r2.shape, dtype=bool)
    if same:
        keep &= ~np.eye(len(xa), len(xb), dtype=bool)
    if mol_a is not None:
        keep &= np.asarray(mol_a)[:, None] != np.asarray(mol_b)[None, :]
    v = r2[keep]
    nan = np.isnan(v)
    v = v[~nan]
    b = np.searchsorted(e, v, side="right") - 1
    b = b[b < nbins]                                               # r2 >= e(nbins): nothing
    return np.bincount(b, minlength=int(nbins)).astype(np.int64), int(np.count_nonzero(nan))


def vanhove_distinct_reference(x, boxes, groups, classes, r_max, nbins, num_lags, origin_every, mol_id=None, floor=0):
    """(head int64 [num_lags + 1, 2], hist int64 [classes, num_lags + 1, nbins], invalid) of the samples x float64 [J, n, 3] (every
    particle's position as a float64 frame holds it, ordinal 0 first).  boxes: [3] or [J, 3], the box each sample ran with (the box NOW
    decides the image and the 1 / V of a visit).  groups [n] (-1: no site; None: everything in group 0), classes [(ga, gb)] ordered,
    mol_id [n] with the exclusion on (None: off).  head[l] = (visits, the bits of the sequential float64 sum of 1 / V over them)."""
    x = np.asarray(x, dtype=np.float64)
    J, n = x.shape[0], x.shape[1]
    boxes = np.broadcast_to(np.asarray(boxes, dtype=np.float64), (J, 3))
    g = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    rows = int(num_lags) + 1
    visits, ivs = np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.float64)
    hist, invalid = np.zeros((len(classes), rows, int(nbins)), dtype=np.int64), 0
    sites = {k: np.nonzero(g == k)[0] for k in set(int(v) for c in classes for v in c)}
    for j, o, row in visits_of(J, origin_every, num_lags, floor):
        L = boxes[j]
        visits[row] += 1
        ivs[row] = ivs[row] + np.float64(1.0) / ((L[0] * L[1]) * L[2])
        for c, (ga, gb) in enumerate(classes):
            ia, ib = sites[int(ga)], sites[int(gb)]
            ma = None if mol_id is None else np.asarray(mol_id)[ia]
            mb = None if mol_id is None else np.asarray(mol_id)[ib]
            h, bad = histogram(x[o][ia], x[j][ib], L, r_max, nbins, same=(ga == gb), mol_a=ma, mol_b=mb)
            hist[c, row] += h
            invalid += bad
    head = np.stack([visits, ivs.view(np.int64)], axis=1)
    return head, hist, invalid
