"""The definition of the device-side contact lifetime correlations (include/vvhip.h: vvhip_contacts_*) in NumPy and Python integers: a loop
over samples.  A contact matrix is a boolean array [N_a, N_b]; a popcount is its sum as a Python int.  Shared by tests/test_contacts.py and
tests/test_gpu_contacts.py; nothing here touches a GPU."""
import numpy as np


def sites(groups, n, g):
    """The particles of group g in ascending index (groups = None: everything in group 0)."""
    if groups is None:
        return np.arange(n) if g == 0 else np.zeros(0, dtype=np.int64)
    return np.nonzero(np.asarray(groups) == g)[0]


def r2_matrix(xa, xb, box):
    """float64 [N_a, N_b]: per axis d = X_i - X_j, n = rint(d * inv_L), d = d - L * n; then (dx dx + dy dy) + dz dz.  Every operation is a
    correctly rounded float64 one and none is contracted: what the device forms."""
    xa, xb, box = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64), np.asarray(box, dtype=np.float64)
    inv = 1.0 / box
    sq = []
    with np.errstate(invalid="ignore"):
        for a in range(3):
            d = xa[:, None, a] - xb[None, :, a]
            d = d - box[a] * np.rint(d * inv[a])
            sq.append(d * d)
    return (sq[0] + sq[1]) + sq[2]


def contact_matrices(x, box, groups, classes, r_cut, mol_id=None):
    """([bool [N_a, N_b] per class], invalid): h of one configuration x [n, 3] (float64 positions as a float64 frame holds them)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    out, invalid = [], 0
    for (ga, gb), rc in zip(classes, r_cut):
        ia, ib = sites(groups, n, ga), sites(groups, n, gb)
        r2 = r2_matrix(x[ia], x[ib], box)
        live = np.ones(r2.shape, dtype=bool)
        if ga == gb:
            live &= ia[:, None] != ib[None, :]
        if mol_id is not None:
            mol = np.asarray(mol_id)
            live &= mol[ia][:, None] != mol[ib][None, :]
        with np.errstate(invalid="ignore"):
            h = live & (r2 < np.float64(rc) * np.float64(rc))
        invalid += int(np.count_nonzero(live & np.isnan(r2)))
        out.append(h)
    return out, invalid


class Recorder:
    """The recorder's state and one method per event, in the words of the header."""

    def __init__(self, num_classes, num_lags, origin_every, continuous=True, max_samples=1 << 62):
        self.C, self.num_lags, self.E, self.continuous, self.max_samples = num_classes, num_lags, origin_every, continuous, max_samples
        self.R = -(-num_lags // origin_every)
        self.dropped = self.invalid = 0
        self.reset()

    def reset(self):
        self.table = [[[0, 0, 0, 0] for _ in range(self.num_lags)] for _ in range(self.C)]
        self.origin, self.cont, self.ord = [None] * self.R, [None] * self.R, [-1] * self.R
        self.samples = self.dropped = self.invalid = 0

    def drop(self):
        self.dropped += 1

    def sample(self, h, invalid=0):
        """h: one boolean matrix per class."""
        if self.samples >= self.max_samples:
            return self.drop()
        j = self.samples
        self.invalid += invalid
        if j % self.E == 0:
            s = (j // self.E) % self.R
            self.origin[s], self.cont[s], self.ord[s] = [m.copy() for m in h], [m.copy() for m in h], j
        for s in range(self.R):
            l = j - self.ord[s]
            if self.ord[s] < 0 or l >= self.num_lags:
                continue
            for c in range(self.C):
                self.cont[s][c] &= h[c]
                row = self.table[c][l]
                row[0] += 1
                row[1] += int(np.count_nonzero(self.origin[s][c]))
                row[2] += int(np.count_nonzero(self.origin[s][c] & h[c]))
                if self.continuous:
                    row[3] += int(np.count_nonzero(self.cont[s][c]))
        self.samples += 1

    def words(self):
        return np.array(self.table, dtype=np.int64).reshape(self.C, self.num_lags, 4)


def contacts_reference(frames, boxes, groups, classes, r_cut, num_lags, origin_every, mol_id=None, continuous=True, max_samples=1 << 62):
    """(int64 table [classes, lags, 4], samples, dropped, invalid) over the configurations `frames` [samples, n, 3], frame k in box boxes[k]."""
    rec = Recorder(len(classes), num_lags, origin_every, continuous, max_samples)
    for x, box in zip(frames, boxes):
        h, bad = contact_matrices(x, box, groups, classes, r_cut, mol_id)
        rec.sample(h, bad if rec.samples < rec.max_samples else 0)
    return rec.words(), rec.samples, rec.dropped, rec.invalid


def planes_to_positions(planes):
    """A frame's planar float64 positions [3, n] as [n, 3]."""
    return np.ascontiguousarray(np.asarray(planes).T)


def layout(rows, cols, num_lags, origin_every, continuous, sites_total, head_words=4):
    """vv_layout.h: contacts_layout, in Python integers."""
    rows_padded = [-(-r // 64) * 64 for r in rows]
    col_words = [-(-c // 64) for c in cols]
    class_words = [a * b for a, b in zip(rows_padded, col_words)]
    sample_words = sum(class_words)
    R = -(-num_lags // origin_every)
    ord_words = (R + 1) // 2 * 2
    table_words = len(rows) * num_lags * 4
    ring_words = R * sample_words * (2 if continuous else 1)
    words_bytes = (head_words + table_words + ord_words + ring_words) * 8
    scratch_bytes = sample_words * 8 + 3 * (-(-sites_total // 16) * 16) * 8
    return dict(rows_padded=rows_padded, col_words=col_words, class_words=class_words, sample_words=sample_words, num_origins=R,
                ord_words=ord_words, table_words=table_words, ring_words=ring_words, words_bytes=words_bytes, scratch_bytes=scratch_bytes,
                total_bytes=words_bytes + scratch_bytes)
