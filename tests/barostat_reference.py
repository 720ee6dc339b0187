"""Reference of the Monte Carlo barostat's device half (include/vvhip.h: "Monte Carlo barostat"), in NumPy and Python integers, and a
NumPy stand-in context for the driver (openmm-velocityverlet_amd/barostat.py).

The arithmetic, stated once in the header, restated here line for line:
    X   stored position in float64: float64(posq) + float64(correction) in mixed precision, float64(posq) in single, posq in double
    F   = 40 - ceil(log2(n_max)), n_max the largest molecule of the WHOLE System
    Q_i = llrint(X_i 2^F), to nearest even; finite |X_i| < 2^22 only (Overflow otherwise)
    S_m = sum of Q_i over the molecule: Python ints, exact
    c_m = (float(S_m) 2^-F) / float(n_m)      float(int) is correctly rounded, 2^-F is exact
    e_a = s_a - 1.0;   d = c_m e_a;   X' = X + d
    store: posq' = float32(X'), corr' = float32(X' - float64(posq')) in mixed; float32(X') in single; X' in double; .w untouched;
           an axis with e_a == 0 keeps its stored bits
A sharded plan holds particles [begin, end) of the System; F comes from the whole System's mol_id.
"""
import numpy as np


class Overflow(Exception):
    pass


def frac_bits(mol_id_system) -> int:
    n_max = int(np.bincount(np.asarray(mol_id_system, dtype=np.int64)).max())
    return 40 - (n_max - 1).bit_length()          # (n - 1).bit_length() = ceil(log2(n)) for n >= 1


def stored_positions(posq, corr, precision) -> np.ndarray:
    x = posq[:, :3].astype(np.float64)
    if precision == "mixed":
        x = x + corr[:, :3].astype(np.float64)
    return x


def centres(x, mol_id, F):
    """{molecule: (centre[3] as float64, n_m)} of the positions x [n, 3] (float64) -- Python-int sums."""
    if not (np.isfinite(x).all() and (np.abs(x) < 2.0 ** 22).all()):
        raise Overflow("a position is not finite or beyond 2^22 nm")
    q = np.rint(x * 2.0 ** F)                     # round half to even; |q| < 2^62: the float64 holds the integer exactly
    sums, count = {}, {}
    for i, m in enumerate(np.asarray(mol_id).tolist()):
        s = sums.setdefault(m, [0, 0, 0])
        for a in range(3):
            s[a] += int(q[i, a])
        count[m] = count.get(m, 0) + 1
    out = {}
    for m, s in sums.items():
        assert all(abs(v) < 2 ** 62 for v in s)
        out[m] = (np.array([(float(v) * 2.0 ** -F) / float(count[m]) for v in s], dtype=np.float64), count[m])
    return out


def scale(posq, corr, mol_id, scale3, precision, F):
    """The arrays after a scale: (posq', corr') as new arrays of the same dtype (corr' is corr for single / double).  mol_id: of these
    particles (a shard passes its slice).  Raises Overflow and changes nothing for a position out of range."""
    x = stored_positions(posq, corr, precision)
    cen = centres(x, mol_id, F)
    e = [float(s) - 1.0 for s in scale3]
    c = np.stack([cen[m][0] for m in np.asarray(mol_id).tolist()])
    new_posq, new_corr = posq.copy(), corr.copy()
    for a in range(3):
        if e[a] == 0.0:
            continue
        xn = x[:, a] + c[:, a] * e[a]
        if precision == "double":
            new_posq[:, a] = xn
        else:
            new_posq[:, a] = xn.astype(np.float32)
            if precision == "mixed":
                new_corr[:, a] = (xn - new_posq[:, a].astype(np.float64)).astype(np.float32)
    return new_posq, new_corr


class StandInContext:
    """What the driver needs of a context, on the CPU: positions in the stored layout of `precision`, box, molecule ids; scale_box and
    restore_box go through the reference above; scales_seen keeps every scale vector it was given."""

    def __init__(self, positions, box, mol_id, precision="mixed", charges=None):
        positions = np.asarray(positions, dtype=np.float64)
        real = np.float64 if precision == "double" else np.float32
        self.precision, self.mol_id = precision, np.asarray(mol_id, dtype=np.int64)
        self.posq = np.zeros((positions.shape[0], 4), dtype=real)
        self.posq[:, :3] = positions
        if charges is not None:
            self.posq[:, 3] = charges
        self.corr = np.zeros_like(self.posq)
        if precision == "mixed":
            self.corr[:, :3] = positions - self.posq[:, :3].astype(np.float64)
        self.box = np.asarray(box, dtype=np.float64).copy()
        self.F = frac_bits(self.mol_id)
        self.num_molecules = int(self.mol_id.max()) + 1
        self._backup = None
        self.scales_seen = []

    def getPeriodicBoxSize(self):
        return self.box.copy()

    def getPositions(self):
        return stored_positions(self.posq, self.corr, self.precision)

    def scale_box(self, scale3):
        s = np.array([float(v) for v in scale3], dtype=np.float64)
        self.scales_seen.append(s)
        new_posq, new_corr = scale(self.posq, self.corr, self.mol_id, s, self.precision, self.F)
        self._backup = (self.posq, self.corr, self.box.copy())
        self.posq, self.corr = new_posq, new_corr
        self.box = self.box * s

    def restore_box(self):
        if self._backup is None:
            raise RuntimeError("no scale to undo")
        self.posq, self.corr, self.box = self._backup
        self._backup = None
