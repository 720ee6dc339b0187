"""The definition of the device-side spatial distribution functions (include/vvhip.h: vvhip_sdf_*) in NumPy, float64, operation for
operation.  Frames: p = X_a - X_o, q = X_b - X_o, n1 = (px px + py py) + pz pz, e1 = p * inverse_norm(n1), t = (qx e1x + qy e1y) + qz e1z,
w = q - t * e1, n2 likewise, e2 = w * inverse_norm(n2), e3 = e1 x e2 with every product rounded before its difference; a frame is bad where
n1 or n2 is NaN or outside [2^-40, 2^40).  Pairs: per axis d = X_s - X_o, n = rint(d * inv_L), d = d - L * n; xi_k = (dx e_kx + dy e_ky) +
dz e_kz; u_k = (xi_k + h) * inv_w with inv_w = n / (2.0 * h); in range iff 0 <= u_k < n on all three axes, the voxel is (int) u_k; a NaN u
of a good frame counts as invalid.  NumPy evaluates every line below as separate float64 operations (no contraction).  Chunked over the
frames so that 500 x 1 000 pairs stay within a few MB per temporary."""
import numpy as np

from acf_reference import N2_MAX, N2_MIN, inverse_norm

CHUNK = 256
MAX_GROUPS = 16


def norm2(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def frame_axes(x, frames):
    """(origin [F, 3], E [F, 3, 3] with the rows e1, e2, e3, good [F]) of the triplets frames [F, 3] = (o, a, b) over the positions x
    [n, 3]; a bad frame's origin and axes are NaN."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    fr = np.asarray(frames, dtype=np.int64).reshape(-1, 3)
    o = x[fr[:, 0]]
    p, q = x[fr[:, 1]] - o, x[fr[:, 2]] - o
    with np.errstate(invalid="ignore", over="ignore"):
        n1 = norm2(p)
        good = (n1 >= N2_MIN) & (n1 < N2_MAX)                         # (False for a NaN)
        e1 = p * inverse_norm(np.where(good, n1, 1.0))[:, None]
        t = dot(q, e1)
        w = q - t[:, None] * e1
        n2 = norm2(w)
        good &= (n2 >= N2_MIN) & (n2 < N2_MAX)
        e2 = w * inverse_norm(np.where(good, n2, 1.0))[:, None]
        e3 = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                       e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    E = np.stack([e1, e2, e3], axis=1)
    return np.where(good[:, None], o, np.nan), np.where(good[:, None, None], E, np.nan), good


def inv_w_of(extent, nbins):
    return np.float64(int(nbins)) / (2.0 * np.float64(extent))


def voxels(o, E, xs, box, extent, nbins, keep=None):
    """(int64 [nbins^3] flat in C order, invalid) of the pairs of the GOOD frames (o [F, 3], E [F, 3, 3]) with the sites xs [S, 3]; keep
    [F, S] bool masks pairs out (counted nowhere)."""
    n = int(nbins)
    box = np.asarray(box, dtype=np.float64)
    inv_L = 1.0 / box
    h, inv_w = np.float64(extent), inv_w_of(extent, nbins)
    hist, invalid = np.zeros(n * n * n, dtype=np.int64), 0
    with np.errstate(invalid="ignore", over="ignore"):
        for f0 in range(0, len(o), CHUNK):
            f1 = min(len(o), f0 + CHUNK)
            d = []
            for a in range(3):
                da = xs[None, :, a] - o[f0:f1, None, a]
                da = da - box[a] * np.rint(da * inv_L[a])
                d.append(da)
            u = []
            for k in range(3):
                xi = (d[0] * E[f0:f1, k, 0, None] + d[1] * E[f0:f1, k, 1, None]) + d[2] * E[f0:f1, k, 2, None]
                u.append((xi + h) * inv_w)
            take = np.ones(u[0].shape, dtype=bool) if keep is None else keep[f0:f1].copy()
            nan = np.isnan(u[0]) | np.isnan(u[1]) | np.isnan(u[2])
            invalid += int(np.count_nonzero(take & nan))
            take &= ~nan
            for k in range(3):
                take &= (u[k] >= 0.0) & (u[k] < n)
            i = [u[k][take].astype(np.int64) for k in range(3)]
            hist += np.bincount((i[0] * n + i[1]) * n + i[2], minlength=n * n * n).astype(np.int64)
    return hist, invalid


def group_array(groups, count):
    return np.zeros(int(count), dtype=np.int64) if groups is None else np.asarray(groups).astype(np.int64).reshape(-1)


def sdf_reference(x, box, frames, classes, extent, nbins, frame_groups=None, site_groups=None, mol_id=None):
    """(table int64 [classes, n, n, n], invalid, bad_frames, frame_visits int64 [16]) of ONE sample: x [N, 3] float64 positions of every
    particle, frames [F, 3], frame_groups [F] (-1: not recorded; None: group 0), site_groups [N] likewise, classes [(frame group, site
    group)], mol_id [N] with the exclusion on (None: off)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    fr = np.asarray(frames, dtype=np.int64).reshape(-1, 3)
    fg, sg = group_array(frame_groups, len(fr)), group_array(site_groups, len(x))
    n = int(nbins)
    o, E, good = frame_axes(x, fr)
    rec = fg >= 0
    visits = np.bincount(fg[rec & good], minlength=MAX_GROUPS).astype(np.int64)
    bad = int(np.count_nonzero(rec & ~good))
    table, invalid = np.zeros((len(classes), n, n, n), dtype=np.int64), 0
    for c, (a, b) in enumerate(classes):
        fi, si = np.nonzero((fg == a) & good)[0], np.nonzero(sg == b)[0]
        keep = None if mol_id is None else np.asarray(mol_id)[fr[fi, 0], None] != np.asarray(mol_id)[None, si]
        h, inv = voxels(o[fi], E[fi], x[si], box, extent, nbins, keep)
        table[c] += h.reshape(n, n, n)
        invalid += inv
    return table, invalid, bad, visits


def sdf_loop(x, box, frames, classes, extent, nbins, frame_groups=None, site_groups=None, mol_id=None):
    """The same by a plain Python loop over pairs, on Python floats (IEEE float64, one operation at a time), for small inputs."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    fr = np.asarray(frames, dtype=np.int64).reshape(-1, 3)
    fg, sg = group_array(frame_groups, len(fr)), group_array(site_groups, len(x))
    n, h = int(nbins), float(extent)
    inv_w = float(n) / (2.0 * h)
    L = [float(b) for b in box]
    inv_L = [1.0 / b for b in L]
    table = np.zeros((len(classes), n, n, n), dtype=np.int64)
    invalid, bad, visits = 0, 0, np.zeros(MAX_GROUPS, dtype=np.int64)
    axes = []
    for f, (io, ia, ib) in enumerate(fr):
        X = [[float(v) for v in x[i]] for i in (io, ia, ib)]
        p, q = [X[1][k] - X[0][k] for k in range(3)], [X[2][k] - X[0][k] for k in range(3)]
        n1 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
        E = None
        if N2_MIN <= n1 < N2_MAX:
            y = float(inverse_norm(np.array([n1]))[0])
            e1 = [v * y for v in p]
            t = (q[0] * e1[0] + q[1] * e1[1]) + q[2] * e1[2]
            w = [q[k] - t * e1[k] for k in range(3)]
            n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
            if N2_MIN <= n2 < N2_MAX:
                y = float(inverse_norm(np.array([n2]))[0])
                e2 = [v * y for v in w]
                e3 = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
                E = (X[0], e1, e2, e3)
        axes.append(E)
        if fg[f] >= 0:
            if E is None:
                bad += 1
            else:
                visits[fg[f]] += 1
    for c, (a, b) in enumerate(classes):
        for f in np.nonzero(fg == a)[0]:
            if axes[f] is None:
                continue
            o, e = axes[f][0], axes[f][1:]
            for s in np.nonzero(sg == b)[0]:
                if mol_id is not None and mol_id[fr[f, 0]] == mol_id[s]:
                    continue
                d = []
                for k in range(3):
                    dk = float(x[s, k]) - o[k]
                    dk = dk - L[k] * float(np.rint(dk * inv_L[k]))
                    d.append(dk)
                u = [(((d[0] * e[k][0] + d[1] * e[k][1]) + d[2] * e[k][2]) + h) * inv_w for k in range(3)]
                if any(v != v for v in u):
                    invalid += 1
                elif all(0.0 <= v < n for v in u):
                    table[c, int(u[0]), int(u[1]), int(u[2])] += 1
    return table, invalid, bad, visits


def pairs_per_sample(frame_groups, site_groups, classes, num_frames, num_atoms):
    """int64 [classes]: N_frames(frame group) * N_sites(site group); the exclusion does not lower it."""
    fg, sg = group_array(frame_groups, num_frames), group_array(site_groups, num_atoms)
    return np.array([int(np.count_nonzero(fg == a)) * int(np.count_nonzero(sg == b)) for a, b in classes], dtype=np.int64)


def inv_volume_sum(boxes):
    """The sequential float64 sum s = s + 1.0 / ((Lx * Ly) * Lz) over the counted samples' boxes, in order."""
    s = np.float64(0.0)
    for b in boxes:
        b = np.asarray(b, dtype=np.float64)
        s = s + np.float64(1.0) / ((b[0] * b[1]) * b[2])
    return float(s)


def frames_of_molecules(mol_id, masses, drude_particles=(), most=None):
    """[F, 3]: per molecule its first three particles that have mass and are no Drude particle (molecules with fewer give no frame), at
    most `most` frames spread evenly over the molecules."""
    mol_id, masses = np.asarray(mol_id), np.asarray(masses)
    ok = masses > 0
    ok[np.asarray(drude_particles, dtype=np.int64)] = False
    out = []
    for m in np.unique(mol_id):
        mem = np.nonzero((mol_id == m) & ok)[0]
        if len(mem) >= 3:
            out.append(mem[:3])
    out = np.array(out, dtype=np.int32).reshape(-1, 3)
    if most is not None and len(out) > most:
        out = out[np.linspace(0, len(out) - 1, most).astype(int)]
    return np.ascontiguousarray(out)
