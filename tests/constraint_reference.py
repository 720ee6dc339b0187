"""Exact solutions of the constrained-update equations, in float64 NumPy: an algorithm-independent reference for every constraint
solver of the product (hydrogen-type clusters by Newton, direct solve or Gauss-Seidel sweeps; SETTLE; the general clusters' coloured
sweeps) and of the oracle.  Test code only.

Positions (OpenMM's applyConstraints).  Old positions x, a step displacement delta; the constrained displacement is

    delta_c = delta + M^-1 sum_k lambda_k grad sigma_k(x),      sigma_k(x) = |x_a - x_b|^2 - d_k^2,

with the gradients taken at the OLD bond vectors r_k = x_a - x_b, and the multipliers chosen so that every constraint holds at
x + delta_c.  solve_positions solves for all multipliers of the cluster at once by Newton's method with the exact Jacobian and
iterates until the residual stops falling (|sigma| ~ 1e-16 d^2), not to a tolerance.

Velocities (applyVelocityConstraints).  The linear version at the current positions: v' = v + M^-1 G^T mu with (G M^-1 G^T) mu = -G v,
G_k = the gradient of r_k . (v_a - v_b); solve_velocities solves it directly.

lagrange_residual is the structural check that needs no exact solution: every SHAKE-family iterate moves particle i by a combination of
ITS OWN old bonds, weighted by its inverse mass, so m_i (delta_c_i - delta_i) lies in the span of the old bond directions however far
the solver has converged.  A correction with a wrong mass or along a new bond does not.

What the solvers see, from the product's host tables (csrc/vv_host.cpp) and the oracle's (oracle/oracle.py: build_constraint_clusters,
build_general_constraints), so that the reference solves the same problem the kernels are handed:
  * hydrogen-type clusters: 1/m_central, 1/m_peripheral and d^2 are packed as float (the float4 cluster parameters);
  * general clusters: d^2, 1/m_a, 1/m_b packed as float;
  * SETTLE: the two distances packed as float (squared in the solver's precision), the inverse masses those of velm.w, i.e. 1/m
    rounded to the `mixed` type (float in single precision, double otherwise);
  * positions: posq in single and double precision; posq + posq_corr summed in double in mixed precision.
pack_inverse_mass / pack_distance below give those roundings; the tests apply them before they call the reference."""
import numpy as np

EPS = np.finfo(np.float64).eps


def pack_inverse_mass(masses, kind, prec):
    """1/m as the solver sees it: kind "cluster" / "general" -> float; "settle" -> the mixed type of `prec`."""
    im = 1.0 / np.asarray(masses, dtype=np.float64)
    if kind == "settle" and prec != "single":
        return im
    return im.astype(np.float32).astype(np.float64)


def pack_distance(dist, kind):
    """The constraint distance the solver converges to: sqrt(float(d^2)) for the float d^2 of clusters / general constraints,
    float(d) for SETTLE."""
    d = np.asarray(dist, dtype=np.float64)
    if kind == "settle":
        return d.astype(np.float32).astype(np.float64)
    return np.sqrt((d * d).astype(np.float32).astype(np.float64))


def _columns(x, inv_mass, cons):
    """W[k] = d(delta_c)/d(lambda_k): inv_mass_a r_k at a, -inv_mass_b r_k at b (shape [k, n, 3])."""
    cons = np.asarray(cons).reshape(-1, 2)
    r = x[cons[:, 0]] - x[cons[:, 1]]
    W = np.zeros((len(cons),) + x.shape)
    for k, (a, b) in enumerate(cons):
        W[k, a] += inv_mass[a] * r[k]
        W[k, b] -= inv_mass[b] * r[k]
    return cons, r, W


def _bond_jacobian(cons, W):
    """J[k, m] = d(bond_k)/d(lambda_m) as vectors: W[m, a_k] - W[m, b_k] (shape [k, m, 3])."""
    return W[:, cons[:, 0]].transpose(1, 0, 2) - W[:, cons[:, 1]].transpose(1, 0, 2)


def solve_positions(x, delta, inv_mass, cons, dist, max_iter=100):
    """Constrained displacement of `x` (float64 [n, 3]) moved by `delta`: returns (delta_c, lambda).  Newton on all multipliers at once,
    exact Jacobian; stops when the largest |sigma_k| / d_k^2 no longer falls (machine precision), and raises if that is above 1e-13."""
    x, delta, inv_mass = (np.asarray(a, dtype=np.float64) for a in (x, delta, inv_mass))
    d2 = np.asarray(dist, dtype=np.float64) ** 2
    cons, r, W = _columns(x, inv_mass, cons)
    D = _bond_jacobian(cons, W)
    lam = np.zeros(len(cons))
    best, stall = np.inf, 0
    for _ in range(max_iter):
        dc = delta + np.tensordot(lam, W, 1)
        b = r + dc[cons[:, 0]] - dc[cons[:, 1]]
        g = (b * b).sum(1) - d2
        err = np.abs(g / d2).max()
        if err < best * 0.5:
            best, stall = err, 0
        else:
            stall += 1
            if stall >= 3:
                break
        J = 2.0 * np.einsum("ka,kma->km", b, D)
        lam = lam - np.linalg.solve(J, g)
    if best > 1e-13:
        raise ArithmeticError(f"reference Newton did not converge: |sigma|/d^2 = {best:.2e}")
    return delta + np.tensordot(lam, W, 1), lam


def solve_velocities(x, v, inv_mass, cons):
    """Velocities with every bond-parallel relative velocity removed at positions `x`: returns (v', mu)."""
    x, v, inv_mass = (np.asarray(a, dtype=np.float64) for a in (x, v, inv_mass))
    cons, r, W = _columns(x, inv_mass, cons)
    D = _bond_jacobian(cons, W)
    A = np.einsum("ka,kma->km", r, D)
    rhs = -((v[cons[:, 0]] - v[cons[:, 1]]) * r).sum(1)
    mu = np.linalg.solve(A, rhs)
    return v + np.tensordot(mu, W, 1), mu


def lagrange_residual(x, delta, delta_c, inv_mass, cons):
    """Relative residual of the least-squares fit of m_i (delta_c_i - delta_i) onto the old bond directions (+r_k at a, -r_k at b).
    Rounding level for any correction of SHAKE form, converged or not; 0 for a zero correction.  Works for velocities as well
    (delta = v, delta_c = v').  Fitted component by component (the bond matrix is block diagonal); a particle in no constraint
    contributes its whole correction to the residual."""
    x = np.asarray(x, dtype=np.float64)
    inv_mass = np.asarray(inv_mass, dtype=np.float64)
    cons = np.asarray(cons).reshape(-1, 2)
    y = (np.asarray(delta_c, dtype=np.float64) - np.asarray(delta, dtype=np.float64)) / inv_mass[:, None]
    ny = np.linalg.norm(y)
    if ny == 0.0:
        return 0.0
    free = np.ones(len(x), bool)
    res2 = 0.0
    for comp in components(len(x), cons):
        idx = np.array(comp)
        free[idx] = False
        local = {g: l for l, g in enumerate(comp)}
        sel = np.array([int(a) in local for a in cons[:, 0]])
        G = np.zeros((int(sel.sum()), len(comp), 3))
        for k, (a, b) in enumerate(cons[sel]):
            r = x[a] - x[b]
            G[k, local[int(a)]] += r
            G[k, local[int(b)]] -= r
        G = G.reshape(len(G), -1).T
        yc = y[idx].reshape(-1)
        coef, *_ = np.linalg.lstsq(G, yc, rcond=None)
        res2 += float(((yc - G @ coef) ** 2).sum())
    res2 += float((y[free] ** 2).sum())
    return float(np.sqrt(res2) / ny)


def momentum_defect(delta, delta_c, inv_mass):
    """|sum_i m_i (delta_c_i - delta_i)| / sum_i |m_i (delta_c_i - delta_i)|: a correction by internal constraint forces moves no centre of mass."""
    p = (np.asarray(delta_c, np.float64) - np.asarray(delta, np.float64)) / np.asarray(inv_mass, np.float64)[:, None]
    s = np.abs(p).sum()
    return 0.0 if s == 0 else float(np.linalg.norm(p.sum(0)) / s)


def angular_momentum_defect(x, delta, delta_c, inv_mass, origin=(0.0, 0.0, 0.0)):
    """|sum_i (x_i - o) x m_i (delta_c_i - delta_i)| relative to sum_i |x_i - o| |m_i (delta_c_i - delta_i)|: central forces along the
    old bonds exert no torque about any point o."""
    x = np.asarray(x, np.float64) - np.asarray(origin, np.float64)
    p = (np.asarray(delta_c, np.float64) - np.asarray(delta, np.float64)) / np.asarray(inv_mass, np.float64)[:, None]
    s = (np.linalg.norm(x, axis=1) * np.linalg.norm(p, axis=1)).sum()
    return 0.0 if s == 0 else float(np.linalg.norm(np.cross(x, p).sum(0)) / s)


def components(n, cons):
    """Connected components of the constraint graph (lists of particle indices, sorted), particles in no constraint left out."""
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for a, b in np.asarray(cons).reshape(-1, 2):
        parent[find(int(a))] = find(int(b))
    seen = {}
    for a in np.unique(np.asarray(cons).reshape(-1)):
        seen.setdefault(find(int(a)), []).append(int(a))
    return [sorted(v) for v in seen.values()]


def solve_all(x, delta, inv_mass, cons, dist, velocities=False):
    """solve_positions / solve_velocities component by component over a whole system; particles in no constraint keep delta.
    Returns (result, {component index tuple: multipliers})."""
    x = np.asarray(x, np.float64)
    out = np.array(delta, dtype=np.float64, copy=True)
    cons = np.asarray(cons).reshape(-1, 2)
    dist = np.asarray(dist, np.float64)
    mult = {}
    for comp in components(len(x), cons):
        idx = np.array(comp)
        local = {g: l for l, g in enumerate(comp)}
        sel = np.array([int(a) in local for a in cons[:, 0]])
        lc = np.array([[local[int(a)], local[int(b)]] for a, b in cons[sel]]).reshape(-1, 2)
        if velocities:
            res, m = solve_velocities(x[idx], out[idx], inv_mass[idx], lc)
        else:
            res, m = solve_positions(x[idx], out[idx], inv_mass[idx], lc, dist[sel])
        out[idx] = res
        mult[tuple(comp)] = m
    return out, mult
