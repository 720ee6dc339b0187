"""CPU: the exact constrained-update reference (tests/constraint_reference.py) against closed forms and its own invariants, and the oracle's
constraint solvers (oracle/vv_oracle.c, called one at a time through ctypes) against the reference on the edge cases of
tests/constraint_cases.py, in all three precisions.  The oracle shares the kernels' algorithms and cluster tables; the reference shares
neither, so this tier states how far the oracle itself is from the exact solution (printed per solver with -s)."""
import ctypes as C

import numpy as np
import pytest

import constraint_cases as cc
import constraint_reference as cr
from oracle import oracle as O

TOL = 1e-5          # VVIntegrator's default constraint tolerance
TIGHT = 1e-10
WORST = {}


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), value)


# ----------------------------------------------------------------------------- the reference against closed forms
def test_two_body_constraint_is_the_root_of_a_quadratic():
    """One constraint between two bodies: bond b = s + lambda (1/m_a + 1/m_b) r with s the unconstrained new bond; |b| = d is a quadratic in
    lambda, the root of smaller magnitude is the constrained step."""
    rng = np.random.default_rng(3)
    for _ in range(20):
        m = rng.uniform(1.0, 40.0, 2)
        im = 1.0 / m
        d = rng.uniform(0.08, 0.2)
        u = rng.standard_normal(3); u /= np.linalg.norm(u)
        x = np.array([np.zeros(3), -d * u]) + rng.uniform(0, 3, 3)
        delta = rng.standard_normal((2, 3)) * 0.03 * d
        dc, lam = cr.solve_positions(x, delta, im, [(0, 1)], [d])
        r = x[0] - x[1]
        s = r + delta[0] - delta[1]
        ims = im.sum()
        qa, qb, qc = ims * ims * r.dot(r), 2 * ims * s.dot(r), s.dot(s) - d * d
        roots = np.roots([qa, qb, qc]).real
        lam_exact = roots[np.argmin(np.abs(roots))]
        assert abs(lam[0] - lam_exact) <= 1e-12 * abs(lam_exact)
        np.testing.assert_allclose(dc[0], delta[0] + im[0] * lam_exact * r, rtol=0, atol=1e-15)
        np.testing.assert_allclose(dc[1], delta[1] - im[1] * lam_exact * r, rtol=0, atol=1e-15)
        # velocities: the bond-parallel part of the relative velocity is removed, the centre of mass keeps its velocity
        v = rng.standard_normal((2, 3))
        v2, _ = cr.solve_velocities(x, v, im, [(0, 1)])
        e = r / np.linalg.norm(r)
        assert abs((v2[0] - v2[1]).dot(e)) < 1e-14
        np.testing.assert_allclose((m[:, None] * v2).sum(0), (m[:, None] * v).sum(0), rtol=1e-14, atol=1e-14)
        np.testing.assert_allclose(np.cross(e, v2[0] - v2[1]), np.cross(e, v[0] - v[1]), atol=1e-14)


def _rot(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


@pytest.mark.parametrize("motion", ["translation", "rotation"])
def test_rigid_motion_of_a_rigid_triangle_needs_no_correction(motion):
    """A symmetric rigid triangle moved rigidly (translated, or rotated by a finite angle about any point) already satisfies its
    constraints: delta_c = delta, lambda = 0.  A rigid-body velocity needs no velocity correction either."""
    masses, pos, cons, dist = cc.triangle(None, 15.999, 1.008, 0.1, 109.47)
    pos = pos + np.array([1.0, 2.0, 0.5])
    im = 1.0 / masses
    if motion == "translation":
        delta = np.tile([0.01, -0.02, 0.005], (3, 1))
    else:
        R, o = _rot([0.3, -1.0, 0.4], 0.35), np.array([0.7, 1.1, 0.2])
        delta = (pos - o) @ R.T + o - pos
    dc, lam = cr.solve_positions(pos, delta, im, cons, dist)
    assert np.abs(lam).max() < 1e-12
    np.testing.assert_allclose(dc, delta, rtol=0, atol=1e-15)
    w = np.array([3.0, -1.0, 2.0])
    v = np.cross(w, pos - pos.mean(0)) + np.array([0.3, 0.1, -0.2])
    v2, mu = cr.solve_velocities(pos, v, im, cons)
    assert np.abs(mu).max() < 1e-12
    np.testing.assert_allclose(v2, v, rtol=0, atol=1e-14)


def test_rotation_of_a_triangle_with_a_stretch():
    """A rotated rigid triangle whose partners are also pushed outward along their bonds: the constrained step undoes the stretch and
    keeps the rotation only to first order (the correction acts along the OLD bonds); the exact solution satisfies every constraint,
    and the correction is a combination of the old bonds."""
    masses, pos, cons, dist = cc.triangle(None, 15.999, 1.008, 0.1, 104.5)
    im = 1.0 / masses
    R = _rot([0, 0, 1], 0.2)
    delta = pos @ R.T - pos
    delta[1:] += 0.01 * (pos[1:] - pos[0])
    dc, lam = cr.solve_positions(pos, delta, im, cons, dist)
    xn = pos + dc
    for (a, b), d in zip(cons, dist):
        assert abs(np.linalg.norm(xn[a] - xn[b]) - d) < 1e-15
    assert cr.lagrange_residual(pos, delta, dc, im, cons) < 1e-13
    assert cr.momentum_defect(delta, dc, im) < 1e-14


@pytest.mark.parametrize("name", ["hydrogen", "settle_shapes", "general"])
def test_reference_invariants(name):
    """On whole cases: every constraint holds to 1e-14 d^2, the correction moves no centre of mass, exerts no torque about any point, and
    lies in the span of the old bonds; a correction with one wrong mass or along the NEW bonds fails the residual by orders of magnitude."""
    spec, kind = cc.case(name)
    rng = np.random.default_rng(5)
    x, im, d = spec.positions, 1.0 / spec.masses, spec.constraint_distances
    cons = spec.constraints
    for disp in ("thermal", "large"):
        delta = cc.displacement(spec, disp, rng)
        dc, _ = cr.solve_all(x, delta, im, cons, d)
        xn = x + dc
        r2 = ((xn[cons[:, 0]] - xn[cons[:, 1]]) ** 2).sum(1)
        assert np.abs(r2 / (d * d) - 1).max() < 1e-14
        assert cr.lagrange_residual(x, delta, dc, im, cons) < 1e-12
        assert cr.momentum_defect(delta, dc, im) < 1e-13
        for o in ([0, 0, 0], [5.0, -3.0, 1.0]):
            assert cr.angular_momentum_defect(x, delta, dc, im, o) < 1e-12
        v = rng.standard_normal(x.shape)
        v2, _ = cr.solve_all(x, v, im, cons, d, velocities=True)
        assert np.abs(((v2[cons[:, 0]] - v2[cons[:, 1]]) * (x[cons[:, 0]] - x[cons[:, 1]])).sum(1)).max() < 1e-14
        assert cr.lagrange_residual(x, v, v2, im, cons) < 1e-12
        # teeth: the right displacement with one particle's mass wrong, and a correction along the new bonds
        wrong = im.copy()
        j = cons[0, 0]
        wrong[j] *= 2.0
        bad = delta + (dc - delta) * (wrong / im)[:, None]
        assert cr.lagrange_residual(x, delta, bad, im, cons) > 1e-3
        assert cr.lagrange_residual(xn, delta, dc, im, cons) > 1e-4


# ----------------------------------------------------------------------------- the oracle's solvers against the reference
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _oracle(spec, kind, prec, solver, vec, tol):
    """Run one oracle solver on the spec's state with `vec` as the step displacement (positions) or the velocities; returns the result
    and what the solver was handed (x, packed inverse masses, packed distances)."""
    L = O.lib(prec)
    st = O.make_state(spec, prec)
    cm = C.c_float if O.MIXED[prec] == np.float32 else C.c_double
    M = O.MIXED[prec]
    buf = np.zeros((spec.num_atoms, 4), M)
    buf[:, :3] = vec
    velocity = solver.endswith("_v")
    if velocity:
        st["velm"][:, :3] = vec
        buf = st["velm"]
    posq, corr, velm = _ptr(st["posq"]), _ptr(st["posq_corr"]), _ptr(st["velm"])
    if kind == "general":
        atoms, params, _, _ = O.build_general_constraints(spec)
        omega = cm(O.general_relaxation(spec))
        fn = L.vvo_general_velocities if velocity else L.vvo_general_positions
        fn(len(atoms), _ptr(atoms), _ptr(params), cm(tol), omega, posq, corr, _ptr(buf))
    else:
        t = O.build_constraint_clusters(spec)
        if kind == "settle":
            a, p = t["settle_atoms"], t["settle_params"]
            assert len(t["shake_atoms"]) == 0
            if velocity:
                L.vvo_settle_velocities(len(a), _ptr(a), posq, corr, velm)
            else:
                L.vvo_settle_positions(len(a), _ptr(a), _ptr(p), posq, corr, velm, _ptr(buf))
        else:
            a, p = t["shake_atoms"], t["shake_params"]
            assert len(t["settle_atoms"]) == 0
            if solver == "newton":
                L.vvo_cluster_positions_newton(len(a), _ptr(a), _ptr(p), cm(tol), posq, corr, _ptr(buf))
            elif solver == "direct_v":
                L.vvo_cluster_velocities_direct(len(a), _ptr(a), _ptr(p), posq, corr, velm)
            elif solver == "sweeps":
                L.vvo_shake_positions(len(a), _ptr(a), _ptr(p), cm(tol), posq, corr, _ptr(buf))
            elif solver == "sweeps_v":
                L.vvo_shake_velocities(len(a), _ptr(a), _ptr(p), cm(tol), posq, corr, velm)
    x, im, d = cc.solver_view(spec, kind, prec, st["posq"], st["posq_corr"])
    vin = np.asarray(vec, M).astype(np.float64)      # what the solver started from, in its own type
    return buf[:, :3].astype(np.float64), vin, x, im, d


def achieved_tolerance(x, out, inv_mass, cons, dist, velocity):
    """The tolerance a result satisfies in the solvers' own convergence measure: max |r'^2 - d^2| / d^2 for positions; for velocities the
    multiplier the next sweep would apply, max m_red |r . (v_a - v_b)| / |r|^2 (m_red = 1 / (1/m_a + 1/m_b) = 2 avgMass)."""
    a, b = cons[:, 0], cons[:, 1]
    r = x[a] - x[b]
    if velocity:
        mred = 1.0 / (inv_mass[a] + inv_mass[b])
        return float(np.max(np.abs(mred * ((out[a] - out[b]) * r).sum(1)) / (r * r).sum(1)))
    rn = r + out[a] - out[b]
    return float(np.max(np.abs((rn * rn).sum(1) - dist * dist) / (dist * dist)))


SOLVERS = {"cluster": ["newton", "direct_v", "sweeps", "sweeps_v"], "settle": ["settle", "settle_v"], "general": ["general", "general_v"]}
EXACT = {"direct_v", "settle", "settle_v"}       # closed-form algorithms: no tolerance, rounding only

# The one known exception to "every iterative solver reaches its tolerance": the Gauss-Seidel sweeps (OpenMM's SHAKE iteration,
# VVHIP_SHAKE_MODE=0) stop silently after 15 sweeps, and on clusters whose centre is LIGHTER than its peripherals (case
# "hydrogen_masses": 1.5 Da centre, 4 Da hydrogens) 15 sweeps are not enough.  Measured on that case, oracle and kernels alike, at any
# tolerance <= 1e-5: positions |r^2 - d^2| / d^2 up to 2.0e-4 (a step of 20 % of the bond; 2.5e-5 for a thermal one), velocities
# (thermal) a multiplier up to 6.8e-3.  These fixed ceilings replace the tolerance for that case and solver only; everything else is
# held to the tolerance it was asked for.
SWEEP_CAP = {("hydrogen_masses", "sweeps"): 3e-4, ("hydrogen_masses", "sweeps_v"): 1e-2}


def effective_tolerance(case, solver, tol):
    return max(tol, SWEEP_CAP.get((case, solver), 0.0))


def reach_limit(solver, prec, tol, inv_mass, cons, dist, v_max):
    """Largest achieved_tolerance() a converged result may show, from the inputs only:
      * positions: the solvers stop once every |r'^2 - d^2| < tol d^2 in their own arithmetic; recomputing that in float64 adds the
        rounding of |r'|^2 in the `mixed` type, a few eps: tol + 64 eps;
      * velocities: the velocity multiplier is formed from (v_a - v_b) . r in the `mixed` type, whose rounding is eps |v| |r|, i.e.
        m_red eps |v| / |r| on the multiplier (above 1e-5 at thermal velocities in single precision): + 16 eps m_red v_max / d_min.
        The hydrogen-type sweeps apply the last sweep's updates (each <= tol) after checking them, which disturbs a cluster's other
        constraints by at most as much again: 2 tol."""
    eps = np.finfo(O.MIXED[prec]).eps
    if not solver.endswith("_v"):
        return tol + 64 * eps
    mred = (1.0 / (inv_mass[cons[:, 0]] + inv_mass[cons[:, 1]])).max()
    return (2 if solver == "sweeps_v" else 1) * tol + 16 * eps * mred * v_max / np.min(dist)


def bound(solver, prec, tol, d_max, im_max, scale, x_max):
    """Largest |result - exact| (nm or nm/ps) a correct solver may show; `scale` = largest |exact result| of a constrained particle.
      * rounding: the solvers form bonds as differences of positions of size x_max (1 ulp of x_max relative to the bond, amplified
        by the few dozen operations of a solve and by the 1 / |bond| of the correction): 64 eps (x_max / d_max) scale, plus 64 eps
        scale for the result's own arithmetic;
      * positions: a constraint the solver leaves with |r^2 - d^2| < tol d^2 has its length off by tol d / 2; corrections of a
        cluster's other constraints spread that over at most its 16 bonds and the mass ratio: 16 tol d_max;
      * velocities: the sweeps stop once every multiplier |delta| <= tol (mass units / ps), i.e. a velocity change of tol |r| / m per
        remaining update, summed over at most 16 bonds per particle: 16 tol d_max im_max.
    `tol` is the tolerance asked for (effective_tolerance() for the named exception), never one measured on the result."""
    eps = np.finfo(O.MIXED[prec]).eps
    r = 64 * eps * scale * (1 + x_max / d_max)
    if prec == "single":
        r *= 4              # (float positions: the old bonds themselves carry 1 ulp of x_max)
    if solver in EXACT:
        return r
    if solver.endswith("_v"):
        return r + 16 * tol * d_max * im_max
    return r + 16 * tol * d_max


def verify(label, case, solver, prec, tol, spec, x, im, d, vin, out, mask, extra=0.0, worst=None):
    """The checks every solver result passes, oracle and kernels alike; raises AssertionError.  vin = what the solver started from
    (displacement or velocities), out = its result, both float64 [n, 3]; extra = additional rounding of how `out` was read back,
    relative to the result's scale.  Returns the relative distance from the exact solution.
      (a) |out - exact| <= bound() with the tolerance asked for;
      (a') the result satisfies its constraints to that tolerance (achieved_tolerance <= reach_limit): a solver that stopped early,
           or did nothing, fails here even where (a) alone would not see it;
      (b) the correction lies in the span of the old bonds (lagrange_residual), at rounding relative to the result;
      (c) it moves no centre of mass and exerts no torque about any point."""
    cons = spec.constraints
    vel = solver.endswith("_v")
    ref, _ = cr.solve_all(x, vin, im, cons, d, velocities=vel)
    assert np.isfinite(out).all(), label
    err = np.abs(out - ref)[mask].max()
    scale = np.abs(ref[mask]).max()
    teff = effective_tolerance(case, solver, tol)
    b = bound(solver, prec, teff, d.max(), im.max(), scale, np.abs(x).max()) + extra * scale
    if worst is not None:
        key = f"{solver}/{prec}/tol={tol:g}"
        worst[key] = max(worst.get(key, 0.0), err / scale)
    assert err <= b, f"{label}: |result - exact| = {err:.3e} (relative {err / scale:.2e}) > bound {b:.3e}"                                  # (a)
    if solver not in EXACT:
        reached = achieved_tolerance(x, out, im, cons, d, vel)
        lim = reach_limit(solver, prec, teff, im, cons, d, np.abs(out[mask]).max())
        assert reached <= lim, f"{label}: constraints satisfied only to {reached:.2e}, asked {teff:g} (limit {lim:.2e})"                      # (a')
    eps = np.finfo(O.MIXED[prec]).eps
    rel = max(1.0, scale / max(np.abs(out - vin)[mask].max(), 1e-300))      # rounding of the result relative to the correction's size
    res = cr.lagrange_residual(x, vin, out, im, cons)
    if worst is not None:
        worst[f"residual/{solver}/{prec}"] = max(worst.get(f"residual/{solver}/{prec}", 0.0), res)
    assert res < (1e3 * eps + extra) * rel, f"{label}: residual {res:.2e}"                                                                 # (b)
    assert cr.momentum_defect(vin, out, im) < 1e3 * eps * rel, f"{label}: momentum defect"                                                 # (c)
    ang = max(cr.angular_momentum_defect(x, vin, out, im, o) for o in ([0, 0, 0], [4.0, -2.0, 1.0]))
    assert ang < 1e4 * eps * rel, f"{label}: angular momentum defect {ang:.2e}"
    return err / scale


def _displacements(solver):
    # velocity solvers at thermal velocities only: the "large" displacement read as a velocity (~10 nm/ps) puts the float rounding of the
    # velocity multiplier above the tolerance in single precision
    return ("thermal",) if solver.endswith("_v") else ("thermal", "large")


@pytest.mark.parametrize("prec", O.PRECISIONS)
@pytest.mark.parametrize("name", cc.CASES)
def test_oracle_solvers_against_exact_solution(name, prec):
    spec, kind = cc.case(name)
    rng = np.random.default_rng(17)
    mask = cc.constrained(spec)
    for solver in SOLVERS[kind]:
        velocity = solver.endswith("_v")
        for disp in _displacements(solver):
            for tol in ((TOL, TIGHT) if prec != "single" and solver not in EXACT else (TOL,)):
                vec = cc.displacement(spec, disp, rng) / (0.002 if velocity else 1.0)
                out, vin, x, im, d = _oracle(spec, kind, prec, solver, vec, tol)
                verify(f"{name} {solver}/{prec}/tol={tol:g} {disp}", name, solver, prec, tol, spec, x, im, d, vin, out, mask, worst=WORST)
                # particles outside every constraint are not touched
                assert np.array_equal(out[~mask], np.asarray(vec, O.MIXED[prec])[~mask].astype(np.float64))


@pytest.mark.parametrize("name", ["hydrogen", "hydrogen_masses", "settle_apex", "general", "drude_hydrogens"])
def test_verify_rejects_wrong_solvers(name):
    """The checks have teeth: a solver that does nothing, one whose correction uses a wrong mass, and one that corrects along the NEW
    bonds fail verify() in every precision, for positions and velocities alike (built from the exact solution itself, so no solver's
    convergence helps them)."""
    spec, kind = cc.case(name)
    rng = np.random.default_rng(29)
    mask = cc.constrained(spec)
    cons = spec.constraints
    for prec in O.PRECISIONS:
        st = O.make_state(spec, prec)
        x, im, d = cc.solver_view(spec, kind, prec, st["posq"], st["posq_corr"])
        for solver in SOLVERS[kind]:
            vel = solver.endswith("_v")
            vin = np.asarray(cc.displacement(spec, "thermal" if vel else "large", rng) / (0.002 if vel else 1.0), O.MIXED[prec]).astype(np.float64)
            ref, _ = cr.solve_all(x, vin, im, cons, d, velocities=vel)
            wrong = im.copy()
            wrong[cons[:, 0]] *= 1.5
            bad = {"no-op": vin.copy(), "wrong mass": vin + (ref - vin) * (wrong / im)[:, None]}
            if not vel:
                xn = x + ref
                # a correction of the same multipliers along the bonds AFTER the step
                _, lam = cr.solve_all(x, vin, im, cons, d)
                alt = vin.copy()
                for comp, l in lam.items():
                    idx = np.array(comp)
                    local = {g: k for k, g in enumerate(comp)}
                    sel = np.array([int(a) in local for a in cons[:, 0]])
                    lc = np.array([[local[int(a)], local[int(b)]] for a, b in cons[sel]])
                    _, _, W = cr._columns(xn[idx], im[idx], lc)
                    alt[idx] += np.tensordot(l, W, 1)
                bad["new bonds"] = alt
            for what, out in bad.items():
                with pytest.raises(AssertionError):
                    verify(f"{name} {solver}/{prec} {what}", name, solver, prec, TOL, spec, x, im, d, vin, out, mask)


def test_zz_print_worst_errors():
    """Prints the largest relative distance from the exact solution per oracle solver, precision and tolerance (run with -s)."""
    for k in sorted(WORST):
        print(f"  {k:40s} {WORST[k]:.2e}")
