"""-m gpu: the kernels' constraint stages, one launch at a time, against the exact constrained update (tests/constraint_reference.py).

Each test uploads old positions, velocities and a step displacement, runs ONE vvhip_debug_launch and reads back:
  * velocities:          kernel A with the plan's constraint bits (vvhip_debug_fused_flags & A_CONS) -> v' (applyVelocityConstraints);
  * positions, classic:  kernel B with B_VV_POS | the constraint bits -> x + delta_c and v = delta_c / dt (applyConstraints);
  * positions, middle:   kernel B with B_DRIFT_MIDDLE | the constraint bits -> x + delta_c and v + (delta_c - delta) / dt, delta = dt v.
and checks on every constrained particle (a) the result against the exact solution, with a bound from the tolerance asked for, and
(a') that the result satisfies its constraints to that tolerance, (b) that the correction lies in the span of the old bonds
(lagrange_residual), (c) that it moves no centre of mass and exerts no torque, on every other particle (d) bit-identity with the same
launch without the constraint bits, and (e) that the status words stay zero.  (a)-(c): test_constraint_reference.py: verify(), shared
with the oracle's tier.  Layouts: the default one for every case (the Drude case with and without the COM temperature group, which
decides whether Drude pairs and SHAKE mates are merged into units), and the periodic layout forced on for two systems that qualify.  The library adds A_SHAKE_GS / B_SHAKE_GS itself under
VVHIP_SHAKE_MODE=0 (Gauss-Seidel sweeps), and A_MTAB / B_MTAB where the plan keeps mass tables.

Stage sets of single launches like these mostly have no compiled specialisation; the tests run them on the generic kernel (run-time
compilation off), which instantiates the same device solvers.  The one-launch step's constraint variants are pinned bit for bit to the
two-launch step by tests/test_gpu_fused.py."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import constraint_cases as cc
import constraint_reference as cr
from test_constraint_reference import TIGHT, TOL, verify

pkg = importlib.import_module("openmm-velocityverlet_amd")
H, I = pkg.vvhip, pkg.integrator
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# constraint stage bits (csrc/vv_args.hpp); test_constraint_stage_bits_match_the_header keeps these copies honest
A_SHAKE_V, A_SHAKE_GS, A_SETTLE, A_GCONS = 1 << 16, 1 << 21, 1 << 22, 1 << 23
B_SHAKE, B_SHAKE_GS, B_SETTLE, B_GCONS = 1 << 13, 1 << 19, 1 << 20, 1 << 21
A_CONS, B_CONS = A_SHAKE_V | A_SETTLE | A_GCONS, B_SHAKE | B_SETTLE | B_GCONS
DT = 0.002
WORST = {}


def test_constraint_stage_bits_match_the_header():
    """CPU: the stage bits above are those of csrc/vv_args.hpp, and A_CONS / B_CONS are the same unions there."""
    src = open(os.path.join(ROOT, "openmm-velocityverlet_amd", "csrc", "vv_args.hpp")).read()
    for name, value in dict(A_SHAKE_V=A_SHAKE_V, A_SHAKE_GS=A_SHAKE_GS, A_SETTLE=A_SETTLE, A_GCONS=A_GCONS, B_SHAKE=B_SHAKE,
                            B_SHAKE_GS=B_SHAKE_GS, B_SETTLE=B_SETTLE, B_GCONS=B_GCONS, B_VV_POS=H.B_VV_POS, B_DRIFT_MIDDLE=H.B_DRIFT_MIDDLE).items():
        m = re.search(rf"\b{name}\s*=\s*1u\s*<<\s*(\d+)", src)
        assert m, name
        assert 1 << int(m.group(1)) == value, name
    assert re.search(r"A_CONS\s*=\s*A_SHAKE_V\s*\|\s*A_SETTLE\s*\|\s*A_GCONS\s*,\s*B_CONS\s*=\s*B_SHAKE\s*\|\s*B_SETTLE\s*\|\s*B_GCONS", src)


class StageRunner:
    """One plan for a case; uploads state, runs one kernel launch, downloads."""

    def __init__(self, spec, prec, tol=None, tune=None, use_com=None):
        self.spec, self.prec = spec, prec
        self.R, self.M = H.REAL[prec], H.MIXED_T[prec]
        it = I.VVIntegrator(300.0, 10.0, 1.0, 40.0, DT)
        if tol is not None:
            it.setConstraintTolerance(tol)
        if use_com is not None:         # explicit choice: without the COM group, Drude pairs and SHAKE mates are merged into units
            it.setUseCOMTempGroup(use_com)
        self.ctx = I.Context(spec, it, precision=prec, force_provider="static", tune=tune)
        self.plan = self.ctx.plan
        f = C.c_uint32()
        H.check(H.lib.vvhip_debug_fused_flags(self.plan, 0, C.byref(f)), self.plan)
        self.cons_a = f.value & A_CONS
        H.check(H.lib.vvhip_debug_fused_flags(self.plan, 1, C.byref(f)), self.plan)
        self.cons_b = f.value & B_CONS
        n = spec.num_atoms
        self.posq = np.zeros((n, 4), self.R)
        self.posq[:, :3] = spec.positions
        self.corr = np.zeros((n, 4), self.R)
        if prec == "mixed":
            self.corr[:, :3] = spec.positions - self.posq[:, :3].astype(np.float64)
        self.invm = (1.0 / spec.masses).astype(self.M)

    def x(self):
        x = self.posq[:, :3].astype(np.float64)
        return x + self.corr[:, :3].astype(np.float64) if self.prec == "mixed" else x

    def _up(self, arr, a):
        a = np.ascontiguousarray(a)
        H.check(H.lib.vvhip_memcpy_h2d(arr.ptr, a.ctypes.data, a.nbytes), what="h2d")

    def run(self, kernel, flags, v, delta=None):
        """Upload posq / corr, velm = (v, 1/m), pos_delta = delta; one launch; returns (velm, posq, corr) as read back."""
        velm = np.zeros((self.spec.num_atoms, 4), self.M)
        velm[:, :3] = v
        velm[:, 3] = self.invm
        self._up(self.ctx.velm, velm)
        self._up(self.ctx.posq, self.posq)
        if self.prec == "mixed":
            self._up(self.ctx.posq_corr, self.corr)
        pd = np.zeros_like(velm)
        if delta is not None:
            pd[:, :3] = delta
        self._up(self.ctx.pos_delta, pd)
        H.check(H.lib.vvhip_debug_launch(self.plan, kernel, flags, 0), self.plan)
        return self.ctx.getVelm(), self.ctx.getPosq(), self.ctx.getPosqCorrection()

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module", autouse=True)
def _generic_kernels():
    old = I.Context.rtc_mode(0)
    yield
    I.Context.rtc_mode(old)


def _positions_of(prec, posq, corr):
    x = posq[:, :3].astype(np.float64)
    return x + corr[:, :3].astype(np.float64) if prec == "mixed" else x


def _check(label, case, solver, prec, tol, spec, x, im, d, vin, out, status, mask, extra=0.0):
    """verify() (tests/test_constraint_reference.py: (a) exact solution with the tolerance asked for, (a') constraints satisfied to it,
    (b) residual, (c) momentum) and (e) the status words: zero for every solver -- the one known exception, the sweeps' silent cap
    (SWEEP_CAP), does not report one either."""
    verify(label, case, solver, prec, tol, spec, x, im, d, vin, out, mask, extra=extra, worst=WORST)
    assert status == [0, 0, 0, 0], f"{label}: status words {status}"                                                                         # (e)


def _solvers(kind, gs):
    if kind == "cluster":
        return ("sweeps_v", "sweeps") if gs else ("direct_v", "newton")
    return {"settle": ("settle_v", "settle"), "general": ("general_v", "general")}[kind]


def _params():
    """Cases x precisions x solver modes (VVHIP_SHAKE_MODE selects the hydrogen-type clusters' solver only) x tolerances (1e-10 only
    where the mixed type resolves it), in the default layout; the Drude case with and without the COM temperature group; and the
    periodic layout forced on (VVHIP_PERIODIC=1) with role words computed (tune periodic_kernels=1) and loaded (=0), in mixed precision
    as tests/test_gpu_periodic.py runs it."""
    out = []
    for name in cc.CASES:
        kind = cc.case(name)[1]
        for prec in ("single", "mixed", "double"):
            for mode in (("default", "sweeps") if kind == "cluster" else ("default",)):
                for tight in ((False, True) if prec != "single" else (False,)):
                    for com in ((True, False) if name == "drude_hydrogens" else (None,)):
                        tag = "" if com is None else ("-com" if com else "-nocom")
                        out.append(pytest.param(name, prec, mode, tight, "default", com,
                                                id=f"{name}-{prec}-{mode}-{'tight' if tight else 'default_tol'}{tag}"))
    # The periodic layout only with the COM group: without it the plan's units are Drude pairs merged with their SHAKE mates, which in
    # the reference topology are not consecutive particles, and the layout refuses them (csrc/vv_host.cpp: try_periodic) -- such a plan
    # keeps the default layout, which drude_hydrogens-*-nocom covers.
    for name in cc.PERIODIC_CASES:
        for pk in (1, 0):
            com = True if name == "periodic_hbonds" else None
            out.append(pytest.param(name, "mixed", "default", False, f"periodic{pk}", com, id=f"{name}-mixed-periodic_kernels{pk}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,prec,mode,tight,layout,com", _params())
def test_constraint_stages_against_exact_solution(name, prec, mode, tight, layout, com, monkeypatch):
    spec, kind = cc.case(name)
    monkeypatch.setenv("VVHIP_SHAKE_MODE", "0" if mode == "sweeps" else "1")
    monkeypatch.delenv("VVHIP_PERIODIC", raising=False)
    tune = None
    if layout.startswith("periodic"):
        monkeypatch.setenv("VVHIP_PERIODIC", "1")
        tune = {"periodic_kernels": int(layout[-1])}
    tol = TIGHT if tight else TOL
    run = StageRunner(spec, prec, tol=tol, tune=tune, use_com=com)
    try:
        if layout.startswith("periodic"):
            assert run.ctx.info.periodic_layout == 1, f"{name}: layout not recognised as periodic"
        assert run.ctx.info.constraints_fused, f"{name}: the plan does not solve these constraints in the kernels"
        assert run.cons_a and run.cons_b
        sv, sp = _solvers(kind, mode == "sweeps")
        x = run.x()
        _, im, d = cc.solver_view(spec, kind, prec, run.posq, run.corr)
        mask = cc.constrained(spec)
        M = run.M
        rng = np.random.default_rng(23)
        for disp in ("thermal", "large"):
            delta = cc.displacement(spec, disp, rng)
            v = (delta / DT).astype(M)
            label = f"{name}/{prec}/{mode}/{layout}/com={com}/tol={tol:g}/{disp}"
            # velocities: kernel A, constraint bits only -- at thermal velocities (test_constraint_reference.py: _displacements)
            if disp == "thermal":
                run.ctx.status_clear()
                va, _, _ = run.run(0, run.cons_a, v)
                st = run.ctx.status_words()
                va0, _, _ = run.run(0, 0, v)
                assert np.array_equal(va[~mask], va0[~mask]), f"{label}: unconstrained velocities changed"                                # (d)
                _check(label + "/vel", name, sv, prec, tol, spec, x, im, d, v.astype(np.float64), va[:, :3].astype(np.float64), st, mask)
            # positions, classic: x += delta_c, v = delta_c / dt
            dm = delta.astype(M)
            run.ctx.status_clear()
            vb, pb, cb = run.run(1, H.B_VV_POS | run.cons_b, v, dm)
            st = run.ctx.status_words()
            vb0, pb0, cb0 = run.run(1, H.B_VV_POS, v, dm)
            assert np.array_equal(vb[~mask], vb0[~mask]) and np.array_equal(pb[~mask], pb0[~mask]) and np.array_equal(cb[~mask], cb0[~mask]), \
                f"{label}: unconstrained particles changed"                                                                              # (d)
            dc = vb[:, :3].astype(np.float64) * DT                     # v = (1/dt) delta_c, rounded in the mixed type
            _check(label + "/classic", name, sp, prec, tol, spec, x, im, d, dm.astype(np.float64), dc, st, mask, extra=4 * np.finfo(M).eps)
            xn = _positions_of(prec, pb, cb)
            assert np.abs(xn - (x + dc))[mask].max() <= 4 * np.finfo(H.REAL[prec]).eps * np.abs(x).max() + 4 * np.finfo(M).eps * np.abs(dc).max(), \
                f"{label}: positions are not x + delta_c"
            # positions, middle: delta = dt/2 v + dt/2 v, x += delta_c, v += (delta_c - delta) / dt
            half = M(0.5) * M(DT)
            d_mid = (half * v + half * v).astype(np.float64)
            run.ctx.status_clear()
            vm, pm, cm = run.run(1, H.B_DRIFT_MIDDLE | run.cons_b, v)
            st = run.ctx.status_words()
            vm0, pm0, cm0 = run.run(1, H.B_DRIFT_MIDDLE, v)
            assert np.array_equal(vm[~mask], vm0[~mask]) and np.array_equal(pm[~mask], pm0[~mask]) and np.array_equal(cm[~mask], cm0[~mask]), f"{label}: unconstrained particles changed"   # (d)
            dcm = d_mid + (vm[:, :3].astype(np.float64) - v.astype(np.float64)) * DT
            _check(label + "/middle", name, sp, prec, tol, spec, x, im, d, d_mid, dcm, st, mask, extra=8 * np.finfo(M).eps * np.abs(v).max() * DT / np.abs(d_mid[mask]).max())
            xm = _positions_of(prec, pm, cm)
            assert np.abs(xm - (x + dcm))[mask].max() <= 4 * np.finfo(H.REAL[prec]).eps * np.abs(x).max() + 8 * np.finfo(M).eps * np.abs(d_mid).max(), \
                f"{label}: positions are not x + delta_c"
    finally:
        run.close()


@pytest.mark.gpu
def test_zz_print_worst_errors():
    """Largest relative distance from the exact solution per device solver, precision and tolerance (run with -s)."""
    for k in sorted(WORST):
        print(f"  {k:40s} {WORST[k]:.2e}")
