"""-m gpu: the device's Nose-Hoover chain (csrc/vv_dev_chain.inc) against the exact reference of tests/chain_reference.py, over the table of
tests/chain_cases.py (tests/test_chain_reference.py shows on the CPU that the reference's bound holds honest fp64 evaluations, convicts a
wrong x^8 coefficient, and that every case reaches its band).

Per case and entry point -- one thermostat application through vvhip_scale_velocity ("scale"), one inside vvhip_step_middle ("middle"), the
two of vvhip_step_vv_first / vvhip_step_vv_second ("classic", bands up to 1 like "middle") -- the start velocities and positions are uploaded
again, the case's chain state is written with setNHState, and after EACH call getNHState gives the state the application left.  2KE is what
the device reports (exactly what its chain consumed), dof kT and the thermostat masses come from ctx.info; chain_reference evaluates the
application exactly on these inputs and vscale, eta, eta_dot, eta_dotdot of every active group must lie within 2 x its bound (the factor 2
for the second-order terms of a first-order analysis; the errors this is after are a hundred times larger).  A group the system does not have
keeps the bits that were set and gets vscale 1.0 exactly.

The case's start values depend on 2KE (chain_cases.start), which only the device knows: a case is run, resolved again with the 2KE it
reported and run again until the two agree (one extra pass per entry point and context in practice: 2KE does not depend on the chain's
state).  "scale" must get there, and its point bands (the doubles next to 2^-4 and 2^-3) are then hit exactly: chain_cases.ke_scale puts
the start's 2KE on the side of its target where the sum eta_dot[0] + eta_dotdot[0] dt/4 can be every double.  Inside whole steps the kick
in front of the thermostat moves 2KE and with it decides that side, and on the wrong one the sums skip doubles: there a
point band of the "factor" target counts as reached within 2 ulps ("prefix" targets do not depend on 2KE and stay exact).  A pass may also
see another 2KE than the one before (what a previous step left in the cos perturbation's caches); a point band then counts as reached
within 1e-6 of the point.  In the classic scheme the chain state is written again in front of the second half: the state the first
half leaves from an argument of 1 would hand the second half arguments far beyond 8 (chain_cases' docstring).

A context lives for a whole family of cases (one system, one chain length, one path), so kernels compiled at run time are compiled once."""
import dataclasses
import importlib
import math

import numpy as np
import pytest

import chain_cases as K
import chain_reference as R
import param_range_cases as P
from oracle import oracle as O

pkg = importlib.import_module("openmm-velocityverlet_amd")
H, I = pkg.vvhip, pkg.integrator
pytestmark = pytest.mark.gpu

LIMIT = 2.0                       # x bound
_START, _REF, _KE2 = {}, {}, {}   # shared between contexts: start values and references per (case, group, 2KE); the 2KE last seen per entry point
WORST = {}                        # path -> (ratio, where): printed by every test for its path


@pytest.fixture(autouse=True)
def _restore_mode():
    old = I.Context.rtc_mode()
    yield
    I.Context.rtc_mode(old)


def _start(case, g, ke2, nkbt, mass):
    key = (case, g, ke2, nkbt, tuple(mass))
    if key not in _START:
        _START[key] = K.start(case, g, ke2, nkbt, mass)
    return _START[key]


def _reference(case, g, ke2, nkbt, mass, state):
    key = (case.nc, case.loops, g, ke2, nkbt, tuple(mass), tuple(map(tuple, state)), case.t_target(g))
    if key not in _REF:
        inp = (case.nc, case.loops, case.step_size, *state, mass, ke2, nkbt, case.t_target(g))
        _REF[key] = (R.reference(*inp), R.chain_fp64(*inp))
    return _REF[key]


class Env:
    """One device context for a family of cases."""

    def __init__(self, path, system, nc, tune=None, cos=0.0, rtc=None):
        if rtc is not None:
            I.Context.rtc_mode(rtc)
        self.path, self.system, self.nc, self.cos = path, system, nc, cos
        self.spec = K.spec_of(system)
        self.it = K.integrator_of(system, nc, cos=cos)
        self.ctx = I.Context(self.spec, self.it, precision="mixed", force_provider="tether", tune=tune)
        info = self.ctx.info
        self.groups = info.num_temp_groups
        assert self.groups == K.SYSTEMS[system]["groups"]
        self.nkbt = [float(x) for x in info.nkbt]
        self.mass = [[float(x) for x in row][:nc] for row in info.eta_mass]
        self.velm0, self.posq0, self.corr0 = self.ctx.getVelm(), self.ctx.getPosq(), self.ctx.getPosqCorrection()
        self.blank = self.ctx.getNHState()
        self.shape = None
        self.inexact = 0
        self.violations = []        # collected over the family and asserted together (finish): one run shows every case that is out

    def close(self):
        self.ctx.close()

    def configure(self, case, middle):
        shape = (case.loops, middle)
        if shape != self.shape:
            self.it._loopsPerStep, self.it._stepSize, self.it._useMiddleScheme = case.loops, case.step_size, middle
            self.ctx._set_params()
            self.shape = shape

    def start_velm(self, case):
        v = self.velm0.copy()
        v[:, :3] *= math.sqrt(K.ke_scale(case))
        return v

    def reset(self, case):
        self.ctx.synchronize()
        self.ctx.velm.upload(self.start_velm(case))
        self.ctx.posq.upload(self.posq0)
        self.ctx.posq_corr.upload(self.corr0)
        self.ctx.forces_valid = False

    def state_for(self, case, ke2):
        """(NHState to write, the start values per active group) for the 2KE the chain is expected to be handed."""
        st = H.NHState.from_buffer_copy(bytes(self.blank))
        starts = []
        for g in range(3):
            if g < self.groups:
                eta, eta_dot, eta_dotdot = _start(case, g, ke2[g], self.nkbt[g], self.mass[g])
                starts.append((list(eta), list(eta_dot), list(eta_dotdot)))
            else:                   # a group the system does not have: finite values that must come back bit for bit
                eta = [0.5 + i for i in range(self.nc)]
                eta_dot = [case.inactive_eta_dot * (1 + g + i) for i in range(self.nc)]
                eta_dotdot = [-7.0 * (i + 1) for i in range(self.nc)]
                st.ke2[g], st.vscale[g] = 321.0 + g, 0.75
            for i in range(self.nc):
                st.eta[g][i], st.eta_dot[g][i], st.eta_dotdot[g][i] = eta[i], eta_dot[i], eta_dotdot[i]
        return st, starts

    def apply(self, case, entry, guesses):
        """Runs the entry point from the case's state, resolved for the 2KE in `guesses` (one list per application).  Returns per
        application (state written, start values, state read back) and the velocities at the end."""
        L, plan, ctx = H.lib, self.ctx.plan, self.ctx
        self.configure(case, entry != "classic")
        self.reset(case)
        out = []
        set0, starts0 = self.state_for(case, guesses[0])
        if entry == "scale":
            ctx.setNHState(set0)
            H.check(L.vvhip_scale_velocity(plan), plan)
            out.append((set0, starts0, ctx.getNHState()))
        elif entry == "middle":
            ctx.calcForces()
            ctx.setNHState(set0)
            H.check(L.vvhip_step_middle(plan, 0), plan)
            out.append((set0, starts0, ctx.getNHState()))
        else:
            ctx.calcForces()
            ctx.setNHState(set0)
            H.check(L.vvhip_step_vv_first(plan), plan)
            out.append((set0, starts0, ctx.getNHState()))
            ctx.calcForces()
            set1, starts1 = self.state_for(case, guesses[1])
            ctx.setNHState(set1)
            H.check(L.vvhip_step_vv_second(plan, 0), plan)
            out.append((set1, starts1, ctx.getNHState()))
        return out, ctx.getVelm()

    def run(self, case, entry):
        """Runs the case until the 2KE it was resolved for is the 2KE the device reports; checks every application.  Returns what `apply`
        returns (for comparisons between contexts)."""
        napps = 2 if entry == "classic" else 1
        keys = [(self.system, self.cos, entry, a, K.ke_scale(case), case.loops, case.name if a else "") for a in range(napps)]
        guesses = [_KE2.get(k, [K.nominal_ke2(case, self.nkbt[g], g) for g in range(self.groups)]) for k in keys]
        exact = False
        for attempt in range(4):
            apps, velm = self.apply(case, entry, guesses)
            seen = [[float(st.ke2[g]) for g in range(self.groups)] for _, _, st in apps]
            if seen == guesses:
                exact = True
                break
            guesses = seen
        for k, s in zip(keys, seen):
            _KE2[k] = s
        assert exact or entry != "scale", (case.name, "2KE of the same velocities changed between two applications", guesses, seen)
        self.inexact += 0 if exact else 1
        for a, (written, starts, got) in enumerate(apps):
            self.check(case, f"{entry}[{a}]", written, starts, got, exact)
        return apps, velm

    def check(self, case, where, written, starts, got, exact):
        nc = self.nc
        for g in range(3):
            if g >= self.groups:
                for name in ("eta", "eta_dot", "eta_dotdot"):
                    a, b = list(getattr(got, name)[g]), list(getattr(written, name)[g])
                    assert [x.hex() for x in a[:nc]] == [x.hex() for x in b[:nc]], (case.name, where, g, name, a, b)
                assert got.ke2[g] == written.ke2[g] and got.vscale[g] == 1.0, (case.name, where, g, got.ke2[g], got.vscale[g])
                continue
            ke2 = float(got.ke2[g])
            assert math.isfinite(ke2) and ke2 > 0
            ref, plain = _reference(case, g, ke2, self.nkbt[g], self.mass[g], starts[g])
            slack = 0
            if case.band_of(g) in K.POINTS:
                if not exact:
                    slack = 2.0 ** 46           # 1e-6 of the point, in ulps
                elif case.target == "factor" and not where.startswith("scale"):
                    slack = 2                   # (the kick has decided whether eta_dot[0] + eta_dotdot[0] dt / 4 can be that double: see the docstring)
            if not K.reaches_its_band(case, g, plain["args"], slack_ulps=slack):
                self.violations.append(f"{case.name} {where} group {g}: misses its band, named argument {dict(plain['args'])[case.label()]!r}")
            if max(abs(float(x)) for _, x in ref["args"]) > K.MAX_ARGUMENT:
                self.violations.append(f"{case.name} {where} group {g}: an argument beyond {K.MAX_ARGUMENT}")
            dev = dict(factor=got.vscale[g], eta=list(got.eta[g])[:nc], eta_dot=list(got.eta_dot[g])[:nc], eta_dotdot=list(got.eta_dotdot[g])[:nc])
            assert got.eta_dot[g][nc] == 0.0
            for (name, d), (_, r) in zip(R.quantities(dev), R.quantities(ref)):
                ratio = R.ratio(d, r)
                if ratio > WORST.get(self.path, (0.0, ""))[0]:
                    WORST[self.path] = (ratio, f"{case.name} {where} group {g} {name}")
                if not ratio <= LIMIT:
                    self.violations.append(f"{case.name} {where} group {g} {name}: device {float(d)!r} exact {float(r.v)!r} |difference| / bound {ratio:.3f}")

    def finish(self):
        w = WORST.get(self.path, (0.0, ""))
        assert not self.violations, f"{self.path}: {len(self.violations)} violations, worst ratio {w[0]:.3f} ({w[1]}):\n" + "\n".join(self.violations[:40])
        assert self.ctx.status_words() == [0, 0, 0, 0], self.ctx.status_words()
        print(f"{self.path}: worst |device - exact| / bound so far {w[0]:.3f} ({w[1]}); cases of {self.system} nc={self.nc} that met a changed 2KE: {self.inexact}")


def _cases(system, nc, entry):
    cases = K.family(system, nc)
    assert cases
    return cases if entry == "scale" else [c for c in cases if c.full_step()]


def _run_family(env, entry, close=True):
    try:
        n = 0
        for case in _cases(env.system, env.nc, entry):
            env.run(case, entry)
            n += 1
        assert n == len(_cases(env.system, env.nc, entry))
        env.finish()
    except BaseException:
        env.close()
        raise
    if close:
        env.close()


def _same_bits(case, a, b, what):
    (apps_a, velm_a), (apps_b, velm_b) = a, b
    for (_, _, sa), (_, _, sb) in zip(apps_a, apps_b):
        assert bytes(sa) == bytes(sb), f"{case.name}: thermostat state differs between {what}"
    assert np.array_equal(velm_a.view(np.uint8), velm_b.view(np.uint8)), f"{case.name}: velocities differ between {what}"


# ---- kernel B's chain with the compiled chain length: one launch and two launches, bit for bit the same
@pytest.mark.parametrize("entry", ["scale", "middle", "classic"])
@pytest.mark.parametrize("system", ["il", "water", "il_large"])
def test_kernel_b_chain_in_the_one_launch_and_the_two_launch_step(system, entry):
    """chain_prefix + propagate_preloaded + the redo, three links.  For the water system (one temperature group, no COM group) the factor
    must have reached the tile waves: every velocity component after "scale" is fp64 v * vscale.  For the 2 590-particle box (several
    blocks, each running its own chain, block 0 recording) the step is also compared with the oracle started from the same chain state,
    at tests/test_gpu_edges._assert_close's tolerance."""
    one = Env("one launch", system, 3, tune={"fused": 1})
    two = Env("two launches", system, 3, tune={"fused": 0})
    try:
        for case in _cases(system, 3, entry):
            a = one.run(case, entry)
            b = two.run(case, entry)
            _same_bits(case, a, b, "the one-launch and the two-launch step")
            if entry == "middle":
                active, launches = one.ctx.fused_status()
                assert (active and launches > 0) or system == "il_large", (active, launches)
                assert two.ctx.fused_status() == (False, 0)
            if system == "water" and entry == "scale":
                v0, v1, s = one.start_velm(case)[:, :3], a[1][:, :3], float(a[0][0][2].vscale[0])
                assert np.array_equal(v1, v0 * s), (case.name, np.abs(v1 / (v0 * s) - 1).max())
            if system == "il_large" and entry == "middle":
                _against_the_oracle(one, case, a)
        one.finish()
        two.finish()
    finally:
        one.close()
        two.close()


def _against_the_oracle(env, case, res):
    """One middle-scheme step of the oracle from the same velocities and the same chain state."""
    from test_gpu_edges import _assert_close
    s = K.SYSTEMS[env.system]
    spec = dataclasses.replace(env.spec, velocities=env.spec.velocities * math.sqrt(K.ke_scale(case)))
    p = O.Params(temperature=s["temperature"], frequency=s["frequency"], drude_temperature=s["drude_temperature"], drude_frequency=s["drude_frequency"],
                 step_size=case.step_size, loops_per_step=case.loops, num_chains=case.nc, max_drude_distance=0.02, use_middle_scheme=True)
    osys = O.OracleSystem(spec, p, "mixed", force_mode=1)
    written = res[0][0][0]
    for g in range(3):
        for i in range(case.nc):
            osys.s.eta[g][i], osys.s.eta_dot[g][i], osys.s.eta_dotdot[g][i] = written.eta[g][i], written.eta_dot[g][i], written.eta_dotdot[g][i]
    osys.step(1)
    _assert_close(osys, env.ctx)


# ---- chain lengths 1, 2 and 4: a kernel compiled at run time for the plan's length, and the generic kernel (chain length a run-time value)
# (run-time compiles cost seconds each: the run-time route takes the single application and the one-launch step, the generic kernel all three)
OTHER_LENGTHS = [(nc, how, entry) for nc in (1, 2, 4) for how, entries in (("rtc", ("scale", "middle")), ("generic", ("scale", "middle", "classic")))
                 for entry in entries]


@pytest.mark.parametrize("nc,how,entry", OTHER_LENGTHS)
def test_other_chain_lengths_in_kernel_b(nc, how, entry):
    env = Env(f"chain length 1/2/4, {how}", "il", nc, rtc=1 if how == "rtc" else 0)
    try:
        _run_family(env, entry, close=False)
        counts, sets = env.ctx.generic_launches()
        assert (counts == (0, 0)) if how == "rtc" else counts[1] > 0, (how, counts, [hex(x) for x in sets])
    finally:
        env.close()


@pytest.mark.parametrize("entry", ["scale", "middle"])
@pytest.mark.parametrize("nc", [1, 2, 4])
def test_inactive_groups_in_the_generic_kernel(nc, entry):
    """The water system's two missing groups carry large finite chain velocities: their lanes compute but must not vote for the redo, and
    their state comes back bit for bit."""
    _run_family(Env("inactive groups, generic", "water", nc, rtc=0), entry)


# ---- the stand-alone chain launch (propagate_regs): small systems sent there by the test hook, and chain lengths 5 and 8
STAND_ALONE = ([("il", nc, entry) for nc in (3, 5, 8) for entry in ("scale", "middle", "classic")]
               + [("water", nc, entry) for nc in (3, 5, 8) for entry in ("scale", "middle")] + [("il_large", 5, "scale"), ("il_large", 5, "middle")])


@pytest.mark.parametrize("system,nc,entry", STAND_ALONE)
def test_stand_alone_chain(system, nc, entry):
    _run_family(Env("stand-alone chain", system, nc, tune={"split_chain_waves": 1}), entry)


# ---- the cos acceleration: in its moment form (kernel B's chain on 2KE rebuilt from moments) and as three launches (stand-alone chain, C_BIAS)
@pytest.mark.parametrize("entry", ["middle", "classic"])
@pytest.mark.parametrize("form", ["moments", "three launches"])
def test_cos_acceleration(form, entry):
    _run_family(Env(f"cos, {form}", "il", 3, tune={"no_moments": 0 if form == "moments" else 1}, cos=0.02), entry)


# ---- a walk
def test_stiff_walk_restarted_from_the_device_state_at_every_step():
    """tests/param_range_cases.py's "stiff_loops3" (200 / 800 per ps, three loops, 2 590 particles) for 30 steps, one at a time; at every step
    the reference starts from the device's own previous state, so nothing accumulates, and the bound must hold.  Prints the steps that had an
    argument beyond 2^-4 or 2^-3.  On the MI355X every one of the 30 steps has an argument beyond 2^-3 (the largest is 0.40), so every
    step of the walk takes the redo with the library exp; worst |device - exact| / bound 0.48."""
    c = P.case("stiff_loops3")
    it = c.integrator(True, 0.0)
    ctx = I.Context(c.spec, it, precision="mixed", force_provider="tether", k_tether=c.k_tether, k_drude=c.k_drude)
    try:
        nkbt = [float(x) for x in ctx.info.nkbt]
        mass = [[float(x) for x in row][:3] for row in ctx.info.eta_mass]
        beyond4, beyond3, largest, worst = [], [], 0.0, (0.0, "")
        prev = ctx.getNHState()
        for step in range(30):
            it.step(1)
            got = ctx.getNHState()
            for g in range(3):
                T = c.drude_temperature if g == 2 else c.temperature
                ref = R.reference(3, c.loops_per_step, c.step_size, list(prev.eta[g])[:3], list(prev.eta_dot[g])[:3], list(prev.eta_dotdot[g])[:3],
                                  mass[g], float(got.ke2[g]), nkbt[g], T)
                top = max(abs(float(a)) for _, a in ref["args"])
                largest = max(largest, top)
                if top > K.P4 and step not in beyond4:
                    beyond4.append(step)
                if K.high_word(top) > K.SMALL_HI and step not in beyond3:
                    beyond3.append(step)
                dev = dict(factor=got.vscale[g], eta=list(got.eta[g])[:3], eta_dot=list(got.eta_dot[g])[:3], eta_dotdot=list(got.eta_dotdot[g])[:3])
                r, name = R.worst_ratio(dev, ref)
                worst = max(worst, (r, f"step {step} group {g} {name}"))
                assert r <= LIMIT, (step, g, name, r)
            prev = got
        print(f"stiff walk: largest |argument| {largest:.4f}; steps beyond 2^-4: {beyond4}; beyond 2^-3: {beyond3}; worst |device - exact| / bound {worst[0]:.3f} ({worst[1]})")
        assert ctx.status_words() == [0, 0, 0, 0]
    finally:
        ctx.close()
