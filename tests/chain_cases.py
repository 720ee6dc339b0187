"""A table of Nose-Hoover chain states whose exp arguments land where the device's chain changes its path, for
tests/test_chain_reference.py (CPU: every case reaches the band it names, by the exact reference alone) and tests/test_gpu_chain.py (the
device against the exact reference).  Test code only.

The device evaluates exp(x) with a degree-11 polynomial up to |x| = 2^-4 (stand-alone chain) or 2^-3 (kernel B's thermostat wave, which
redoes the whole application with the library exp when the high word of any |x| exceeded that of 2^-3), csrc/vv_dev_chain.inc.  A case
names ONE exp evaluation of the reference's sequence (chain_reference: ("factor", loop), ("down", loop, link), ("up", loop, link)) and the
band of |x| it must land in, in the temperature groups listed in `hot`; the other groups stay small.  Targets:

    "factor"   -dt/2 eta_dot[0] of the first loop: the scale factor's own exp;
    "prefix"   the first loop's -dt/8 eta_dot[2] in front of link 1 (chain length 2: -dt/8 eta_dot[1] in front of link 0): an exp that
               kernel B evaluates before the kinetic energy exists (chain_prefix);
    "late"     -dt/8 eta_dot[1] in front of link 0 in the SECOND of three loops: the first loop stays inside 2^-3, the coupling
               eta_dotdot[1] = dof eta_dot[0]^2 - f^2 then carries link 1 out of it, so the range test fires after a loop of fast evaluations.

The start values depend on the kinetic energy the chain will be handed (eta_dotdot[0] is recomputed from it), so a case is resolved
against (2KE, dof kT, the thermostat masses) by `start()`: a bisection on the float line over the plain fp64 chain (chain_reference.chain_fp64)
until the named argument IS the band's double (point bands) or sits at the band's aim (intervals).  The steps are powers of two (dt/2 =
2^-11 with one loop, 2^-13 with three) so that -dt/2 x and -dt/8 x are exact.  Point bands keep the link above the target at rest (its exp
is exactly 1): a product with a rounded exp skips doubles.

What is left out, by rule and not at run time.  Chain lengths of two or more couple link 1 to eta_dot[0]: eta_dotdot[1] = dof eta_dot[0]^2 -
f^2 enters link 1 twice before the next loop evaluates -dt/8 eta_dot[1], which is A = dof x^2 / 4 for a factor argument x, and every link hands
4 A^2 to the next one.  Above A = 1 / 4 that runs away (the reference reaches arguments of 1e19 within three loops of eight links, and
overflows).  With three loops and two or more links the "factor" target therefore stops at 2^-4, the bands up to the next double above 2^-3
are reached by the "prefix" target, and what lies beyond by the "late" target, whose named argument is held at 0.16, inside (2^-3, 1 / 4).
An argument of 4 with three loops drives a single link past 8 as well (2KE e^8).  tests/test_chain_reference.py asserts that every case of
the table, by the reference alone, keeps every argument at or below 8 and every quantity finite."""
import dataclasses
import math
import struct

import chain_reference as R

P4, P3 = 2.0 ** -4, 2.0 ** -3
SMALL_HI = 0x3FC00000                                                   # csrc/vv_dev_chain.inc: CHAIN_EXP_SMALL_HI, the high word of 2^-3
FIRST_HI = struct.unpack("<d", struct.pack("<Q", (SMALL_HI + 1) << 32))[0]      # the first double whose high word exceeds it
MAX_ARGUMENT = 8.0

# name -> (lowest |x|, highest |x|, the |x| the solver aims at); a point band has all three equal
BANDS = {
    "tiny": (math.ulp(0.0), 2.0 ** -6, 2.0 ** -9),
    "mid": (math.nextafter(2.0 ** -6, 1), math.nextafter(P4, 0), 2.0 ** -5),
    "below_2^-4": (math.nextafter(P4, 0),) * 3,
    "above_2^-4": (math.nextafter(P4, 1),) * 3,
    "upper": (math.nextafter(P4, 1), math.nextafter(P3, 0), 0.1),
    "2^-3": (P3,) * 3,
    "next_2^-3": (math.nextafter(P3, 1),) * 3,
    "first_hi": (FIRST_HI,) * 3,
    "0.3": (0.3 * (1 - 2.0 ** -10), 0.3 * (1 + 2.0 ** -10), 0.3),
    "1": (1 - 2.0 ** -10, 1 + 2.0 ** -10, 1.0),
    "4": (4 * (1 - 2.0 ** -10), 4 * (1 + 2.0 ** -10), 4.0),
    "beyond": (FIRST_HI, 0.25, 0.16),                                   # ("late" cases: above 1 / 4 the coupling runs away, see _table)
}
POINTS = [b for b, (lo, hi, _) in BANDS.items() if lo == hi]
IN_RANGE = ["tiny", "mid", "below_2^-4", "above_2^-4", "upper", "2^-3", "next_2^-3"]      # kernel B's fast exp serves them
OUT_OF_RANGE = ["first_hi", "0.3", "1", "4"]                                              # the redo with the library exp
SENSITIVE = ["upper", "2^-3"]                                                             # (2^-4, 2^-3]: where a wrong x^8 term shows
STEP = {1: 2.0 ** -10, 3: 3 * 2.0 ** -12}                                                 # ps; dt/2 = 2^-11 and 2^-13
assert STEP[1] / 1 / 2 == 2.0 ** -11 and STEP[3] / 3 / 2 == 2.0 ** -13

# the systems of tests/test_gpu_chain.py: temperatures [K] and thermostat frequencies [1/ps] they are created with (the thermostat masses
# are fixed at creation) and the temperature groups they have
SYSTEMS = {
    "il": dict(temperature=333.0, drude_temperature=1.0, frequency=10.0, drude_frequency=40.0, groups=3),
    "il_large": dict(temperature=333.0, drude_temperature=1.0, frequency=10.0, drude_frequency=40.0, groups=3),
    "water": dict(temperature=300.0, drude_temperature=1.0, frequency=10.0, drude_frequency=40.0, groups=1),
}
HOT = {"all": (0, 1, 2), "g0": (0,), "g2": (2,)}


def high_word(x):
    return (struct.unpack("<Q", struct.pack("<d", abs(x)))[0] >> 32) & 0x7FFFFFFF


def in_band(band, x, slack_ulps=0):
    """|x| lies in the band (a point band: within slack_ulps ulps of the point)."""
    lo, hi, _ = BANDS[band]
    return lo - slack_ulps * math.ulp(lo) <= abs(x) <= hi + slack_ulps * math.ulp(hi)


@dataclasses.dataclass(frozen=True)
class Case:
    system: str
    nc: int                    # chain length
    loops: int                 # loops per step
    target: str                # "factor", "prefix", "late" (above)
    band: str
    sign: int                  # sign of the named argument
    hot: str = "all"           # groups that carry the band (HOT); the others get "tiny"
    inactive_eta_dot: float = 0.0      # != 0: written into the chain of the groups the system does not have (they must come back untouched)

    @property
    def name(self):
        return f"{self.system}-nc{self.nc}-loops{self.loops}-{self.target}-{self.band}-{'pos' if self.sign > 0 else 'neg'}-{self.hot}"

    @property
    def step_size(self):
        return STEP[self.loops]

    @property
    def groups(self):
        return SYSTEMS[self.system]["groups"]

    def t_target(self, g):
        s = SYSTEMS[self.system]
        return s["drude_temperature"] if g == 2 else s["temperature"]

    def label(self):
        """The evaluation the case names (a label of chain_reference's argument list)."""
        if self.target == "factor":
            return ("factor", 0)
        if self.target == "prefix":
            return ("down", 0, 1 if self.nc >= 3 else 0)
        return ("down", 1, 0)

    def band_of(self, g):
        return self.band if g in HOT[self.hot] else "tiny"

    def full_step(self):
        """Also run inside whole steps: the bands up to 1."""
        return self.band != "4"


def _key(x):                   # floats in their order, as integers
    k = struct.unpack("<q", struct.pack("<d", x))[0]
    return k if k >= 0 else -(k & 0x7FFFFFFFFFFFFFFF)


def _unkey(k):
    return struct.unpack("<d", struct.pack("<q", k if k >= 0 else (-k) | -0x8000000000000000))[0]


def _solve(fn, want):
    """s with fn(s) == want, or as close as the float line allows; fn is monotone and close to affine."""
    f0, f1 = fn(0.0), fn(1.0)
    s = (want - f0) / (f1 - f0)
    rising = f1 > f0
    width = abs(s) * 2.0 ** -40 + 2.0 ** -60
    lo, hi = _key(s - width), _key(s + width)
    assert (fn(_unkey(lo)) <= want <= fn(_unkey(hi))) if rising else (fn(_unkey(lo)) >= want >= fn(_unkey(hi))), "no bracket"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if (fn(_unkey(mid)) < want) == rising:
            lo = mid
        else:
            hi = mid
    best = min((_unkey(k) for k in range(lo - 2, hi + 3)), key=lambda x: (abs(fn(x) - want), abs(x)))
    return best


def _arguments(case, g, state, ke2, nkbt, eta_mass, loops=1):
    """{label: fp64 argument} of the first `loops` loops."""
    eta, eta_dot, eta_dotdot = state
    res = R.chain_fp64(case.nc, loops, case.step_size / case.loops * loops, eta, eta_dot, eta_dotdot, eta_mass, ke2, nkbt, case.t_target(g))
    return dict(res["args"])


def start(case, g, ke2, nkbt, eta_mass):
    """(eta, eta_dot, eta_dotdot), lists of case.nc floats, for temperature group g of a system whose chain is handed ke2 and has the
    target nkbt = dof kT and the thermostat masses eta_mass."""
    nc, band = case.nc, case.band_of(g)
    dt2, dt4, dt8, _ = R.step_constants(case.step_size, case.loops, case.t_target(g))
    flip = -1.0 if g % 2 else 1.0
    # a lively, small background: arguments of 2^-9 ... 2^-8, accelerations that add a quarter to their link
    eta = [0.01 * (i + 1) * flip for i in range(nc)]
    eta_dot = [flip * (-1.0) ** i * 2.0 ** -9 * (1 + i / 8) / dt8 for i in range(nc)]
    eta_dot[0] = flip * 2.0 ** -10 / dt2
    eta_dotdot = [eta_dot[i] / (4 * dt4) for i in range(nc)]
    point = band in POINTS
    want = case.sign * BANDS[band][2]
    if case.target == "late" and band != "tiny":
        # the factor's argument x of the first loop is what is solved for: link 1 receives eta_dotdot[1] dt/4 = dof x^2 ... twice before the
        # second loop's -dt/8 eta_dot[1] is formed, which therefore is about -dof x^2 / 4
        def late(s):
            eta_dot[0] = s
            return abs(_arguments(case, g, (eta, eta_dot, eta_dotdot), ke2, nkbt, eta_mass, loops=2)[case.label()])
        x = math.sqrt(4 * BANDS["beyond"][2] / (nkbt / R.step_constants(case.step_size, case.loops, case.t_target(g))[3]))
        lo, hi = -case.sign * 0.5 * x / dt2, -case.sign * 2.0 * x / dt2
        assert late(lo) < BANDS["beyond"][2] < late(hi), "no bracket"
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if late(mid) < BANDS["beyond"][2] else (lo, mid)
        eta_dot[0] = lo
        return eta, eta_dot, eta_dotdot
    if case.target in ("factor", "late") or band == "tiny" and case.target != "prefix":
        if point and nc >= 2:
            eta_dot[1] = eta_dotdot[1] = 0.0    # link 1 at rest: link 0's expfac is exactly 1
        label, var = ("factor", 0), 0
    else:
        var = 2 if nc >= 3 else 1              # the link whose eta_dot the named argument multiplies
        label = case.label()
        if point:                              # nothing is added to the link, and the link above is at rest: the argument is -dt/8 times the start value
            eta_dotdot[var] = 0.0
            if var + 1 < nc:
                eta_dot[var + 1] = eta_dotdot[var + 1] = 0.0
        if want > P3:                          # the exp is e^|x| > 1 and multiplies every link below twice per sweep: start those small
            for i in range(var):
                eta_dot[i] *= math.exp(-2 * (var - i) * abs(want))
                eta_dotdot[i] *= math.exp(-2 * (var - i) * abs(want))

    def fn(s):
        eta_dot[var] = s
        return _arguments(case, g, (eta, eta_dot, eta_dotdot), ke2, nkbt, eta_mass)[label]

    eta_dot[var] = _solve(fn, want)
    return eta, eta_dot, eta_dotdot


def named_argument(case, g, args):
    """The argument the case names, from an argument list [(label, value)] of the whole application."""
    return dict(args)[case.label()]


def reaches_its_band(case, g, args, slack_ulps=0):
    """The case's claim about group g, from an argument list of the whole application: the named evaluation lies in the band, with the sign
    asked for.  A "tiny" group stays at or below 2^-6 in EVERY evaluation; a "late" group stays at or below 2^-3 through the first loop,
    with the factor's argument of the sign asked for, and the named evaluation of the second loop is beyond the fast exp's range."""
    band = case.band_of(g)
    a = {lab: float(v) for lab, v in args}
    if band == "tiny":
        named = a[case.label()] if case.target != "late" else a[("factor", 0)]
        return all(abs(v) <= BANDS["tiny"][1] for v in a.values()) and (named > 0) == (case.sign > 0)
    if case.target == "late":
        first = max(abs(v) for lab, v in a.items() if lab[1] == 0)
        x = a[case.label()]
        return high_word(first) <= SMALL_HI and in_band("beyond", x) and (a[("factor", 0)] > 0) == (case.sign > 0)
    x = a[case.label()]
    return in_band(band, x, slack_ulps) and (x > 0) == (case.sign > 0)


# ---- the table
def _table():
    out = []
    for nc in (1, 2, 3, 4, 5, 8):
        for loops in (1, 3):
            coupled = loops == 3 and nc >= 2
            for sign in (+1, -1):
                for band in IN_RANGE + OUT_OF_RANGE:
                    beyond = band in OUT_OF_RANGE
                    if coupled and band not in ("tiny", "mid", "below_2^-4", "above_2^-4"):
                        continue                                   # A = dof x^2 / 4 >= 1 / 4: the prefix and "late" targets reach these bands instead
                    if band == "4" and loops == 3:
                        continue                                   # (chain length 1: 2KE e^8 drives the next loop's argument past 8)
                    for hot in (("all", "g0", "g2") if beyond else ("all",)):
                        out.append(Case("il", nc, loops, "factor", band, sign, hot))
                if nc >= 2:
                    for band in IN_RANGE + OUT_OF_RANGE:
                        beyond = band in OUT_OF_RANGE
                        if beyond and loops == 3:
                            continue
                        for hot in (("all", "g0", "g2") if beyond else ("all",)):
                            out.append(Case("il", nc, loops, "prefix", band, sign, hot))
                if coupled:
                    for hot in ("all", "g0", "g2"):
                        out.append(Case("il", nc, 3, "late", "beyond", sign, hot))
    # an inactive group: the one-group water system with large finite chain velocities written into the groups it does not have
    for nc in (1, 2, 3, 4, 5, 8):
        for loops in (1, 3):
            for band in ("tiny", "upper", "2^-3", "0.3"):
                if loops == 3 and nc >= 2 and band in ("2^-3", "0.3"):
                    continue
                out.append(Case("water", nc, loops, "factor", band, -1 if band == "upper" else +1, "g0", inactive_eta_dot=3.0e7))
            if loops == 3 and nc >= 2:
                out.append(Case("water", nc, 3, "late", "beyond", +1, "g0", inactive_eta_dot=-3.0e7))
    # several blocks, each running its own chain: the 2 590-particle box, chain lengths of kernel B's compiled default and the stand-alone launch
    for nc in (3, 5):
        for band in ("upper", "2^-3", "first_hi", "0.3"):
            out.append(Case("il_large", nc, 1, "factor", band, +1, "g2" if band == "first_hi" else "all"))
        out.append(Case("il_large", nc, 3, "late", "beyond", +1, "g0"))
    return out


CASES = _table()
assert len({c.name for c in CASES}) == len(CASES)


def spec_of(system):
    import importlib
    systems = importlib.import_module("openmm-velocityverlet_amd").systems
    if system == "water":
        return systems.spce_water(30, seed=8)
    return systems.drude_il(cells=(1, 1, 1), pairs_per_cell=12, seed=21) if system == "il" else systems.drude_il(cells=(1, 1, 1), pairs_per_cell=70, seed=7)


def integrator_of(case_or_system, nc, loops=1, middle=True, cos=0.0):
    import importlib
    I = importlib.import_module("openmm-velocityverlet_amd").integrator
    s = SYSTEMS[case_or_system]
    it = I.VVIntegrator(s["temperature"], s["frequency"], s["drude_temperature"], s["drude_frequency"], STEP[loops], nc, loops)
    it.setMaxDrudeDistance(0.02 if case_or_system != "water" else 0.0)
    it.setCosAcceleration(cos)
    it.setUseMiddleScheme(middle)
    return it


_PLAN_INPUTS = {}


def plan_inputs(system, nc):
    """(nkbt[3], eta_mass[3][nc], groups) as the host plan computes them (no GPU needed)."""
    if (system, nc) not in _PLAN_INPUTS:
        import importlib
        pkg = importlib.import_module("openmm-velocityverlet_amd")
        plan, info, _ = pkg.integrator.create_plan(spec_of(system), integrator_of(system, nc))
        pkg.vvhip.lib.vvhip_plan_destroy(plan)
        assert info.num_temp_groups == SYSTEMS[system]["groups"]
        _PLAN_INPUTS[(system, nc)] = ([float(x) for x in info.nkbt], [[float(x) for x in row][:nc] for row in info.eta_mass])
    return _PLAN_INPUTS[(system, nc)]


def ke_scale(case):
    """What the GPU tests multiply the start's kinetic energy by: eta_dotdot[0] dt/4 then has the sign of the eta_dot[0] that a "factor"
    target asks for, the start value is the smaller of the two terms of their sum, and the sum can be every double next to the band's
    (otherwise the start value may lie in the binade above, where the sums skip every other one)."""
    return 1.0 - 0.15 * case.sign


def nominal_ke2(case, nkbt, g):
    """A kinetic energy for the CPU tests, which have no device to report one: ke_scale times a start 2 % ... 6 % off the target."""
    return nkbt * (1.0 + 0.02 * (g + 1) * (-1.0) ** g) * ke_scale(case)


def family(system, nc):
    """The cases of one (system, chain length): what one device context runs."""
    return [c for c in CASES if c.system == system and c.nc == nc]
