"""An exact reference for the Nose-Hoover chain, with a running bound on what an fp64 evaluation may differ from it.  Test code only;
standard library only.

`reference()` restates VVIntegrator::propagateNHChain (openmmapi/src/VVIntegrator.cpp:340-376, the stale expfac of lines 364-366 -- quirk
Q10 -- included) on decimal.Decimal at 80 digits.  Its inputs are the exact binary values of the fp64 inputs (Decimal(float) is exact);
dt2, dt4, dt8 and kT are formed in fp64 first, as the host forms them, and converted exactly.  Every variable carries, next to its value, a
first-order bound on the error that an fp64 evaluation of the same operation sequence may have (u = 2^-53):

    add, sub, mul                      u |result| + the propagated input bounds (mul: the product of the two input bounds as well)
    division by a thermostat mass     2u |result|   (covers the device's multiplication by the rounded reciprocal)
    exp(a)                             value (e^bound(a) - 1) + 2u value   (polynomial < 1 ulp for |x| <= 2^-3, library exp 1 ulp; one to spare)

Correlations are ignored (every term enters with its absolute value), so the bound is an upper one to first order; the GPU tests allow twice
the bound for what a first-order analysis leaves out.  `chain_fp64()` is the same operation sequence in plain Python floats with a
pluggable exp: the stand-in for "some fp64 implementation" that tests/test_chain_reference.py holds against the bound, and what
tests/chain_cases.py solves its start values with."""
import decimal
import math
from decimal import Decimal

CTX = decimal.Context(prec=80, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
U = Decimal(2) ** -53
BOLTZ = (1.380649e-23 * 6.02214076e23) / 1000.0        # the reference's BOLTZ (kJ/mol/K), formed in fp64


class V:
    """A value and the bound on an fp64 evaluation's error in it.  (Values go through CTX and the sign-only operations copy_negate /
    copy_abs: Decimal's operators, unary minus and abs() included, round to the thread's context of 28 digits.  The bounds may.)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=Decimal(0)):
        self.v, self.e = (v if isinstance(v, Decimal) else Decimal(v)), e

    def __float__(self):
        return float(self.v)


def _add(a, b):
    v = CTX.add(a.v, b.v)
    return V(v, CTX.add(CTX.multiply(U, v.copy_abs()), CTX.add(a.e, b.e)))


def _sub(a, b):
    return _add(a, V(b.v.copy_negate(), b.e))


def _mul(a, b):
    v = CTX.multiply(a.v, b.v)
    e = CTX.multiply(U, v.copy_abs()) + CTX.multiply(a.v.copy_abs(), b.e) + CTX.multiply(b.v.copy_abs(), a.e) + CTX.multiply(a.e, b.e)
    return V(v, CTX.plus(e))


def _div_mass(a, m):
    """a / m, m an exact input: 2u for the quotient (or the product with the rounded reciprocal)."""
    v = CTX.divide(a.v, m.v)
    return V(v, CTX.add(CTX.multiply(2 * U, v.copy_abs()), CTX.divide(a.e, m.v.copy_abs())))


def _exp(a):
    v = CTX.exp(a.v)
    grow = CTX.subtract(CTX.exp(a.e), Decimal(1))
    return V(v, CTX.add(CTX.multiply(v, grow), CTX.multiply(2 * U, v)))


def step_constants(step_size, loops_per_step, t_target):
    """dt2, dt4, dt8 and kT as the host forms them, in fp64."""
    dt2 = step_size / loops_per_step / 2
    dt4 = dt2 / 2
    dt8 = dt4 / 2
    return dt2, dt4, dt8, BOLTZ * t_target


def _sequence(nc, loops, eta, eta_dot, eta_dotdot, mass, ke2, ke2_target, dt2, dt4, dt8, kT, one, add, sub, mul, div_mass, exp, neg):
    """API:340-376, operation for operation, on whatever number type the callbacks work with.  Returns factor, the advanced arrays and the exp
    arguments in evaluation order as (label, argument): ("down", loop, link) for the sweep API:352-357, ("factor", loop) for API:358,
    ("up", loop, link) for API:367-374."""
    args = []
    eta, eta_dot, eta_dotdot = list(eta), list(eta_dot), list(eta_dotdot)
    factor = one
    expfac = one
    eta_dotdot[0] = div_mass(sub(ke2, ke2_target), mass[0])
    for iloop in range(loops):
        for ich in range(nc - 1, -1, -1):
            a = mul(neg(dt8), eta_dot[ich + 1])
            args.append((("down", iloop, ich), a))
            expfac = exp(a)
            eta_dot[ich] = mul(eta_dot[ich], expfac)
            eta_dot[ich] = add(eta_dot[ich], mul(eta_dotdot[ich], dt4))
            eta_dot[ich] = mul(eta_dot[ich], expfac)
        a = mul(neg(dt2), eta_dot[0])
        args.append((("factor", iloop), a))
        factor = mul(factor, exp(a))
        for ich in range(nc):
            eta[ich] = add(eta[ich], mul(dt2, eta_dot[ich]))
        eta_dotdot[0] = div_mass(sub(mul(mul(ke2, factor), factor), ke2_target), mass[0])
        eta_dot[0] = mul(eta_dot[0], expfac)                      # stale expfac (quirk Q10)
        eta_dot[0] = add(eta_dot[0], mul(eta_dotdot[0], dt4))
        eta_dot[0] = mul(eta_dot[0], expfac)
        for ich in range(1, nc):
            a = mul(neg(dt8), eta_dot[ich + 1])
            args.append((("up", iloop, ich), a))
            expfac = exp(a)
            eta_dot[ich] = mul(eta_dot[ich], expfac)
            eta_dotdot[ich] = div_mass(sub(mul(mul(mass[ich - 1], eta_dot[ich - 1]), eta_dot[ich - 1]), kT), mass[ich])
            eta_dot[ich] = add(eta_dot[ich], mul(eta_dotdot[ich], dt4))
            eta_dot[ich] = mul(eta_dot[ich], expfac)
    return dict(factor=factor, eta=eta[:nc], eta_dot=eta_dot[:nc], eta_dotdot=eta_dotdot[:nc], args=args)


def _check_inputs(nc, eta, eta_dot, eta_dotdot, eta_mass):
    assert len(eta) >= nc and len(eta_dot) >= nc and len(eta_dotdot) >= nc and len(eta_mass) >= nc
    xs = list(eta[:nc]) + list(eta_dot[:nc]) + list(eta_dotdot[:nc]) + list(eta_mass[:nc])
    assert all(math.isfinite(float(x)) for x in xs), "the reference is for finite inputs"


def reference(nc, loops_per_step, step_size, eta, eta_dot, eta_dotdot, eta_mass, ke2, ke2_target, t_target):
    """The exact chain.  All arguments are Python floats (lists of at least nc); eta_dot[nc], the element behind the last link, is 0 as in
    the reference, which never writes it.  Returns {"factor": V, "eta" / "eta_dot" / "eta_dotdot": [V] * nc, "args": [(label, V)]}."""
    _check_inputs(nc, eta, eta_dot, eta_dotdot, eta_mass)
    D = lambda x: V(Decimal(float(x)))
    dt2, dt4, dt8, kT = step_constants(float(step_size), int(loops_per_step), float(t_target))
    return _sequence(nc, int(loops_per_step), [D(x) for x in eta[:nc]], [D(x) for x in eta_dot[:nc]] + [D(0.0)], [D(x) for x in eta_dotdot[:nc]],
                     [D(x) for x in eta_mass[:nc]], D(ke2), D(ke2_target), D(dt2), D(dt4), D(dt8), D(kT), V(Decimal(1)),
                     _add, _sub, _mul, _div_mass, _exp, lambda a: V(a.v.copy_negate(), a.e))


def chain_fp64(nc, loops_per_step, step_size, eta, eta_dot, eta_dotdot, eta_mass, ke2, ke2_target, t_target, exp=math.exp):
    """The same sequence in Python floats (round to nearest, no contraction), `exp` for the exponential.  Same result layout, floats."""
    _check_inputs(nc, eta, eta_dot, eta_dotdot, eta_mass)
    F = float
    dt2, dt4, dt8, kT = step_constants(F(step_size), int(loops_per_step), F(t_target))
    return _sequence(nc, int(loops_per_step), [F(x) for x in eta[:nc]], [F(x) for x in eta_dot[:nc]] + [0.0], [F(x) for x in eta_dotdot[:nc]],
                     [F(x) for x in eta_mass[:nc]], F(ke2), F(ke2_target), dt2, dt4, dt8, kT, 1.0,
                     lambda a, b: a + b, lambda a, b: a - b, lambda a, b: a * b, lambda a, m: a / m, exp, lambda a: -a)


def exp_degree7(x):
    """The degree-7 Taylor polynomial (Horner): exact to < 1 ulp only up to |x| = 2^-6 -- the sensitivity check's wrong exp."""
    p = 1.0 / 5040.0
    for c in (1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0):
        p = p * x + c
    return p


def quantities(res):
    """[(name, value)] of a result: the factor, then eta, eta_dot, eta_dotdot link by link."""
    out = [("factor", res["factor"])]
    for name in ("eta", "eta_dot", "eta_dotdot"):
        out += [(f"{name}[{i}]", x) for i, x in enumerate(res[name])]
    return out


def ratio(got, ref):
    """|got - exact| / bound of one quantity (0 where both vanish)."""
    d = CTX.subtract(Decimal(float(got)), ref.v).copy_abs()
    if d == 0:
        return 0.0
    return float(CTX.divide(d, ref.e)) if ref.e != 0 else math.inf


def worst_ratio(got, ref):
    """(largest |got - exact| / bound over the quantities of a result, its name); `got` in the layout of chain_fp64."""
    worst = (0.0, "")
    for (name, g), (_, r) in zip(quantities(got), quantities(ref)):
        worst = max(worst, (ratio(g, r), name))
    return worst
