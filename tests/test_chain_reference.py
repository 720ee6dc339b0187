"""The exact Nose-Hoover chain reference (tests/chain_reference.py) and its case table (tests/chain_cases.py), on the CPU: the reference's
bound holds what an honest fp64 evaluation does (the oracle's C restatement, which tests/test_ref_api.py pins bit for bit to the reference
project's VVIntegrator.cpp, and the oracle's Python statement), every case of the table reaches the band it names at the evaluation it
names with every argument at or below 8, and the bound is tight enough to convict an exp with a wrong x^8 term -- in the cases above 2^-4,
not in the easy ones.  tests/test_gpu_chain.py then holds the device's chain against the same bound.

Inputs: the thermostat masses and targets of the systems the GPU tests run (the host plan computes them without a GPU) and a nominal
kinetic energy (chain_cases.nominal_ke2) in place of the one the device will report."""
import math
from decimal import Decimal

import numpy as np
import pytest

import chain_cases as K
import chain_reference as R
from oracle import oracle as O

FAMILIES = sorted({(c.system, c.nc) for c in K.CASES})
_RESOLVED = {}


def resolved(case):
    """Per temperature group of the case: (inputs, exact reference, plain fp64 chain with math.exp), computed once."""
    if case not in _RESOLVED:
        nkbt, mass = K.plan_inputs(case.system, case.nc)
        out = []
        for g in range(case.groups):
            ke2 = K.nominal_ke2(case, nkbt[g], g)
            eta, eta_dot, eta_dotdot = K.start(case, g, ke2, nkbt[g], mass[g])
            inp = (case.nc, case.loops, case.step_size, eta, eta_dot, eta_dotdot, mass[g], ke2, nkbt[g], case.t_target(g))
            out.append((inp, R.reference(*inp), R.chain_fp64(*inp)))
        _RESOLVED[case] = out
    return _RESOLVED[case]


def _oracle(fn, inp):
    nc, loops, step, eta, eta_dot, eta_dotdot, mass, ke2, nkbt, t = inp
    a = [np.array(eta, np.float64), np.array(list(eta_dot) + [0.0], np.float64), np.array(eta_dotdot, np.float64)]
    f = fn(a[0], a[1], a[2], np.array(mass, np.float64), ke2, nkbt, t, step, loops)
    assert a[1][nc] == 0.0
    return dict(factor=f, eta=list(a[0]), eta_dot=list(a[1][:nc]), eta_dotdot=list(a[2]))


def test_the_table_covers_what_it_claims():
    """Every band at every target, both signs, chain lengths 1-4 (kernel B) and 5, 8 (stand-alone), loops 1 and 3, out of range in group 0
    only, in group 2 only and in all groups, an inactive group -- and nothing is filtered: the families partition the table."""
    have = {(c.target, c.band) for c in K.CASES}
    for band in K.IN_RANGE + K.OUT_OF_RANGE:
        assert ("factor", band) in have and ("prefix", band) in have, band
    assert ("late", "beyond") in have
    il = [c for c in K.CASES if c.system == "il"]
    for nc in (1, 2, 3, 4, 5, 8):
        for loops in (1, 3):
            for sign in (1, -1):
                assert any(c.nc == nc and c.loops == loops and c.sign == sign and c.band in K.SENSITIVE for c in il), (nc, loops, sign)
        for hot in ("all", "g0", "g2"):
            assert any(c.nc == nc and c.hot == hot and (c.band in K.OUT_OF_RANGE or c.target == "late") for c in il), (nc, hot)
        assert any(c.nc == nc and c.system == "water" and c.inactive_eta_dot != 0 and c.band == "0.3" for c in K.CASES)
    assert any(c.system == "il_large" for c in K.CASES)
    assert sum(len(K.family(s, nc)) for s, nc in FAMILIES) == len(K.CASES) > 600
    assert K.high_word(K.BANDS["2^-3"][0]) == K.SMALL_HI == K.high_word(K.BANDS["next_2^-3"][0])
    assert K.high_word(K.BANDS["first_hi"][0]) == K.SMALL_HI + 1 and K.high_word(math.nextafter(K.FIRST_HI, 0)) == K.SMALL_HI
    assert K.BANDS["below_2^-4"][0] < K.P4 < K.BANDS["above_2^-4"][0] and math.nextafter(K.BANDS["below_2^-4"][0], 1) == K.P4


@pytest.mark.parametrize("system,nc", FAMILIES)
def test_every_case_reaches_its_band(system, nc):
    """(b) From the reference's argument list: the named evaluation lies in the named band (a point band: the fp64 sequence gives that very
    double, and the exact argument lies within its own bound of it), every argument is at most 8 and every quantity finite."""
    n = 0
    for case in K.family(system, nc):
        for g, (inp, ref, plain) in enumerate(resolved(case)):
            assert [lab for lab, _ in ref["args"]] == [lab for lab, _ in plain["args"]]
            assert K.reaches_its_band(case, g, plain["args"]), (case.name, g, dict(plain["args"])[case.label()])
            for (lab, a), (_, b) in zip(ref["args"], plain["args"]):
                assert abs(a.v) <= K.MAX_ARGUMENT, (case.name, g, lab, float(a))
                assert abs(a.v - Decimal(b)) <= a.e, (case.name, g, lab, float(a), b)
            slack = 0 if case.band_of(g) not in K.POINTS else 4
            assert K.reaches_its_band(case, g, [(lab, float(a)) for lab, a in ref["args"]], slack_ulps=slack), (case.name, g)
            assert all(math.isfinite(float(v.v)) and math.isfinite(float(v.e)) for _, v in R.quantities(ref)), (case.name, g)
            n += 1
    assert n == sum(c.groups for c in K.family(system, nc))


@pytest.mark.parametrize("system,nc", FAMILIES)
def test_fp64_evaluations_lie_inside_the_bound(system, nc):
    """(a) The oracle's C restatement (bit for bit the reference's own VVIntegrator.cpp, tests/test_ref_api.py), its Python statement and
    this module's plain fp64 chain: every quantity of every case within the bound."""
    worst = 0.0
    for case in K.family(system, nc):
        for g, (inp, ref, plain) in enumerate(resolved(case)):
            for what, got in (("C", _oracle(O.propagate_nh_chain, inp)), ("py", _oracle(O.propagate_nh_chain_py, inp)), ("plain", plain)):
                r, name = R.worst_ratio(got, ref)
                assert r <= 1.0, (case.name, g, what, name, r)
                worst = max(worst, r)
    print(f"{system} nc={nc}: worst |fp64 - exact| / bound {worst:.3f}")


@pytest.mark.parametrize("system,nc", FAMILIES)
def test_the_bound_convicts_a_degree_7_exp(system, nc):
    """(c) The plain fp64 chain with the degree-7 Taylor polynomial for exp (the x^8 term and everything above missing): outside the bound of
    at least one quantity in every group whose named argument lies in (2^-4, 2^-3], inside every bound in the cases at or below 2^-6."""
    sensitive = easy = 0
    for case in K.family(system, nc):
        for g, (inp, ref, _) in enumerate(resolved(case)):
            band = case.band_of(g)
            if band not in K.SENSITIVE and band != "tiny":
                continue
            r, name = R.worst_ratio(R.chain_fp64(*inp, exp=R.exp_degree7), ref)
            if band == "tiny":
                assert r <= 1.0, (case.name, g, name, r)
                easy += 1
            else:
                assert r > 1.0, (case.name, g, name, r)
                sensitive += 1
    assert easy > 0 and (sensitive > 0 or system != "il")


def test_decimal_agrees_with_mpmath():
    """(d) The same sequence on mpmath at 80 digits: values equal to 40 digits."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 80
    M = mp.mpf
    for case in K.CASES[::5]:
        for g, (inp, ref, _) in enumerate(resolved(case)):
            nc, loops, step, eta, eta_dot, eta_dotdot, mass, ke2, nkbt, t = inp
            dt2, dt4, dt8, kT = R.step_constants(step, loops, t)
            got = R._sequence(nc, loops, [M(x) for x in eta], [M(x) for x in eta_dot] + [M(0)], [M(x) for x in eta_dotdot], [M(x) for x in mass],
                              M(ke2), M(nkbt), M(dt2), M(dt4), M(dt8), M(kT), M(1), lambda a, b: a + b, lambda a, b: a - b, lambda a, b: a * b,
                              lambda a, m: a / m, mp.exp, lambda a: -a)
            for (name, a), (_, b) in zip(R.quantities(got), R.quantities(ref)):
                b = M(str(b.v))
                assert abs(a - b) <= M(10) ** -40 * max(abs(b), M(10) ** -300), (case.name, g, name)
