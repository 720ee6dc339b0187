"""-m gpu: the stage sets vvhip_debug_fused_flags reports are the stage sets a step launches.

The step entry points and the accessor read one composition of the thermostat application (csrc/vv_steps.cpp: compose_application), in
each of its modes: plain, the cos perturbation in moment form, and the cos perturbation as the bias -> sums -> scale sequence.  With
run-time compilation off and the one-launch step off, a launch whose stage set has no compiled kernel runs the generic one and
vvhip_generic_launches reports that set; it must be the accessor's, up to the bits that are named here:
  * what run_a / run_b add on their own (mass tables, arithmetic layout, Gauss-Seidel sweeps): removed from the launched set;
  * what the accessor leaves out on purpose (the load of a stale forceExtra; without NH particles the cos(kz) store): removed from
    the launched set as well -- none of the plans below launches either, so the comparison stays exact;
  * the hand-over pair A_NOSTORE / B_KICK: both sides carry it in a two-launch step, so it is compared like every other bit, and
    the accessor's two words must agree on it."""
import ctypes as C
import importlib
import os
import re

import pytest

import constraint_cases as cc

pkg = importlib.import_module("openmm-velocityverlet_amd")
H, I, S = pkg.vvhip, pkg.integrator, pkg.systems
pytestmark = pytest.mark.gpu

_HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "openmm-velocityverlet_amd", "csrc", "vv_args.hpp")).read()


def _bit(name):
    return 1 << int(re.search(rf"\b{name}\s*=\s*1u\s*<<\s*(\d+)", _HEADER).group(1))


OWN = (_bit("A_MTAB") | _bit("A_PERIODIC") | _bit("A_SHAKE_GS"), _bit("B_MTAB") | _bit("B_PERIODIC") | _bit("B_SHAKE_GS"))
LEFT_OUT = (_bit("A_FE_LOAD"), 0)      # (+ A_CZ_STORE without NH particles: every plan here has them)
A_NOSTORE, B_KICK, A_GCONS, B_CHAIN = _bit("A_NOSTORE"), _bit("B_KICK"), _bit("A_GCONS"), _bit("B_CHAIN")


def _accessor(ctx, kernel):
    f = C.c_uint32()
    H.check(H.lib.vvhip_debug_fused_flags(ctx.plan, kernel, C.byref(f)), ctx.plan)
    return f.value


def _launched_and_reported(spec, it, tune, steps=3):
    """(counts, stage sets) of the generic launches of `steps` two-launch steps, the accessor's two words, the step's phase count."""
    old = I.Context.rtc_mode(0)
    try:
        ctx = I.Context(spec, it, precision="mixed", force_provider="tether", tune=dict(tune, fused=0))
        try:
            it.step(steps)
            ctx.synchronize()
            counts, sets = ctx.generic_launches()
            return counts, sets, (_accessor(ctx, 0), _accessor(ctx, 1)), H.lib.vvhip_step_middle_phases(ctx.plan)
        finally:
            ctx.close()
    finally:
        I.Context.rtc_mode(old)


def _same(kernel, launched, reported):
    return (launched & ~(OWN[kernel] | LEFT_OUT[kernel])) == reported


@pytest.mark.parametrize("cos,no_moments,phases", [(0.0, 0, 2), (0.02, 0, 2), (0.02, 1, 3)], ids=["plain", "cos_moments", "cos_three_launches"])
def test_kernel_b_runs_the_set_the_accessor_reports(cos, no_moments, phases):
    """Four chain links: kernel B's compiled specialisations carry the three-link chain only, so every step's kernel B is a generic launch."""
    spec = S.drude_il(cells=(1, 1, 1), pairs_per_cell=20, seed=2)
    it = I.VVIntegrator(333.0, 10.0, 1.0, 40.0, 0.001, numNHChains=4)
    it.setMaxDrudeDistance(0.02)
    if cos:
        it.setCosAcceleration(cos)
    counts, sets, acc, nph = _launched_and_reported(spec, it, {"no_moments": no_moments})
    assert nph == phases
    assert counts[1] == 3
    assert acc[1] & B_CHAIN
    assert _same(1, sets[1], acc[1]), f"kernel B launched 0x{sets[1]:x}, the accessor reports 0x{acc[1]:x}"
    assert bool(acc[0] & A_NOSTORE) == bool(acc[1] & B_KICK)


def test_kernel_a_runs_the_set_the_accessor_reports():
    """General constraint clusters: A_GCONS has no compiled kernel, so every step's kernel A is a generic launch."""
    spec, kind = cc.case("general")
    assert kind == "general"
    counts, sets, acc, nph = _launched_and_reported(spec, I.VVIntegrator(300.0, 10.0, 1.0, 40.0, 0.002), {})
    assert nph == 2
    assert counts[0] > 0
    assert acc[0] & A_GCONS
    assert _same(0, sets[0], acc[0]), f"kernel A launched 0x{sets[0]:x}, the accessor reports 0x{acc[0]:x}"
    assert bool(acc[0] & A_NOSTORE) == bool(acc[1] & B_KICK)
