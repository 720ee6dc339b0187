"""-m gpu: the fused step at the edges of its parameter range (tests/param_range_cases.py; tests/test_param_range.py shows on the CPU that
every case reaches its regime) against the oracle: temperatures 1 K ... 5000 K (the fixed-point scales of the thermostat sums, clamped in
the cold cases; the hard wall's sqrt(kB T_D)), dt 1e-5 / 4e-3 ps, thermostat frequencies 0.1 ... 800 per ps, masses x 0.01 / x 100 / a
0.05 u Drude particle on a 200 u parent, starts 30 and 100 times hotter than the target (no overflow report, still right), and positions
400 box lengths out (cos_kz's library-cosine branch: whole waves, a wave with lanes of both kinds, one lane next to pi / 2).

Bounds, none of them taken from the product's output: positions and velocities 1e-9 relative after 10 steps (test_gpu_edges._assert_close),
2KE 1e-10 (test_molecules_larger_than_a_wave_with_com_group) plus the resolution of the fixed-point sums, blocks x 0.5 x 2^-k per group
(negligible unless the exponent is clamped; test_param_range.py holds it below 1e-10 of the smallest group even then), the chain state as
test_chain_length_and_loops, the viscosity as test_gpu_steps.test_bulk_drude_il.  Single precision (temperature cases): four times the gap
between the oracle in single and in double precision, measured per case (param_range_cases.single_gap; TUNING_LOG.md has the figures)."""
import importlib

import numpy as np
import pytest

import param_range_cases as P
from oracle import oracle as O, cases

pkg = importlib.import_module("openmm-velocityverlet_amd")
I = pkg.integrator
pytestmark = pytest.mark.gpu

REPLAYED = [P.COLD, "hot30", "hot100", "mixed_wave"]      # also through run_graph, and one launch against two


def _trajectories():
    out = []
    for name in P.CASES:
        if name == "node":                      # needs the host build of cos_short_range to be made: see test_node_lane
            continue
        c = P.case(name)
        out += [pytest.param(name, middle, prec, cos, id=f"{name}-{'middle' if middle else 'classic'}-{prec}-cos{cos:g}")
                for middle in (True, False) for prec in c.precisions for cos in c.cos_values]
    return out


def _context(c, prec, middle, cos, tune=None):
    it = c.integrator(middle, cos)
    return it, I.Context(c.spec, it, precision=prec, force_provider="tether", k_tether=c.k_tether, k_drude=c.k_drude, tune=tune)


def _errors(osys, ctx):
    x_o, x_g = osys.positions(), ctx.getPositions()
    v_o, v_g = osys.velm[:, :3].astype(np.float64), ctx.getVelocities()
    m = osys.velm[:, 3] != 0
    assert np.isfinite(x_g).all() and np.isfinite(v_g[m]).all()
    return P.rel_gap(x_g, x_o), P.rel_gap(v_g, v_o, m)


def _sum_resolution(c, ctx, prec):
    """blocks x 0.5 x 2^-k: what rounding every block's partial 2KE sums to fixed point can cost (csrc/vv_dev_wave.inc: block_fixed_point_sum)."""
    shape = I.plan_launch_shape(c.spec, c.integrator(), prec)
    blocks = min(max(shape[1], shape[2]), ctx.info.num_waves)
    return blocks * 0.5 * 2.0 ** -P.scale_exponent(list(ctx.info.nkbt))[1]


def _check(name, middle, prec, cos):
    c = P.case(name)
    osys = P.oracle_run(name, middle, cos, prec)
    it, ctx = _context(c, prec, middle, cos)
    try:
        it.step(P.NSTEPS)
        ex, ev = _errors(osys, ctx)
        st, ntg = ctx.getNHState(), osys.s.num_tg
        ke_o, ke_g = osys.ke2()[:ntg], np.array(list(st.ke2))[:ntg]
        eke = float(np.abs(ke_g / ke_o - 1).max())
        print(f"{name} middle={middle} {prec} cos={cos}: rel err pos {ex:.2e} vel {ev:.2e} 2KE {eke:.2e}")
        if prec == "single":
            gap = P.single_gap(name, middle, cos)
            assert ex < 4 * gap["x"] and ev < 4 * gap["v"] and eke < 4 * gap["ke2"], (ex, ev, eke, gap)
        else:
            assert ex < 1e-9 and ev < 1e-9, (ex, ev)
            assert np.allclose(ke_g, ke_o, rtol=1e-10, atol=_sum_resolution(c, ctx, prec)), (ke_g, ke_o)
            ch = osys.chain_state()
            for g in range(ntg):
                assert np.allclose(list(st.eta[g])[:3], ch["eta"][g][:3], rtol=1e-8, atol=1e-14), (g, list(st.eta[g])[:3], ch["eta"][g])
                assert np.allclose(list(st.eta_dot[g])[:3], ch["eta_dot"][g][:3], rtol=1e-7, atol=1e-12), (g, list(st.eta_dot[g])[:3], ch["eta_dot"][g])
        if cos != 0:
            (v_g, inv_g), (v_o, inv_o) = it.getViscosity(), osys.viscosity()
            assert v_g == pytest.approx(v_o, rel=1e-4, abs=1e-9) and inv_g == pytest.approx(inv_o, rel=1e-4, abs=1e-9), (v_g, v_o, inv_g, inv_o)
        assert ctx.status() == (False, False)
    finally:
        ctx.close()


@pytest.mark.parametrize("name,middle,prec,cos", _trajectories())
def test_trajectory_against_the_oracle(name, middle, prec, cos):
    _check(name, middle, prec, cos)


@pytest.mark.skipif(not P.have_probe(), reason="needs g++ and an FMA-capable CPU (the host build of cos_short_range)")
@pytest.mark.parametrize("middle", [True, False])
def test_node_lane(middle):
    """Double precision, one hydrogen whose cos argument lies within 2^-36 of pi / 2 with |x| <= 1024: that lane alone takes the library
    cosine in its wave's first cos stages."""
    _check("node", middle, "double", 0.02)


def _state(c, prec, middle, cos, mode, tune=None):
    it, ctx = _context(c, prec, middle, cos, tune)
    try:
        if mode == "graph":
            ctx.run_graph(P.NSTEPS, steps_per_graph=5)
        else:
            it.step(P.NSTEPS)
        active, launches = ctx.fused_status()
        return dict(posq=ctx.getPosq(), velm=ctx.getVelm(), corr=ctx.getPosqCorrection() if prec == "mixed" else None, nh=bytes(ctx.getNHState()),
                    active=active, launches=launches, words=ctx.status_words())
    finally:
        ctx.close()


def _same(a, b, label):
    for k in ("posq", "velm", "corr"):
        if a[k] is not None:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{label}: {k} differs"
    assert a["nh"] == b["nh"], f"{label}: thermostat state differs"
    assert a["words"] == [0, 0, 0, 0] and b["words"] == [0, 0, 0, 0], (a["words"], b["words"])


@pytest.mark.parametrize("middle", [True, False])
@pytest.mark.parametrize("name", REPLAYED)
def test_graph_replay_equals_eager(name, middle):
    c = P.case(name)
    cos = c.cos_values[-1]
    _same(_state(c, "mixed", middle, cos, "eager"), _state(c, "mixed", middle, cos, "graph"), f"{name} middle={middle}")


@pytest.mark.parametrize("prec", ["mixed", "double"])
@pytest.mark.parametrize("name", REPLAYED)
def test_one_launch_step_equals_two_launch_step(name, prec):
    c = P.case(name)
    cos = c.cos_values[-1]
    one = _state(c, prec, True, cos, "eager", tune={"fused": 1})
    two = _state(c, prec, True, cos, "eager", tune={"fused": 0})
    assert one["active"] and one["launches"] == P.NSTEPS, (one["active"], one["launches"])
    assert not two["active"] and two["launches"] == 0
    _same(one, two, f"{name}/{prec}")


# ---- the cos stages one by one at unwrapped positions, all three precision modes
COS_STAGES = ("cosforce.", "bias.", "remove.", "restore.")
KEEP = 40       # particles of the "mixed" variant that stay in the box


def _shifted_inputs(prec, variant):
    inp = dict(cases.case_bulk(prec))
    n = inp["velm"].shape[0]
    mask = {"up": np.ones(n, bool), "down": np.ones(n, bool), "mixed": np.arange(n) >= KEEP, "none": np.zeros(n, bool)}[variant]
    R = O.REAL[prec]
    z = inp["posq"][:, 2].astype(np.float64) + (inp["posq_corr"][:, 2].astype(np.float64) if prec == "mixed" else 0.0)
    z = z + np.where(mask, (-1.0 if variant == "down" else 1.0) * P.SHIFT_BOXES * float(inp["box"][2]), 0.0)
    posq, corr = inp["posq"].copy(), inp["posq_corr"].copy()
    posq[:, 2] = z.astype(R)
    if prec == "mixed":
        corr[:, 2] = (z - posq[:, 2].astype(np.float64)).astype(R)
    inp["posq"], inp["posq_corr"] = posq, corr
    return inp, mask


def _cos_stages(K, inp):
    return {k: v for k, v in cases.run_sequence(K, inp).items() if k.startswith(COS_STAGES)}


def _hip_stages(prec, inp):
    from hipkernels import HipKernels
    K = HipKernels(prec, inp)
    try:
        return _cos_stages(K, inp)
    finally:
        K.close()


@pytest.mark.parametrize("prec", O.PRECISIONS)
@pytest.mark.parametrize("variant", ["up", "down", "mixed"])
def test_cos_stages_at_unwrapped_positions(variant, prec):
    """cosforce, bias, remove, restore of oracle/cases.run_sequence on case_bulk's inputs moved 400 box lengths along z (a copy: the golden
    files know nothing of it), kernels against oracle within test_gpu_kernels' element-wise bounds: the device library's cosine against
    glibc's, both within 1 ulp.  The lanes of the mixed wave that stay in the box must give the bits of a run with nothing shifted."""
    from hipkernels import spec_from_inputs, integrator_from_inputs
    from test_gpu_kernels import _compare
    inp, mask = _shifted_inputs(prec, variant)
    R = O.REAL[prec]
    x = 2 * 3.1415926 * inp["posq"][:, 2].astype(np.float64) * float(R(1.0 / float(inp["box"][2])))
    assert (np.abs(x[mask]) > 1024).all() and (np.abs(x[~mask]) <= 1024).all()
    want = _cos_stages(O.Kernels("oracle", prec), inp)
    got = _hip_stages(prec, inp)
    assert set(got) == set(want) and len(want) == 4, sorted(want)
    _compare(got, want, prec, f"bulk shifted {variant}/{prec}")
    if variant == "mixed":
        _, slots = I.plan_layout(spec_from_inputs(inp), integrator_from_inputs(inp), prec)
        first = slots[:64, 0]
        first = first[first >= 0]
        assert mask[first].any() and not mask[first].all()          # lanes of both kinds in the first wave
        plain = _hip_stages(prec, _shifted_inputs(prec, "none")[0])
        rows = ~mask[inp["masses"] != 0]                             # the snapshot holds the massive particles' rows
        assert rows.sum() > 10
        assert np.array_equal(got["cosforce.fe"][rows].view(np.uint8), plain["cosforce.fe"][rows].view(np.uint8))
        assert not np.array_equal(got["cosforce.fe"][~rows], plain["cosforce.fe"][~rows])
