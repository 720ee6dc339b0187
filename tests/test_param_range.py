"""CPU: the cases of tests/param_range_cases.py reach the regimes they claim, and the oracle -- the reference side of
tests/test_gpu_param_range.py -- is finite there in every precision mode.  Also measures, per temperature case, the gap between the
oracle in single and in double precision: four times that gap is what the GPU test allows the product in single precision."""
import importlib

import numpy as np
import pytest

import param_range_cases as P
from oracle import oracle as O

pkg = importlib.import_module("openmm-velocityverlet_amd")
I = pkg.integrator

needs_probe = pytest.mark.skipif(not P.have_probe(), reason="needs g++ and an FMA-capable CPU (the host build of cos_short_range)")
SCHEMES = [True, False]


def _finite(osys, cos):
    m = osys.velm[:, 3] != 0
    ok = np.isfinite(osys.positions()).all() and np.isfinite(osys.velm[m]).all() and np.isfinite(osys.ke2()).all()
    ch = osys.chain_state()
    ok = ok and all(np.isfinite(ch[k]).all() for k in ch) and np.isfinite(osys.vscale()).all()
    if cos != 0:
        ok = ok and np.isfinite(osys.viscosity()).all()
    return bool(ok)


def _cases_without_probe():
    return [c for c in P.CASES if c != "node"]


@pytest.mark.parametrize("middle", SCHEMES)
@pytest.mark.parametrize("name", _cases_without_probe())
def test_oracle_stays_finite(name, middle):
    c = P.case(name)
    for cos in c.cos_values:
        for prec in ("mixed", "single", "double"):
            osys = P.oracle_run(name, middle, cos, prec)
            assert _finite(osys, cos), (name, middle, cos, prec)
            ke = osys.ke2()[: osys.s.num_tg]
            assert (ke > 0).all() and ke.sum() < 200 * osys.t["nkbt"].sum(), (name, prec, ke)       # sane: nothing blew up


@needs_probe
@pytest.mark.parametrize("middle", SCHEMES)
def test_oracle_stays_finite_at_the_node(middle):
    for prec in ("mixed", "single", "double"):
        assert _finite(P.oracle_run("node", middle, 0.02, prec), 0.02), (middle, prec)


@pytest.mark.parametrize("name", P.TEMPERATURE_CASES[:2])
def test_cold_cases_clamp_the_scale_exponent(name):
    """pick_scale(total, 1024) wants 2^49 (1 K) / 2^41 (30 K) and is held at 2^40; at 333 K and above it is not clamped."""
    c = P.case(name)
    info, _ = I.plan_layout(c.spec, c.integrator(), "mixed")
    nkbt = np.array(list(info.nkbt))
    assert np.allclose(nkbt, P.oracle_run(name, True, 0.02, "mixed").t["nkbt"], rtol=1e-14)
    wanted, used = P.scale_exponent(nkbt)
    assert wanted > 40 and used == 40, (wanted, used)
    for other in P.TEMPERATURE_CASES[2:]:
        o = P.case(other)
        w, u = P.scale_exponent(list(I.plan_layout(o.spec, o.integrator(), "mixed")[0].nkbt))
        assert w == u < 40, (other, w, u)


@pytest.mark.parametrize("name", P.TEMPERATURE_CASES[:2])
def test_fixed_point_resolution_where_the_exponent_is_clamped(name):
    """Every block rounds its partial sums to multiples of 2^-k (csrc/vv_dev_wave.inc: block_fixed_point_sum), so a group's 2KE is off by at
    most blocks x 0.5 x 2^-k.  With k held at 40 that must still be below the 1e-10 the GPU tests ask of the sums, for the smallest group
    (the centre-of-mass group at 1 K: 0.5 kJ/mol) -- otherwise the clamp in pick_scale is too low."""
    c = P.case(name)
    info, _ = I.plan_layout(c.spec, c.integrator(), "mixed")
    shape = I.plan_launch_shape(c.spec, c.integrator(), "mixed")
    blocks = min(max(shape[1], shape[2]), info.num_waves)              # no more blocks with particles than tile waves
    k = P.scale_exponent(list(info.nkbt))[1]
    for middle in SCHEMES:
        smallest = P.oracle_run(name, middle, 0.02, "mixed").ke2().min()
        derived = blocks * 0.5 * 2.0 ** -k / smallest
        print(f"{name} middle={middle}: {blocks} blocks, k = {k}, smallest 2KE {smallest:.3g}: resolution {derived:.2e}")
        assert 0 < derived < 1e-10, (blocks, k, smallest, derived)


def test_cases_start_near_their_targets():
    """Temperatures of the three groups after one step within a factor 3 of the targets (the hot starts: of ke_factor times them)."""
    for name in P.CASES:
        if name == "node" and not P.have_probe():
            continue
        c = P.case(name)
        osys = P.oracle_run(name, True, c.cos_values[-1], "double", steps=1)
        ratio = osys.ke2().sum() / osys.t["nkbt"].sum()
        assert c.ke_factor / 3 < ratio < c.ke_factor * 3, (name, ratio)
    for name in ("hot30", "hot100"):                  # ... and the hot starts stay below the 1024 x headroom of the sums all the way
        worst = []
        P.oracle_run(name, True, 0.02, "double", watch=lambda o: worst.append(o.ke2().sum() / o.t["nkbt"].sum()))
        assert 20 < max(worst) < 200, (name, worst)


@pytest.mark.parametrize("middle", SCHEMES)
def test_hard_wall_fires_at_5000_K(middle):
    """Without the wall (max_drude_distance 0) some Drude pair is beyond the case's wall (0.002 nm) after one of the ten steps.  Up to the first such step
    the walled run is the same run, so there its wall stage meets that pair beyond the wall and takes the sqrt(kB T_D) branch."""
    c = P.case(P.HOT_THERMOSTAT)
    p = c.params(middle, 0.02)
    p.max_drude_distance = 0.0
    free = O.OracleSystem(c.spec, p, "mixed", force_mode=1)
    d, par = c.spec.drude_pairs[:, 0], c.spec.drude_pairs[:, 1]
    beyond = 0
    for _ in range(P.NSTEPS):
        free.step(1)
        x = free.positions()
        beyond = int((np.linalg.norm(x[d] - x[par], axis=1) > c.max_drude_distance).sum())
        if beyond:
            break
    assert beyond > 0
    walled = P.oracle_run(P.HOT_THERMOSTAT, middle, 0.02, "mixed").positions()
    assert np.linalg.norm(walled[d] - walled[par], axis=1).max() < 1.5 * c.max_drude_distance


@needs_probe
@pytest.mark.parametrize("prec", ["mixed", "double"])
@pytest.mark.parametrize("name", ["up400", "down400", "mixed_wave"])
def test_unwrapped_cases_leave_the_short_range_of_the_cosine(name, prec):
    c = P.case(name)
    z, inv = P.real_z(c.spec, prec)
    x = 2 * 3.1415926 * z * inv
    assert (np.abs(x[c.shifted]) > 1024).all() and (np.abs(x[~c.shifted]) <= 1024).all()
    ok = P.cos_ok(z, inv)
    assert np.array_equal(ok, ~c.shifted)                 # the library cosine for exactly the shifted particles
    assert c.shifted.sum() == c.spec.num_atoms - (P.MIXED_WAVE_UNSHIFTED if name == "mixed_wave" else 0)
    # the wave layout: all lanes of all waves take the fallback, or -- the mixed wave -- lanes of both kinds share the first wave
    _, slots = I.plan_layout(c.spec, c.integrator(True, 0.02), prec)
    waves = slots[:, 0].reshape(-1, 64)
    used = waves >= 0
    kinds = [set(ok[w[u]].tolist()) for w, u in zip(waves, used) if u.any()]
    if name == "mixed_wave":
        assert kinds[0] == {True, False} and all(k == {False} for k in kinds[1:]), kinds
        assert 0 < int(ok[waves[0][used[0]]].sum()) < int(used[0].sum())
    else:
        assert all(k == {False} for k in kinds)


@needs_probe
def test_node_case_sits_next_to_pi_over_two():
    c = P.case("node")
    z, inv = P.real_z(c.spec, "double")
    i = c.node_particle
    x = 2 * 3.1415926 * z * inv
    assert abs(x[i]) <= 1024 and abs(x[i] - np.pi / 2) < 2.0 ** -36 and c.spec.masses[i] > 0
    ok = P.cos_ok(z, inv)
    assert not ok[i] and ok.sum() == c.spec.num_atoms - 1
    base_z = P.base("small").positions[:, 2]
    assert abs(z[i] - float(c.spec.box[2]) / 4) < 1e-7 * float(c.spec.box[2])
    assert np.array_equal(np.delete(z, i), np.delete(base_z, i))


@pytest.mark.parametrize("middle", SCHEMES)
@pytest.mark.parametrize("name", P.TEMPERATURE_CASES)
def test_single_precision_gap(name, middle):
    """The oracle in single against the oracle in double over the case's ten steps.  Below 1e-3 relative the GPU test holds the product
    in single precision to four times this gap (tests/test_gpu_param_range.py); the figures are in TUNING_LOG.md."""
    gap = P.single_gap(name, middle)
    print(f"{name} middle={middle}: single-double gap pos {gap['x']:.2e} vel {gap['v']:.2e} 2KE {gap['ke2']:.2e}")
    assert all(np.isfinite(v) and 0 < v < 1e-3 for v in gap.values()), gap
