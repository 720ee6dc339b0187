"""The Monte Carlo barostat on the CPU: properties of the reference arithmetic (tests/barostat_reference.py) and the host-side driver
(openmm-velocityverlet_amd/barostat.py) against the NumPy stand-in context.  The device half is tests/test_gpu_barostat.py."""
import copy
from fractions import Fraction
import importlib.util
import json
import os

import numpy as np
import pytest

import barostat_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the driver is plain numpy: loaded by path, so these tests need neither the built library nor a GPU)
_spec = importlib.util.spec_from_file_location("vv_barostat_driver", os.path.join(ROOT, "openmm-velocityverlet_amd", "barostat.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

PRECISIONS = ("single", "mixed", "double")


def _system(seed=3):
    """Molecules of 1, 2, 5 and 70 particles, interleaved ids, positions far outside a 3 nm box, negative ones included."""
    rng = np.random.default_rng(seed)
    mol = np.concatenate([np.arange(40), np.repeat(np.arange(40, 60), 2), np.repeat(np.arange(60, 70), 5), np.full(70, 70)])
    mol = mol[rng.permutation(mol.size)]
    centre = rng.uniform(-40.0, 40.0, (71, 3))
    pos = centre[mol] + rng.normal(0.0, 0.15, (mol.size, 3))
    return pos, mol


def _stored_ulp(x, precision):
    """One rounding of the stored type at |x|: float32 / the float32 pair (2^-47 |x|: half an ulp of the correction plus the float64 add) / float64."""
    x = np.abs(x)
    if precision == "single":
        return np.spacing(x.astype(np.float32)).astype(np.float64)
    if precision == "mixed":
        return np.maximum(x, 1e-30) * 2.0 ** -47
    return np.spacing(x)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_molecules_move_rigidly(precision):
    pos, mol = _system()
    ctx = R.StandInContext(pos, [3.0, 3.0, 3.0], mol, precision)
    x0 = ctx.getPositions()
    ctx.scale_box([1.01, 0.97, 1.2])
    x1 = ctx.getPositions()
    worst = 0.0
    exact = np.vectorize(Fraction, otypes=[object])          # (float64 differences would add roundings of their own)
    for m in np.unique(mol):
        idx = np.flatnonzero(mol == m)
        change = (exact(x1[idx]) - exact(x1[idx[0]])) - (exact(x0[idx]) - exact(x0[idx[0]]))
        bound = _stored_ulp(x1[idx], precision) + _stored_ulp(x1[idx[0]], precision)
        ratio = np.abs(change.astype(np.float64)) / bound
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0), (precision, m)
    print(f"{precision}: largest change of an intramolecular vector = {worst:.3f} of the bound")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_centres_scale_with_the_box(precision):
    pos, mol = _system()
    s = np.array([1.01, 0.97, 1.2])
    ctx = R.StandInContext(pos, [3.0, 3.0, 3.0], mol, precision)
    before = R.centres(ctx.getPositions(), mol, ctx.F)
    ctx.scale_box(s)
    x1 = ctx.getPositions()
    after = R.centres(x1, mol, ctx.F)
    assert ctx.F == 40 - 7                      # the largest molecule has 70 particles
    for m in before:
        ulp = _stored_ulp(x1[mol == m], precision).max(axis=0)
        assert np.all(np.abs(after[m][0] - s * before[m][0]) <= 2.0 ** -ctx.F + ulp), (precision, m)
    assert np.array_equal(ctx.box, np.array([3.0, 3.0, 3.0]) * s)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_axis_with_unit_scale_keeps_its_bits(precision):
    pos, mol = _system()
    ctx = R.StandInContext(pos, [3.0, 3.0, 3.0], mol, precision)
    if precision == "mixed":                    # a correction no split would produce: a re-split would change it
        ctx.corr[:, 1] = np.float32(0.25)
    ctx.posq[:, 3] = np.arange(mol.size)        # charges
    posq0, corr0 = ctx.posq.copy(), ctx.corr.copy()
    ctx.scale_box([0.97, 1.0, 1.2])
    assert ctx.posq[:, 1].tobytes() == posq0[:, 1].tobytes() and ctx.corr[:, 1].tobytes() == corr0[:, 1].tobytes()
    assert ctx.posq[:, 3].tobytes() == posq0[:, 3].tobytes() and ctx.corr[:, 3].tobytes() == corr0[:, 3].tobytes()
    assert not np.array_equal(ctx.posq[:, 0], posq0[:, 0]) and not np.array_equal(ctx.posq[:, 2], posq0[:, 2])


def test_reference_sums_do_not_depend_on_order_and_refuse_bad_positions():
    pos, mol = _system()
    perm = np.random.default_rng(5).permutation(mol.size)
    F = R.frac_bits(mol)
    a, b = R.centres(pos, mol, F), R.centres(pos[perm], mol[perm], F)
    assert all(np.array_equal(a[m][0], b[m][0]) for m in a)
    for bad in (2.0 ** 22, np.nan, -np.inf):
        p = pos.copy()
        p[7, 1] = bad
        with pytest.raises(R.Overflow):
            R.centres(p, mol, F)
    p = pos.copy()
    p[7, 1] = np.nextafter(2.0 ** 22, 0.0)      # the largest position taken
    R.centres(p, mol, F)


# ---------------------------------------------------------------------------------------------- the driver
def test_modes_are_the_five_of_the_reference_s_helper():
    assert B.MODES == {"iso": ((0, 1, 2),), "semi-iso": ((0, 1), (2,)), "xyz": ((0,), (1,), (2,)), "xy": ((0,), (1,)), "z": ((2,),)}
    with pytest.raises(ValueError):
        B.MonteCarloBarostat(1.0, 300.0, mode="triclinic")


@pytest.mark.parametrize("mode", sorted(B.MODES))
def test_scale_vector_is_the_root_of_the_volume_ratio_on_the_group_s_axes(mode):
    pos, mol = _system()
    ctx = R.StandInContext(pos, [3.0, 3.1, 3.2], mol, "mixed")
    baro = B.MonteCarloBarostat(1.0, 300.0, mode=mode, seed=11)
    seen_groups = set()
    for k in range(24):
        volume = float(np.prod(ctx.getPeriodicBoxSize()))
        baro.attempt(ctx, lambda: 0.0)
        g, d_volume, _, _ = baro.last
        seen_groups.add(g)
        f = ((volume + d_volume) / volume) ** (1.0 / len(B.MODES[mode][g]))
        expect = [f if a in B.MODES[mode][g] else 1.0 for a in range(3)]
        assert ctx.scales_seen[k].tolist() == expect
    assert seen_groups == set(range(len(B.MODES[mode])))


# p(V) ~ V^N exp(-P V / kT) for N ideal molecules: mean (N + 1) kT / P, variance (N + 1) (kT / P)^2.  N = 16 one-particle molecules, T = 300 K,
# P = 1000 bar, a FIXED step 2 sqrt(N + 1) kT / P (an adaptive step breaks detailed balance: 1-3 % of bias at this N), 40 000 attempts, the
# first tenth discarded.  The same law in plain NumPy, 8 seeds per mode, gave the mean at 0.981-1.011 and the variance at 0.953-1.036 of
# the analytic values: hence 3 % and 8 %.  A missing N ln(V'/V) puts the mean off by a factor of about 17, a missing + 1 by about 6 %.
# The particles sit at the origin: with the anisotropic modes the box's aspect ratio is a free random walk over tens of thousands of
# attempts (only the volume is bound), and positions that follow an edge would leave the 2^22 nm the fixed point takes.
@pytest.mark.parametrize("mode", ["iso", "semi-iso", "xyz"])
def test_ideal_gas_volume_law(mode):
    N, T, P_bar, attempts = 16, 300.0, 1000.0, 40000
    baro = B.MonteCarloBarostat(P_bar, T, mode=mode, seed=2024, adapt=False)
    v_unit = baro.kT / baro.pressure
    baro.setVolumeScale(2.0 * np.sqrt(N + 1) * v_unit)
    edge = ((N + 1) * v_unit) ** (1.0 / 3.0)
    ctx = R.StandInContext(np.zeros((N, 3)), [edge] * 3, np.arange(N), "double")
    volumes = np.empty(attempts)
    for k in range(attempts):
        baro.attempt(ctx, lambda: 0.0)
        volumes[k] = np.prod(ctx.box)
    v = volumes[attempts // 10:]
    mean, var = v.mean() / ((N + 1) * v_unit), v.var() / ((N + 1) * v_unit ** 2)
    print(f"{mode}: mean / analytic = {mean:.4f}, variance / analytic = {var:.4f}, accepted {baro.accepted} of {baro.attempts}")
    assert baro.getVolumeScale() == 2.0 * np.sqrt(N + 1) * v_unit          # adapt=False
    assert abs(mean - 1.0) < 0.03
    assert abs(var - 1.0) < 0.08


class _Scripted:
    """potential_energy whose second call of every attempt decides it: +1e12 kJ/mol rejects, -1e12 accepts."""

    def __init__(self, decisions):
        self.decisions, self.calls = list(decisions), 0

    def __call__(self):
        self.calls += 1
        if self.calls % 2:
            return 0.0
        return -1e12 if self.decisions[self.calls // 2 - 1] else 1e12


@pytest.mark.parametrize("accepted_of_10,factor", [(0, 1 / 1.1), (2, 1 / 1.1), (3, 1.0), (7, 1.0), (8, 1.1), (10, 1.1)])
def test_adaptation_thresholds(accepted_of_10, factor):
    pos, mol = _system()
    ctx = R.StandInContext(pos, [3.0, 3.0, 3.0], mol, "double")
    baro = B.MonteCarloBarostat(1.0, 300.0, mode="z", seed=1)
    script = [k < accepted_of_10 for k in range(10)]
    energy = _Scripted(script)
    for k in range(10):
        assert baro.attempt(ctx, energy) == script[k]
        if k < 9:
            assert baro.getVolumeScale() == 0.01 * 27.0            # nothing moves before the tenth attempt
            assert baro.window_attempts == [k + 1]
    assert baro.getVolumeScale() == pytest.approx(0.01 * 27.0 * factor, rel=1e-15)
    assert baro.window_attempts == [0] and baro.window_accepted == [0]
    assert (baro.attempts, baro.accepted) == (10, accepted_of_10)


def test_adaptation_cap_frozen_step_and_per_group_counters():
    pos, mol = _system()
    # the cap: 1.1 x 0.29 V would pass 0.3 V
    ctx = R.StandInContext(pos, [3.0, 3.0, 3.0], mol, "double")
    baro = B.MonteCarloBarostat(1.0, 300.0, mode="iso", seed=1)
    baro.setVolumeScale(0.29 * 27.0)
    for _ in range(10):
        baro.attempt(ctx, _Scripted([True]))
    v_now = float(np.prod(ctx.box))
    assert baro.getVolumeScale() == min(0.29 * 27.0 * 1.1, 0.3 * v_now) and baro.getVolumeScale() <= 0.3 * v_now
    # adapt=False: the counters still turn over, the step stays
    ctx = R.StandInContext(pos, [3.0, 3.0, 3.0], mol, "double")
    frozen = B.MonteCarloBarostat(1.0, 300.0, mode="iso", seed=1, adapt=False)
    frozen.setVolumeScale(0.5)
    for _ in range(25):
        frozen.attempt(ctx, _Scripted([True]))
    assert frozen.getVolumeScale() == 0.5 and frozen.window_attempts == [5] and frozen.attempts == 25
    # per group: every attempt accepted, so a group's step grows by 1.1 exactly when ITS tenth attempt comes
    ctx = R.StandInContext(pos, [3.0, 3.0, 3.0], mol, "double")
    baro = B.MonteCarloBarostat(1.0, 300.0, mode="xyz", seed=4)
    count, grown = [0, 0, 0], [0, 0, 0]
    for _ in range(90):
        baro.attempt(ctx, _Scripted([True]))
        g = baro.last[0]
        count[g] += 1
        if count[g] % 10 == 0:
            grown[g] += 1
        for k in range(3):
            assert baro.window_attempts[k] == count[k] % 10
            assert baro.getVolumeScale(k) == pytest.approx(0.01 * 27.0 * 1.1 ** grown[k], rel=1e-14)
    assert min(grown) >= 1 and len(set(count)) > 1


def _harmonic(ctx, x0, k=2000.0):
    return lambda: 0.5 * k * float(np.sum((ctx.getPositions() - x0) ** 2))


def test_state_round_trip_continues_the_same_sequence():
    pos, mol = _system()
    x0 = pos.copy()

    def run(n_first, n_second, restart):
        ctx = R.StandInContext(pos, [3.0, 3.0, 3.0], mol, "mixed")
        baro = B.MonteCarloBarostat(1000.0, 300.0, mode="semi-iso", seed=7)
        out = [baro.attempt(ctx, _harmonic(ctx, x0)) for _ in range(n_first)]
        if restart:
            state = json.loads(json.dumps(baro.getState()))
            baro = B.MonteCarloBarostat(1000.0, 300.0, mode="semi-iso", seed=12345)
            baro.setState(state)
            kept = copy.deepcopy(ctx)
            ctx = kept
        out += [baro.attempt(ctx, _harmonic(ctx, x0)) for _ in range(n_second)]
        return out, ctx.box.tobytes(), ctx.posq.tobytes(), ctx.corr.tobytes(), baro.getState()

    whole, again = run(35, 35, False), run(35, 35, True)
    assert whole == again
    assert 0 < sum(whole[0]) < 70               # both outcomes occur
    other = B.MonteCarloBarostat(1.0, 300.0, mode="iso")
    with pytest.raises(ValueError):
        other.setState(whole[4])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rejected_attempt_leaves_the_arrays_bit_identical(precision):
    pos, mol = _system()
    ctx = R.StandInContext(pos, [3.0, 3.0, 3.0], mol, precision)
    before = (ctx.posq.tobytes(), ctx.corr.tobytes(), ctx.box.tobytes())
    baro = B.MonteCarloBarostat(1.0, 300.0, mode="iso", seed=3)
    assert baro.attempt(ctx, _Scripted([False])) is False
    assert len(ctx.scales_seen) == 1            # the move was made, then undone
    assert (ctx.posq.tobytes(), ctx.corr.tobytes(), ctx.box.tobytes()) == before
    assert (baro.attempts, baro.accepted) == (1, 0)


# ---------------------------------------------------------------------------------------------- the plan's host side (no GPU)
def test_unbound_plan_reports_its_host_fields_and_refuses_in_order():
    """vvhip_barostat_read fills molecules and F on an unbound plan; a bad scale component, then image pairs with scale[2] != 1, then the
    missing bind are what vvhip_barostat_scale says, in this order; a shard that cuts a molecule is named."""
    import ctypes as C
    import importlib

    import barostat_cases as K
    pkg = importlib.import_module("openmm-velocityverlet_amd")
    I, S = pkg.integrator, pkg.systems
    H = I.H
    vec = lambda *s: C.byref((C.c_double * 3)(*s))
    err = lambda p: H.lib.vvhip_last_error(p).decode()
    spec = K.synthetic()

    def plan_of(spec, shard=None, mirror=None):
        it = I.VVIntegrator(300.0, 10.0, 1.0, 40.0, 0.001)
        if len(spec.drude_pairs):
            it.setMaxDrudeDistance(0.02)
        else:
            it.setUseCOMTempGroup(False)
        if mirror is not None:
            it.setMirrorLocation(mirror)
        return I.create_plan(spec, it, "mixed", shard)

    plans = []
    try:
        plan, _, keep = plan_of(spec)
        plans.append(plan)
        rec = H.BarostatRecord()
        assert H.lib.vvhip_barostat_read(plan, C.byref(rec)) == H.OK
        assert (rec.molecules, rec.frac_bits, rec.pending, rec.scales, rec.restores) == (spec.num_molecules, R.frac_bits(spec.mol_id), 0, 0, 0)
        assert rec.frac_bits == 32                                      # the largest molecule has 130 particles: 40 - 8
        cut = K.shard_cut(spec)
        part, _, keep2 = plan_of(spec, (cut, spec.num_atoms))
        plans.append(part)
        assert H.lib.vvhip_barostat_read(part, C.byref(rec)) == H.OK
        assert rec.molecules == len(set(spec.mol_id[cut:].tolist())) and rec.frac_bits == 32      # F of the whole System
        torn, _, keep3 = plan_of(spec, (0, 3))
        plans.append(torn)
        assert H.lib.vvhip_barostat_scale(torn, vec(1.0, 1.0, 1.1)) == H.ERR_UNSUPPORTED and "cuts a molecule" in err(torn)
        edl = S.edl_slab(num_ion_pairs=4, num_electrode=16)
        images, _, keep4 = plan_of(edl, mirror=float(edl.box[2]) / 2)
        plans.append(images)
        assert H.lib.vvhip_barostat_scale(images, vec(1.0, float("nan"), 1.1)) == H.ERR_INVALID and "scale[1]" in err(images)
        assert H.lib.vvhip_barostat_scale(images, vec(1.0, 1.0, -1.1)) == H.ERR_INVALID and "scale[2]" in err(images)
        assert H.lib.vvhip_barostat_scale(images, vec(1.0, 1.0, 1.1)) == H.ERR_UNSUPPORTED and "mirror" in err(images)
        assert H.lib.vvhip_barostat_scale(images, vec(1.1, 1.0, 1.0)) == H.ERR_INVALID and "vvhip_bind" in err(images)
        assert H.lib.vvhip_barostat_restore(images) == H.ERR_INVALID and "vvhip_bind" in err(images)
    finally:
        for p in plans:
            H.lib.vvhip_plan_destroy(p)
