"""Maxwell-Boltzmann start velocities on the device (include/vvhip.h: vvhip_set_velocities_to_temperature) on the GPU: the raw draw
against the NumPy statement (tests/thermalize_reference.py); the same bits under every wave layout, launch shape and shard split; seeds;
the temperatures of the draw; the in-kernel velocity constraints on it; the removal of the centre-of-mass motion behind it; no hidden
state next to graph runs and a series; the refusals.  Systems and seeds: tests/thermalize_cases.py, whose bounds tests/test_thermalize.py
shows the statement itself to meet."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import thermalize_cases as K            # noqa: E402
import thermalize_reference as ref      # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S, I = pkg.systems, pkg.integrator
H = I.H

pytestmark = pytest.mark.gpu

NH_FIELDS = ("eta", "eta_dot", "eta_dotdot", "ke2", "vscale", "v_bias")
A_CONS = (1 << 16) | (1 << 22) | (1 << 23)       # csrc/vv_args.hpp: A_SHAKE_V | A_SETTLE | A_GCONS (tests/test_gpu_constraint_stages.py keeps the bits honest)
SEED = K.SEEDS[0]


@pytest.fixture(scope="module")
def specs():
    """Every system once per module (the constrained ones take a moment to build); tests do not change them."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = K.SYSTEMS[name]()
        return made[name]
    return get


@pytest.fixture(scope="module")
def reference(specs):
    """The statement's velocities, once per (system, seed, mode)."""
    made = {}

    def get(name, seed, drude):
        key = (name, seed, drude)
        if key not in made:
            spec = specs(name)
            made[key] = ref.velocities(spec.masses, spec.drude_pairs, K.T, seed, K.T_DRUDE if drude else None)
            made[key].setflags(write=False)
        return made[key]
    return get


def make(spec, precision="mixed", **kw):
    it = I.VVIntegrator(K.T, 10.0, K.T_DRUDE, 40.0, 0.001, 3, 1)
    it.setRandomNumberSeed(SEED)
    if len(spec.drude_pairs):
        it.setMaxDrudeDistance(0.02)
    if spec.image_pairs:
        it.setMirrorLocation(float(spec.box[2]) / 2)
    return it, I.Context(spec, it, precision=precision, force_provider="tether", **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def nh_arrays(ctx):
    st = ctx.getNHState()
    return [np.array(getattr(st, f)) for f in NH_FIELDS]


def untouched(ctx):
    """Everything the draw must leave alone: velm.w, positions, the correction, forces, the thermostat state, the four status words."""
    return [np.ascontiguousarray(ctx.getVelm()[:, 3]), ctx.getPosq(), ctx.getPosqCorrection(), ctx.getForce()] + nh_arrays(ctx) + [np.array(ctx.status_words())]


def state(ctx):
    return [ctx.getPosq(), ctx.getPosqCorrection(), ctx.getVelm()] + nh_arrays(ctx)


def cons_a_of(ctx):
    f = C.c_uint32()
    H.check(H.lib.vvhip_debug_fused_flags(ctx.plan, 0, C.byref(f)), ctx.plan)
    return f.value & A_CONS


# ------------------------------------------------------------------------------------------ 1. the raw draw against the statement
RAW = [(name, prec, drude) for name in ("il", "edl") for prec in ("single", "mixed", "double") for drude in (False, True)]


@pytest.mark.parametrize("name,precision,drude", RAW, ids=[f"{n}-{p}-{'drude' if d else 'plain'}" for n, p, d in RAW])
def test_raw_draw_equals_the_statement(specs, reference, name, precision, drude):
    """|v - v_ref| <= 1e-13 sigma_i + eps_store |v_ref| with sigma_i = sqrt(R T / m_i): the uniforms are exact in float64, log, sqrt and
    sincos a few ulp on |n| <= 6.7 (<= 1e-14 sigma; the bound allows ten times that); eps_store = 2^-23 where `mixed` is float, else 0."""
    spec = specs(name)
    m = np.asarray(spec.masses, dtype=np.float64)
    massive = m > 0
    v_ref = reference(name, SEED, drude)
    it, ctx = make(spec, precision)
    try:
        junk = np.array(spec.velocities, dtype=np.float64)
        junk[~massive] = 0.0123                                  # massless rows hold something that only a store of 0 removes
        junk[massive] += 7.0
        ctx.setVelocities(junk)
        before = untouched(ctx)
        rec = ctx.setVelocitiesToTemperature(K.T, drude_temperature=K.T_DRUDE if drude else None, constraints=False)      # (the integrator's seed)
        v = ctx.getVelocities()
        sigma = np.zeros_like(m)
        sigma[massive] = np.sqrt(ref.R * K.T / m[massive])
        eps_store = 2.0 ** -23 if precision == "single" else 0.0
        tol = 1e-13 * sigma[:, None] + eps_store * np.abs(v_ref)
        err = np.abs(v - v_ref)
        print(f"{name} {precision} {'drude' if drude else 'plain'}: max |v - v_ref| / sigma = {float((err[massive] / sigma[massive, None]).max()):.3e}, "
              f"max err / tol = {float((err[massive] / tol[massive]).max()):.3e}")
        assert np.all(err[massive] <= tol[massive])
        assert np.all(v[~massive] == 0.0) and not np.any(np.signbit(v[~massive]))
        assert same_bits(untouched(ctx), before)
        pairs = ref.split_pairs(m, spec.drude_pairs)
        assert (rec.drawn, rec.zeroed, rec.pairs_split) == (int(massive.sum()), int((~massive).sum()), len(pairs) if drude else 0)
        assert rec.constrained == 0 and rec.cm_removed == 0 and list(rec.v_removed) == [0.0, 0.0, 0.0]
        if name == "edl":
            assert rec.zeroed == len(spec.image_pairs) > 0 and ctx.info.num_slots_used < spec.num_atoms      # images: massless and without a lane
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 2. layout, launch shape and shard split
def _draw(spec, precision="mixed", drude=True, seed=SEED, **kw):
    it, ctx = make(spec, precision, **kw)
    try:
        ctx.setVelocitiesToTemperature(K.T, seed, K.T_DRUDE if drude else None, constraints=False)
        return ctx.getVelm(), ctx.info
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def il_default_draw(specs):
    velm, info = _draw(specs("il"))
    assert info.periodic_layout == 0 and info.num_waves > 8
    velm.setflags(write=False)
    return velm


def test_same_bits_under_the_arithmetic_wave_layout(specs, il_default_draw, monkeypatch):
    monkeypatch.setenv("VVHIP_PERIODIC", "1")
    velm, info = _draw(specs("il"))
    assert info.periodic_layout == 1                              # another slot order, another number of waves
    assert np.array_equal(bits(velm), bits(il_default_draw))


@pytest.mark.parametrize("tune", [{"block_threads": 128}, {"grid_cap_a": 1}, {"grid_cap_a": 3}], ids=["block_threads-128", "one-block", "three-blocks"])
def test_same_bits_with_the_launch_shape_tuned(specs, il_default_draw, tune):
    """The draw's kernel always runs 512-thread blocks, so its launch shape depends on grid_cap_a alone: a grid capped below the number
    of wave groups walks the rest with the kernel's stride.  block_threads shapes the plan's other launches (the constraint launch behind
    the draw among them), not this kernel: the case shows that the setting leaves the draw alone."""
    velm, _ = _draw(specs("il"), tune=tune)
    assert np.array_equal(bits(velm), bits(il_default_draw))


@pytest.mark.parametrize("precision", ["mixed", "single"])
def test_two_shards_concatenate_to_the_unsharded_draw(specs, il_default_draw, precision):
    spec = specs("il")
    mol = np.asarray(spec.mol_id)
    cut = int(np.nonzero(mol == mol[spec.num_atoms // 3])[0].min())      # a cut between molecules, not at a multiple of 64
    assert 0 < cut < spec.num_atoms and cut % 64 != 0
    whole = il_default_draw if precision == "mixed" else _draw(spec, precision)[0]
    parts = [_draw(spec, precision, shard=s)[0] for s in ((0, cut), (cut, spec.num_atoms))]
    assert parts[0].shape[0] == cut
    assert np.array_equal(bits(np.concatenate(parts)), bits(whole))


# ------------------------------------------------------------------------------------------ 3. seeds
def test_seeds(specs, il_default_draw):
    """The same seed twice: the same bits.  Another seed: other bits, and the normals (v / sigma_i, plain mode) of the two draws correlate
    below 5 / sqrt(3 N), five standard deviations of the correlation of 3 N independent pairs of normals."""
    spec = specs("il")
    m = np.asarray(spec.masses, dtype=np.float64)
    again, _ = _draw(spec)
    assert np.array_equal(bits(again), bits(il_default_draw))
    a, _ = _draw(spec, drude=False, seed=SEED)
    b, _ = _draw(spec, drude=False, seed=SEED + 1)
    c, _ = _draw(spec, drude=False, seed=K.SEEDS[1])
    sigma = np.sqrt(ref.R * K.T / m)[:, None]
    for other in (b, c):
        assert not np.array_equal(bits(a), bits(other))
        r = ref.correlation(a[:, :3] / sigma, other[:, :3] / sigma)
        print(f"correlation {r:.4e}, bound {5 / np.sqrt(3 * m.size):.4e}")
        assert abs(r) < 5 / np.sqrt(3 * m.size)


# ------------------------------------------------------------------------------------------ 4. temperatures
@pytest.mark.parametrize("name", K.STATISTICS)
@pytest.mark.parametrize("seed", K.SEEDS, ids=["seed0", "seed1"])
def test_temperatures_of_the_draw(specs, name, seed):
    """Five standard deviations of each estimator, sqrt(2 / dof) relative (tests/thermalize_cases.py); tests/test_thermalize.py shows that
    the statement passes with these systems and seeds."""
    spec = specs(name)
    m = np.asarray(spec.masses, dtype=np.float64)
    n_massive = int(np.count_nonzero(m > 0))
    it, ctx = make(spec)
    try:
        ctx.setVelocitiesToTemperature(K.T, seed, constraints=False)
        t = ref.plain_temperature(m, ctx.getVelocities())
        print(f"{name} seed {seed:#x}: plain T = {t:.3f} K, bound {K.plain_bound(m) * K.T:.3f} K")
        assert abs(t / K.T - 1) <= K.plain_bound(m)
        if name in K.DRUDE:
            pairs = ref.split_pairs(m, spec.drude_pairs)
            rec = ctx.setVelocitiesToTemperature(K.T, seed, K.T_DRUDE, constraints=False)
            assert rec.pairs_split == len(pairs) == len(spec.drude_pairs)      # (so the report's Drude DOF are 3 per split pair)
            t_drude = ctx.getDrudeTemperatures()[5]
            two_ke = ref.two_ke(m, ctx.getVelocities())
            mean, five_sd = K.total_2ke(n_massive, len(pairs), ref.R)
            print(f"{name} seed {seed:#x}: T_Drude = {t_drude:.4f} K, bound {K.drude_bound(len(pairs)) * K.T_DRUDE:.4f} K; 2KE = {two_ke:.2f}, expected {mean:.2f} +- {five_sd:.2f}")
            assert abs(t_drude / K.T_DRUDE - 1) <= K.drude_bound(len(pairs))
            assert abs(two_ke - mean) <= five_sd
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 5. constraints
CONSTRAINED = [(name, prec) for name in ("il_hbonds", "water", "il_allbonds") for prec in ("mixed", "double")]
REL_V = 1e-3       # nm/ps: tests/test_gpu_constraints.py's bound on the bond-parallel relative velocity at the default tolerance 1e-5


@pytest.mark.parametrize("name,precision", CONSTRAINED, ids=[f"{n}-{p}" for n, p in CONSTRAINED])
def test_constraints_are_applied_to_the_draw(specs, name, precision):
    spec = specs(name)
    cons = np.asarray(spec.constraints)
    free = np.ones(spec.num_atoms, bool)
    free[cons.ravel()] = False
    drude = len(spec.drude_pairs) > 0
    it1, ctx1 = make(spec, precision)
    it2, ctx2 = make(spec, precision)
    try:
        assert ctx1.info.constraints_fused and cons_a_of(ctx1) != 0
        assert (ctx1.info.num_shake_clusters > 0, ctx1.info.num_settle_clusters > 0, ctx1.info.num_general_constraints > 0) == \
            (name == "il_hbonds", name == "water", name == "il_allbonds")
        rec = ctx1.setVelocitiesToTemperature(K.T, drude_temperature=K.T_DRUDE if drude else None)
        assert rec.constrained == 1
        velm = ctx1.getVelm()
        x, v = ctx1.getPositions(), velm[:, :3].astype(np.float64)
        r = x[cons[:, 0]] - x[cons[:, 1]]
        rel = ((v[cons[:, 0]] - v[cons[:, 1]]) * r).sum(1) / np.sqrt((r * r).sum(1))
        raw_rec = ctx2.setVelocitiesToTemperature(K.T, drude_temperature=K.T_DRUDE if drude else None, constraints=False)
        assert raw_rec.constrained == 0
        raw = ctx2.getVelm()
        v_raw = raw[:, :3].astype(np.float64)
        rel_raw = ((v_raw[cons[:, 0]] - v_raw[cons[:, 1]]) * r).sum(1) / np.sqrt((r * r).sum(1))
        print(f"{name} {precision}: bond-parallel relative velocity raw {np.abs(rel_raw).max():.3e} -> {np.abs(rel).max():.3e} nm/ps, status {ctx1.status_words()}")
        assert np.abs(rel_raw).max() > 0.1                           # the raw draw violates them
        assert np.abs(rel).max() < REL_V
        assert ctx1.status_words() == [0, 0, 0, 0]
        assert free.any() == (name != "water")                       # (every particle of a rigid water is constrained)
        assert np.array_equal(bits(velm[free]), bits(raw[free]))     # outside the constraints: the raw draw's bits
        # the same as the raw draw followed by ONE launch of kernel A with the plan's constraint stages
        H.check(H.lib.vvhip_debug_launch(ctx2.plan, 0, cons_a_of(ctx2), 0), ctx2.plan)
        assert np.array_equal(bits(ctx2.getVelm()), bits(velm))
    finally:
        ctx1.close()
        ctx2.close()


# ------------------------------------------------------------------------------------------ 6. REMOVE_CM
def test_remove_cm(specs):
    spec = specs("il")
    m = np.asarray(spec.masses, dtype=np.float64)
    it1, ctx1 = make(spec)
    it2, ctx2 = make(spec)
    try:
        rec = ctx1.setVelocitiesToTemperature(K.T, drude_temperature=K.T_DRUDE, remove_cm=True)
        assert rec.cm_removed == 1 and rec.constrained == 0       # (no constraints in this System)
        v = ctx1.getVelocities()
        v_rms = float(np.sqrt(np.mean(np.sum(v ** 2, axis=1))))
        residual = float(np.linalg.norm(np.sum(m[:, None] * v, axis=0)) / np.sum(m))
        print(f"|sum m v| / M = {residual / v_rms:.3e} v_rms, removed {list(rec.v_removed)}")
        assert residual <= 1e-9 * v_rms                           # tests/test_gpu_cm_motion.py's bound outside single precision
        plain = ctx2.setVelocitiesToTemperature(K.T, drude_temperature=K.T_DRUDE)
        assert plain.cm_removed == 0
        V = ctx2.remove_cm_motion()
        assert np.array_equal(np.array(rec.v_removed).view(np.uint64), V.view(np.uint64)) and np.abs(V).max() > 0
        assert np.array_equal(bits(ctx1.getVelm()), bits(ctx2.getVelm()))
        assert ctx1.cm_motion_record().removals == 0              # a one-off removal: the schedule's record stays clean
    finally:
        ctx1.close()
        ctx2.close()


def test_remove_cm_is_refused_on_a_shard_with_the_velocities_untouched(specs):
    spec = specs("il")
    mol = np.asarray(spec.mol_id)
    cut = int(np.nonzero(mol == mol[spec.num_atoms // 2])[0].min())
    it, ctx = make(spec, shard=(0, cut))
    try:
        before = ctx.getVelm()
        with pytest.raises(H.VVHipError) as e:
            ctx.setVelocitiesToTemperature(K.T, remove_cm=True)
        assert e.value.code == H.ERR_UNSUPPORTED and "shard" in str(e.value)
        assert np.array_equal(bits(ctx.getVelm()), bits(before))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 7. no hidden state
def test_no_hidden_state_next_to_graph_runs_and_a_series(specs):
    """A context whose velocities were drawn on the device and one that got the same velocities through setVelocities run the same 40
    steps (graphs of 20: the one-launch step where it is the default) to the same bits; a later draw changes neither how the steps are
    launched nor a running series."""
    spec = specs("il")
    it1, ctx1 = make(spec)
    it2, ctx2 = make(spec)
    try:
        ctx1.setVelocitiesToTemperature(K.T, drude_temperature=K.T_DRUDE)
        ctx2.setVelocities(ctx1.getVelocities())
        assert np.array_equal(bits(ctx1.getVelm()), bits(ctx2.getVelm()))
        for ctx in (ctx1, ctx2):
            ctx.run_graph(40, steps_per_graph=20)
        assert same_bits(state(ctx1), state(ctx2))
        launched = (ctx1.generic_launches(), ctx1.fused_status(), ctx1.series_info().graph_captures, ctx1.series_info().steps)
        nh = nh_arrays(ctx1)
        ctx1.setVelocitiesToTemperature(K.T, SEED + 5, K.T_DRUDE)
        assert (ctx1.generic_launches(), ctx1.fused_status(), ctx1.series_info().graph_captures, ctx1.series_info().steps) == launched
        assert same_bits(nh_arrays(ctx1), nh)
        # ... and the graphs captured before the draw are still the ones that run
        ctx2.setVelocities(ctx1.getVelocities())
        for ctx in (ctx1, ctx2):
            ctx.run_graph(20, steps_per_graph=20)
        assert same_bits(state(ctx1), state(ctx2))
        assert ctx1.series_info().graph_captures == launched[2]
        # inside an active series: rows and cursor stay
        ctx1.series_start(10, capacity=8)
        ctx1.run_graph(20, steps_per_graph=20)
        rows = ctx1.series_read()
        assert len(rows) == 2 and rows.dropped == 0
        ctx1.setVelocitiesToTemperature(K.T, SEED + 6, K.T_DRUDE)
        after = ctx1.series_read()
        assert list(after.step) == list(rows.step) and after.dropped == 0
        assert same_bits([after.raw, after.eta, after.ke2, after.vscale], [rows.raw, rows.eta, rows.ke2, rows.vscale])
        ctx1.run_graph(10, steps_per_graph=10)
        assert list(ctx1.series_read().step) == list(rows.step) + [int(rows.step[-1]) + 10]      # the cursor went on from where it was
    finally:
        ctx1.close()
        ctx2.close()


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(specs):
    spec = specs("il")
    it, ctx = make(spec)
    plan2, _, keep = I.create_plan(spec, I.VVIntegrator(K.T, 10.0, K.T_DRUDE, 40.0, 0.001), "mixed")
    try:
        before = ctx.getVelm()
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(H.VVHipError) as e:
                ctx.setVelocitiesToTemperature(bad)
            assert e.value.code == H.ERR_INVALID and "temperature" in str(e.value)
        # an unbound plan
        assert H.lib.vvhip_set_velocities_to_temperature(plan2, K.T, -1.0, 1, 0, None) == H.ERR_INVALID
        assert "vvhip_bind" in H.lib.vvhip_last_error(plan2).decode()
        # inside a capture: the host is capturing the plan's stream (the call would have to block for its record)
        hip = C.CDLL("libamdhip64.so")
        graph = C.c_void_p()
        assert hip.hipStreamBeginCapture(C.c_void_p(ctx.stream), 2) == 0          # hipStreamCaptureModeRelaxed
        try:
            rc = H.lib.vvhip_set_velocities_to_temperature(ctx.plan, K.T, -1.0, 1, 0, None)
            msg = H.lib.vvhip_last_error(ctx.plan).decode()
        finally:
            assert hip.hipStreamEndCapture(C.c_void_p(ctx.stream), C.byref(graph)) == 0
            if graph.value:
                hip.hipGraphDestroy(graph)
        assert rc == H.ERR_INVALID and "capture" in msg
        assert np.array_equal(bits(ctx.getVelm()), bits(before))                  # nothing was drawn by any of them
        rec = ctx.setVelocitiesToTemperature(0.0)                                 # T = 0 is a temperature: everything at rest
        assert rec.drawn == spec.num_atoms and np.all(ctx.getVelocities() == 0.0)
    finally:
        H.lib.vvhip_plan_destroy(plan2)
        ctx.close()
