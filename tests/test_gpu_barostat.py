"""The Monte Carlo barostat's device half (include/vvhip.h: vvhip_barostat_*) on the GPU: a scale against the NumPy / Python-integer
reference (tests/barostat_reference.py) bit for bit in the three precisions; nothing else moves; a restore is the state before, bit for
bit; overflow; shards; the refusals in their order; the new box reaches the steps, a series row and a checkpoint; and the driver
(openmm-velocityverlet_amd/barostat.py) on the GPU context against the same driver on the NumPy stand-in.  The system:
tests/barostat_cases.py."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import barostat_cases as K              # noqa: E402
import barostat_reference as ref        # noqa: E402
import checkpoint_cases as CK           # noqa: E402
import thermalize_cases as TK           # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
S, I = pkg.systems, pkg.integrator
H = I.H
B = pkg.barostat

pytestmark = pytest.mark.gpu

PRECISIONS = ("single", "mixed", "double")
SCALES = [(1.01, 1.01, 1.01), (0.97, 1.0, 1.2), (1.0, 1.0, 1.0000001)]
OTHERS = ("velm", "force", "force_extra", "random", "thermostat", "epoch", "cursor")      # the digest words a scale must leave alone


@pytest.fixture(scope="module")
def spec():
    s = K.synthetic()
    for a in (s.positions, s.masses, s.mol_id):
        a.setflags(write=False)
    return s


def make(spec, precision="mixed", cos=0.0, **kw):
    it = I.VVIntegrator(300.0, 10.0, 1.0, 40.0, 0.001, 3, 1)
    if len(spec.drude_pairs):
        it.setMaxDrudeDistance(0.02)
    else:
        it.setUseCOMTempGroup(False)            # (the molecule of 130 particles spans three waves)
    if spec.image_pairs:
        it.setMirrorLocation(float(spec.box[2]) / 2)
    if cos:
        it.setCosAcceleration(cos)
    return it, I.Context(spec, it, precision=precision, force_provider="tether", **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def arrays(ctx):
    return ctx.getPosq(), ctx.getPosqCorrection()


def expected(ctx, spec, scale, posq=None, corr=None):
    b, e = ctx.shard
    posq, corr = (ctx.getPosq(), ctx.getPosqCorrection()) if posq is None else (posq, corr)
    return ref.scale(posq, corr, np.asarray(spec.mol_id)[b:e], scale, ctx.precision, ref.frac_bits(spec.mol_id))


def code_of(call):
    with pytest.raises(H.VVHipError) as e:
        call()
    return e.value.code, str(e.value)


# ------------------------------------------------------------------------------------------ 1. a scale against the reference
@pytest.mark.parametrize("precision", PRECISIONS)
def test_scale_equals_the_reference_bit_for_bit_and_nothing_else_moves(spec, precision):
    it, ctx = make(spec, precision)
    try:
        slots = np.zeros((ctx.info.num_waves * 64, 2), dtype=np.int32)
        assert H.lib.vvhip_plan_get_slots(ctx.plan, slots.ctypes.data, slots.shape[0]) == slots.shape[0]
        big = np.flatnonzero(np.asarray(spec.mol_id) == K.N_SINGLE)
        assert len({int(k) // 64 for k in np.flatnonzero(np.isin(slots[:, 0], big))}) >= 3       # the big molecule spans three waves
        assert (slots[:, 0] < 0).any() and ctx.info.num_slots_used < spec.num_atoms             # idle lanes; particles without a lane
        assert ctx.info.num_waves > 8                                                           # a second block
        rec = ctx.barostat_record()
        assert (rec.molecules, rec.frac_bits, rec.pending, rec.scales) == (spec.num_molecules, 32, 0, 0)
        box = np.array(spec.box, dtype=np.float64)
        for k, s in enumerate(SCALES):
            posq0, corr0 = arrays(ctx)
            want_posq, want_corr = expected(ctx, spec, s, posq0, corr0)
            other = ctx.state_digest()
            ctx.scale_box(s)
            posq1, corr1 = arrays(ctx)
            assert np.array_equal(bits(posq1), bits(want_posq)), (precision, s)
            assert np.array_equal(bits(corr1), bits(want_corr)), (precision, s)
            assert np.array_equal(bits(posq1[:, 3]), bits(posq0[:, 3])) and np.array_equal(bits(corr1[:, 3]), bits(corr0[:, 3]))
            for a in range(3):
                if s[a] == 1.0:
                    assert np.array_equal(bits(posq1[:, a]), bits(posq0[:, a])) and np.array_equal(bits(corr1[:, a]), bits(corr0[:, a]))
                else:
                    assert not np.array_equal(bits(posq1[:, a]), bits(posq0[:, a]))
            now = ctx.state_digest()
            assert {n: now[n] for n in OTHERS} == {n: other[n] for n in OTHERS}
            box = box * np.array(s)
            rec = ctx.barostat_record()
            assert np.array_equal(ctx.getPeriodicBoxSize(), box) and list(rec.box_after) == box.tolist()
            assert (rec.pending, rec.scales, rec.restores) == (1, k + 1, 0)
        assert ctx.status_words() == [0, 0, 0, 0]
    finally:
        ctx.close()


@pytest.mark.parametrize("tune", [{"block_threads": 128}, {"grid_cap_a": 1}, {"grid_cap_a": 3}], ids=["block_threads-128", "one-block", "three-blocks"])
def test_same_bits_with_the_launch_shape_tuned(spec, tune):
    it, ctx = make(spec, "mixed", tune=tune)
    try:
        want = expected(ctx, spec, SCALES[1])
        ctx.scale_box(SCALES[1])
        got = arrays(ctx)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 2. restore
@pytest.mark.parametrize("precision", PRECISIONS)
def test_restore_is_the_state_before_bit_for_bit(spec, precision):
    it, ctx = make(spec, precision)
    try:
        code, msg = code_of(ctx.restore_box)                                   # nothing pending
        assert code == H.ERR_INVALID and "no scale" in msg
        ctx.run_eager(2)
        before, box = ctx.state_digest(), ctx.getPeriodicBoxSize()
        ctx.scale_box(SCALES[1])
        assert ctx.state_digest()["posq"] != before["posq"]
        ctx.restore_box()
        assert ctx.state_digest() == before
        assert np.array_equal(ctx.getPeriodicBoxSize(), box)
        rec = ctx.barostat_record()
        assert (rec.pending, rec.scales, rec.restores) == (0, 1, 1) and list(rec.box_before) == box.tolist()
        assert code_of(ctx.restore_box)[0] == H.ERR_INVALID                    # once only
        # a second scale while one is pending is the implicit accept: the restore goes back to the state between the two
        ctx.scale_box(SCALES[0])
        between, box_between = ctx.state_digest(), ctx.getPeriodicBoxSize()
        ctx.scale_box(SCALES[1])
        ctx.restore_box()
        assert ctx.state_digest() == between and np.array_equal(ctx.getPeriodicBoxSize(), box_between)
        # after a step
        ctx.scale_box(SCALES[0])
        ctx.run_eager(1)
        assert ctx.barostat_record().pending == 0
        code, msg = code_of(ctx.restore_box)
        assert code == H.ERR_INVALID and "steps" in msg
        # after set_box, with the very box the plan holds too
        ctx.scale_box(SCALES[0])
        ctx.setPeriodicBoxSize(*ctx.getPeriodicBoxSize())
        assert code_of(ctx.restore_box)[0] == H.ERR_INVALID
        assert ctx.status_words() == [0, 0, 0, 0]
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 3. overflow
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("bad", [2.0 ** 23, float("nan")], ids=["2^23", "nan"])
def test_position_out_of_range_changes_nothing(spec, precision, bad):
    it, ctx = make(spec, precision)
    try:
        good = ctx.getPosq()
        broken = good.copy()
        broken[1234, 1] = bad                                                  # a one-particle molecule, in a lane
        ctx.posq.upload(broken)
        before, box = ctx.state_digest(), ctx.getPeriodicBoxSize()
        code, msg = code_of(lambda: ctx.scale_box(SCALES[0]))
        assert code == H.ERR_OVERFLOW and "2^22" in msg
        assert ctx.state_digest() == before and np.array_equal(ctx.getPeriodicBoxSize(), box)
        assert ctx.barostat_record().pending == 0 and ctx.barostat_record().scales == 0
        assert code_of(ctx.restore_box)[0] == H.ERR_INVALID
        assert ctx.status_words() == [0, 0, 0, 0]                              # this call only: nothing sticky
        ctx.posq.upload(good)
        want = expected(ctx, spec, SCALES[0])
        ctx.scale_box(SCALES[0])                                               # the next valid call works
        got = arrays(ctx)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 4. shards
@pytest.mark.parametrize("precision", ["mixed", "single"])
def test_two_shards_concatenate_to_the_unsharded_result(spec, precision):
    cut = K.shard_cut(spec)

    def scaled(shard):
        it, ctx = make(spec, precision, shard=shard)
        try:
            assert ctx.barostat_record().frac_bits == 32                       # of the whole System on every shard
            ctx.scale_box(SCALES[1])
            return arrays(ctx)
        finally:
            ctx.close()

    whole = scaled(None)
    parts = [scaled((0, cut)), scaled((cut, spec.num_atoms))]
    assert parts[0][0].shape[0] == cut
    for k in range(2):
        assert np.array_equal(bits(np.concatenate([parts[0][k], parts[1][k]])), bits(whole[k]))
    # a shard that cuts a molecule is refused
    it, ctx = make(spec, precision, shard=(0, 3))
    try:
        code, msg = code_of(lambda: ctx.scale_box(SCALES[1]))
        assert code == H.ERR_UNSUPPORTED and "cuts a molecule" in msg
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 5. refusals, in their order; image pairs
def test_refusals_in_their_order_and_image_pairs():
    edl = TK.edl()
    it, ctx = make(edl)
    it2 = I.VVIntegrator(300.0, 10.0, 1.0, 40.0, 0.001)
    it2.setMaxDrudeDistance(0.02)
    it2.setMirrorLocation(float(edl.box[2]) / 2)
    plan2, _, keep = I.create_plan(edl, it2, "mixed")                          # unbound, with image pairs
    vec = lambda *s: C.byref((C.c_double * 3)(*s))
    err = lambda p: H.lib.vvhip_last_error(p).decode()
    try:
        # 1. a bad component wins over everything behind it
        for k, bad in enumerate((float("nan"), 0.0, -1.0, float("inf"))):
            s = [1.0, 1.0, 1.1]
            s[k % 3] = bad
            assert H.lib.vvhip_barostat_scale(plan2, vec(*s)) == H.ERR_INVALID and f"scale[{k % 3}]" in err(plan2)
        # 2. image pairs with scale[2] != 1, also on an unbound plan
        assert H.lib.vvhip_barostat_scale(plan2, vec(1.0, 1.0, 1.1)) == H.ERR_UNSUPPORTED and "mirror" in err(plan2)
        # 3. an unbound plan
        assert H.lib.vvhip_barostat_scale(plan2, vec(1.1, 1.0, 1.0)) == H.ERR_INVALID and "vvhip_bind" in err(plan2)
        assert H.lib.vvhip_barostat_restore(plan2) == H.ERR_INVALID
        rec = H.BarostatRecord()
        assert H.lib.vvhip_barostat_read(plan2, C.byref(rec)) == H.OK and rec.molecules == edl.num_molecules and rec.pending == 0
        # 4. inside a capture: the host is capturing the plan's stream (the call would have to block for its bad word)
        before = ctx.state_digest()
        hip = C.CDLL("libamdhip64.so")
        graph = C.c_void_p()
        assert hip.hipStreamBeginCapture(C.c_void_p(ctx.stream), 2) == 0      # hipStreamCaptureModeRelaxed
        try:
            rc = H.lib.vvhip_barostat_scale(ctx.plan, vec(1.1, 1.0, 1.0))
            msg = err(ctx.plan)
        finally:
            assert hip.hipStreamEndCapture(C.c_void_p(ctx.stream), C.byref(graph)) == 0
            if graph.value:
                hip.hipGraphDestroy(graph)
        assert rc == H.ERR_INVALID and "capture" in msg
        code, msg = code_of(lambda: ctx.scale_box((1.0, 1.0, 0.99)))
        assert code == H.ERR_UNSUPPORTED and "mirror" in msg
        assert ctx.state_digest() == before and ctx.barostat_record().pending == 0
        # scale[2] == 1 is taken: the images (massless, without a lane) move with their molecules, bit for bit as the reference says
        assert ctx.info.num_slots_used < edl.num_atoms
        want = expected(ctx, edl, (1.01, 0.97, 1.0))
        ctx.scale_box((1.01, 0.97, 1.0))
        got = arrays(ctx)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
        ctx.restore_box()
        assert ctx.state_digest() == before
    finally:
        H.lib.vvhip_plan_destroy(plan2)
        ctx.close()


# ------------------------------------------------------------------------------------------ 6. the box reaches the steps
def test_box_reaches_graph_steps_series_rows_and_checkpoints():
    """With the cos acceleration the box enters the step's arithmetic (cos(2 pi z / Lz)): after the same scale, 100 steps through captured
    graphs equal 100 eager steps digest for digest -- a graph that kept the old box would not --; a series row recorded afterwards carries
    the new box; a checkpoint taken after scale + steps restarts bit for bit, and there is nothing to restore after its load.  Two RUNS
    are compared as the checkpoint tests compare them (tests/checkpoint_cases.py: state / assert_same): every array and every digest,
    the thermostat section without the 8 bytes per copy of the rendezvous' self-tuning wait, which follow the blocks' timing."""
    il = TK.il()
    s = (1.02, 0.99, 1.05)
    it1, ctx1 = make(il, cos=0.02)
    it2, ctx2 = make(il, cos=0.02)
    it3, ctx3 = make(il, cos=0.02)
    try:
        for ctx in (ctx1, ctx2):
            ctx.run_graph(50, 50)                                               # (ctx1 now holds graphs captured with the old box)
            ctx.scale_box(s)
        assert ctx1.state_digest() == ctx2.state_digest()
        ctx1.series_start(50, capacity=4, drude=False)
        ctx1.run_graph(100, 50)
        ctx2.run_eager(100)
        d1 = ctx1.state_digest()
        CK.assert_same(CK.state(ctx1), CK.state(ctx2), "graph against eager steps after the scale")
        rows = ctx1.series_read()
        new_box = np.array(il.box, dtype=np.float64) * np.array(s)
        assert len(rows) == 2 and all(list(b) == new_box.tolist() for b in rows.box)
        ctx1.series_stop()
        # the old box gives other bits: the check above can fail
        ctx3.run_graph(50, 50)
        ctx3.scale_box(s)
        ctx3.setPeriodicBoxSize(*il.box)
        ctx3.run_graph(100, 50)
        assert ctx3.state_digest()["velm"] != d1["velm"]
        # checkpoint after scale + steps
        blob = ctx1.createCheckpoint()
        ctx1.run_graph(50, 50)
        ctx3.scale_box((1.1, 1.1, 1.1))
        ctx3.loadCheckpoint(blob)
        assert np.array_equal(ctx3.getPeriodicBoxSize(), new_box)
        assert code_of(ctx3.restore_box)[0] == H.ERR_INVALID                    # the backup does not travel, and the load ends a pending scale
        ctx3.run_graph(50, 50)
        CK.assert_same(CK.state(ctx3), CK.state(ctx1), "restart from a checkpoint taken after scale + steps")
    finally:
        for ctx in (ctx1, ctx2, ctx3):
            ctx.close()


# ------------------------------------------------------------------------------------------ 7. end to end
def test_driver_on_the_gpu_context_equals_the_driver_on_the_stand_in(spec):
    """50 attempts of MonteCarloBarostat(mode="semi-iso") with the same seed on the GPU context and on the NumPy stand-in, the energy a
    NumPy harmonic function of the downloaded positions: the same accept / reject sequence, the same final box and position bits."""
    x0 = np.array(spec.positions, dtype=np.float64)

    def harmonic(ctx):
        return lambda: 0.5 * K.E2E_SPRING * float(np.sum((ctx.getPositions() - x0) ** 2))

    it, gpu = make(spec, "mixed")
    cpu = ref.StandInContext(spec.positions, spec.box, spec.mol_id, "mixed", charges=spec.charges)
    try:
        assert np.array_equal(bits(gpu.getPosq()), bits(cpu.posq)) and np.array_equal(bits(gpu.getPosqCorrection()), bits(cpu.corr))
        outcomes = []
        for ctx in (gpu, cpu):
            baro = B.MonteCarloBarostat(K.E2E_PRESSURE_BAR, 300.0, mode="semi-iso", seed=99)
            outcomes.append([baro.attempt(ctx, harmonic(ctx)) for _ in range(50)])
        assert outcomes[0] == outcomes[1]
        assert 5 <= sum(outcomes[0]) <= 45                                      # both outcomes occur
        assert np.array_equal(gpu.getPeriodicBoxSize().view(np.uint64), cpu.getPeriodicBoxSize().view(np.uint64))
        assert np.array_equal(bits(gpu.getPosq()), bits(cpu.posq)) and np.array_equal(bits(gpu.getPosqCorrection()), bits(cpu.corr))
        rec = gpu.barostat_record()
        assert rec.scales == 50 and rec.restores == 50 - sum(outcomes[0])
    finally:
        gpu.close()
