"""-m gpu: checkpoints and the state digest on the device (include/vvhip.h: "checkpoint").  Every comparison of two states is bitwise;
the one exception (the rendezvous' self-tuning wait) is stated in tests/checkpoint_cases.py.  Systems: D (Drude ionic liquid, 15 pairs),
W (22 rigid waters: one wave and a bit, SETTLE), E (electrode slab: Langevin subset, images, field, device generator), H (D with
hydrogen constraints).  Nothing here provokes a fault or a missed rendezvous."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import checkpoint_cases as K       # noqa: E402
import digest_reference as ref     # noqa: E402

pkg = importlib.import_module("openmm-velocityverlet_amd")
H, I, systems, reporters = pkg.vvhip, pkg.integrator, pkg.systems, pkg.reporters
pytestmark = pytest.mark.gpu


def _live():
    n, b = C.c_int64(0), C.c_int64(0)
    assert H.lib.vvhip_debug_live_buffers(C.byref(n), C.byref(b)) == H.OK
    return n.value


# ------------------------------------------------------------------------------------------ 1. the digest
def _numpy_digests(ctx):
    """Every section's digest from the arrays as downloaded (thermostat, epoch and cursor: from the payloads a save downloads)."""
    b = ctx.shard[0]
    R, M = np.dtype(H.REAL[ctx.precision]).itemsize, np.dtype(H.MIXED_T[ctx.precision]).itemsize
    fe_ptr = C.c_void_p()
    H.check(H.lib.vvhip_force_extra(ctx.plan, C.byref(fe_ptr)), ctx.plan)
    ctx.synchronize()
    fe = np.empty((ctx.nloc, 3), dtype=H.REAL[ctx.precision])
    assert H.lib.vvhip_memcpy_d2h(fe.ctypes.data, fe_ptr, fe.nbytes) == H.OK
    _, sections = ref.read_blob(ctx.createCheckpoint())
    has_ld = ctx.info.num_normal_ld + ctx.info.num_pairs_ld > 0
    return dict(posq=ref.digest(ctx.getPosq(), b * R), correction=ref.digest(ctx.getPosqCorrection(), b * R) if ctx.precision == "mixed" else 0,
                velm=ref.digest(ctx.getVelm(), b * M), force=ref.digest(ctx.getForce()), force_extra=ref.digest(fe, b * 3 * R // 4),
                random=ref.digest(ctx.random.download()) if has_ld else 0, thermostat=ref.digest(sections["thermostat"][1]),
                epoch=ref.digest(sections["epoch"][1]), cursor=ref.digest(sections["cursor"][1]))


def _tune(ctx, **kw):
    for k, v in kw.items():
        H.check(H.lib.vvhip_debug_tune(ctx.plan, k.encode(), int(v)), ctx.plan)


@pytest.mark.parametrize("prec", ["single", "mixed", "double"])
@pytest.mark.parametrize("name", ["D", "W"])
def test_digest_equals_numpy_whatever_the_launch_shape(name, prec):
    """The same state digested with the launch shape the plan chose, with a forced one (128-thread blocks, three of them at most: the
    kernel strides) and with loaded slot words: the same words, equal to NumPy on the downloaded arrays."""
    it, ctx = K.make(name, prec)
    try:
        it.step(7)
        got = ctx.state_digest()
        want = _numpy_digests(ctx)
        assert got == want, [k for k in want if want[k] != got[k]]
        assert got["random"] == 0 and (got["correction"] != 0) == (prec == "mixed") and all(got[k] != 0 for k in ("posq", "velm", "force", "thermostat", "cursor"))
        assert ctx.state_digest() == got                                 # reading it changes nothing
        _tune(ctx, block_threads=128, grid_cap_a=3)
        assert ctx.state_digest() == got, "forced launch shape"
        _tune(ctx, periodic_kernels=0)
        assert ctx.state_digest() == got, "loaded slot words"
    finally:
        ctx.close()
    for tune in (dict(block_threads=128, grid_cap_a=3), dict(periodic_kernels=0)):      # ... and in plans that were made that way
        it, ctx = K.make(name, prec, tune=tune)
        try:
            it.step(7)
            got = ctx.state_digest()
            want = _numpy_digests(ctx)
            assert got == want, (tune, [k for k in want if want[k] != got[k]])
        finally:
            ctx.close()


def test_digest_of_langevin_system_and_shard_additivity():
    it, ctx = K.make("E")
    try:
        it.step(7)
        got = ctx.state_digest()
        assert got == _numpy_digests(ctx) and got["random"] != 0
    finally:
        ctx.close()
    spec = K.system("D")
    mol = np.asarray(spec.mol_id)
    cut = int(np.nonzero(mol == mol[spec.num_atoms // 2])[0].min())          # a molecule boundary
    parts = []
    for shard in (None, (0, cut), (cut, spec.num_atoms)):
        it, ctx = K.make("D", shard=shard)
        try:
            parts.append(ctx.state_digest())
            if shard is not None:
                assert parts[-1] == _numpy_digests(ctx)
        finally:
            ctx.close()
    for k in ("posq", "correction", "velm", "force_extra"):
        assert (parts[1][k] + parts[2][k]) & ref.M64 == parts[0][k], k


# ------------------------------------------------------------------------------------------ 2. restart in a fresh context
SPLIT = (23, 17)      # (an odd count: the save falls on thermostat parity 1)
RESTART = [("D", "single", True, 0.0, "step"), ("D", "double", True, 0.0, "step")] + \
          [(n, "mixed", m, c, how) for (n, m, c) in (("D", True, 0.0), ("W", True, 0.0), ("H", True, 0.0), ("E", True, 0.0), ("D", False, 0.0),
                                                    ("E", False, 0.0), ("D", True, 0.02)) for how in ("step", "eager", "graph")]


def _restart(name, prec, middle, cos, how, split=SPLIT, spg=4):
    it, ctx = K.make(name, prec, middle, cos)
    try:
        K.drive(it, ctx, how, split[0], spg)
        K.drive(it, ctx, how, split[1], spg)
        whole = K.state(ctx)
    finally:
        ctx.close()
    it, ctx = K.make(name, prec, middle, cos)
    try:
        K.drive(it, ctx, how, split[0], spg)
        saved = K.state(ctx)
    finally:
        ctx.close()
    it, ctx = K.make(name, prec, middle, cos)                               # the "new process": nothing but the blob survives
    try:
        ctx.loadCheckpoint(saved["blob"])
        K.assert_same(saved, K.state(ctx), "right after the load")
        assert (ctx.random_index, ctx.forces_valid) == (saved["random_index"], saved["forces_valid"])
        K.drive(it, ctx, how, split[1], spg)
        K.assert_same(whole, K.state(ctx), f"{name}/{prec}/middle={middle}/cos={cos}/{how}")
        assert ctx.series_info().steps == sum(split)                        # the step counter travelled
    finally:
        ctx.close()


@pytest.mark.parametrize("name,prec,middle,cos,how", RESTART)
def test_restart_in_a_fresh_context_continues_bit_for_bit(name, prec, middle, cos, how):
    _restart(name, prec, middle, cos, how)


def test_restart_of_langevin_graph_replays():
    """E through run_graph(100, 50) before and after the save: every replay refills the normals, so the continuation needs the generator's
    epoch and seed and the random cursor."""
    _restart("E", "mixed", True, 0.0, "graph", split=(100, 100), spg=50)


# ------------------------------------------------------------------------------------------ 3. rewind in the same plan
@pytest.mark.parametrize("how", ["eager", "graph"])
def test_rewind_in_the_same_plan_with_the_one_launch_step(how):
    """30 steps, save, 30 steps (A), load, 30 steps (B): steps 31..60 carry the same rendezvous tags both times, so stale words would
    pass for fresh ones if the load did not clear them."""
    it, ctx = K.make("D")
    try:
        assert ctx.fused_status()[0]
        K.drive(it, ctx, how, 30, 10)
        saved = K.state(ctx)
        K.drive(it, ctx, how, 30, 10)
        a = K.state(ctx)
        launches = ctx.fused_status()[1]
        ctx.loadCheckpoint(saved["blob"])
        K.assert_same(saved, K.state(ctx), "right after the load")
        K.drive(it, ctx, how, 30, 10)
        K.assert_same(a, K.state(ctx), f"rewind/{how}")
        assert ctx.fused_status()[0] and ctx.fused_status()[1] > launches and ctx.recovery_count() == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 4. across configurations of the plan
@pytest.mark.parametrize("tune", [dict(fused=0), dict(block_threads=128, grid_cap_a=3, grid_cap_b=2)], ids=["two launches", "launch shape"])
def test_a_blob_continues_in_a_differently_tuned_plan(tune):
    """A blob saved by the default plan, loaded into a plan MADE with another configuration, continues to the bits of the run that took
    the same configuration at the same step without going through a blob (the default plan, retuned after step 23)."""
    it, ctx = K.make("D")
    try:
        it.step(23)
        blob = ctx.createCheckpoint()
        it.step(17)
        default = K.state(ctx)
    finally:
        ctx.close()
    it, ctx = K.make("D")
    try:
        it.step(23)
        _tune(ctx, **tune)
        it.step(17)
        whole = K.state(ctx)
    finally:
        ctx.close()
    if "fused" in tune:      # the two-launch step is the one-launch step's bits (the thermostat copies differ in rv_seq, which counts one-launch steps)
        for k in ("posq", "correction", "velm", "force"):
            assert np.array_equal(default[k].view(np.uint8), whole[k].view(np.uint8)), k
    it, ctx = K.make("D", tune=tune)
    try:
        assert ctx.fused_status()[0] == (False if "fused" in tune else ctx.fused_status()[0])
        ctx.loadCheckpoint(blob)
        it.step(17)
        K.assert_same(whole, K.state(ctx), str(tune))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 5. schedules follow the step counter
def test_series_and_removal_schedules_continue_at_the_same_steps():
    def observed(ctx):
        s = ctx.series_read()
        rows = {int(st): (s.raw[j].tobytes(), s.eta[j].tobytes(), s.ke2[j].tobytes()) for j, st in enumerate(s.step)}
        return rows, ctx.cm_motion_record()
    it, ctx = K.make("D")
    try:
        ctx.series_start(7, 16)
        ctx.remove_cm_motion_every(5)
        ctx.run_eager(40)
        rows_whole, rec_whole = observed(ctx)
        whole = K.state(ctx)
    finally:
        ctx.close()
    assert sorted(rows_whole) == [7, 14, 21, 28, 35] and rec_whole.removals == 8      # in front of steps 0, 5, .., 35
    it, ctx = K.make("D")
    try:
        ctx.series_start(7, 16)
        ctx.remove_cm_motion_every(5)
        ctx.run_eager(23)
        blob = ctx.createCheckpoint()
        with pytest.raises(H.VVHipError) as e:                                        # a running series refuses the load
            ctx.loadCheckpoint(blob)
        assert e.value.code == H.ERR_INVALID and "series" in e.value.message
    finally:
        ctx.close()
    it, ctx = K.make("D")
    try:
        ctx.loadCheckpoint(blob)
        ctx.series_start(7, 16)
        ctx.remove_cm_motion_every(5)
        ctx.run_eager(17)
        rows, rec = observed(ctx)
        assert sorted(rows) == [28, 35] and all(rows[k] == rows_whole[k] for k in rows)
        assert rec.removals == len([s for s in range(23, 40) if s % 5 == 0]) == 3     # in front of steps 25, 30, 35
        K.assert_same(whole, K.state(ctx), "schedules")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 6. sections
def test_integrator_sections_plus_hand_uploads_continue_as_the_full_blob():
    it, ctx = K.make("D", middle=False)
    try:
        it.step(23)
        full, part = ctx.createCheckpoint("all"), ctx.createCheckpoint("integrator")
        arrays = dict(posq=ctx.getPosq(), correction=ctx.getPosqCorrection(), velm=ctx.getVelm(), force=ctx.getForce())
        table = H.checkpoint_sections(full)
        assert len(full) - len(part) == sum(ref.align16(arrays[k].nbytes) for k in arrays) + 4 * 40
        assert list(H.checkpoint_sections(part)) == ["force_extra", "thermostat", "epoch", "cursor"]
        assert all(table[k].bytes == arrays[k].nbytes for k in arrays)
        it.step(17)
        whole = K.state(ctx)
    finally:
        ctx.close()
    it, ctx = K.make("D", middle=False)
    try:
        ctx.posq.upload(arrays["posq"]); ctx.posq_corr.upload(arrays["correction"]); ctx.velm.upload(arrays["velm"]); ctx.force.upload(arrays["force"])
        ctx.loadCheckpoint(part)
        it.step(17)
        K.assert_same(whole, K.state(ctx), "integrator sections")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 7. refusals and integrity
def test_refusals_leave_the_state_untouched_and_close_returns_every_buffer():
    start = _live()
    it, ctx = K.make("D")
    try:
        it.step(5)
        blob = ctx.createCheckpoint()
        it.step(3)
        before = ctx.state_digest()
        s = H.checkpoint_sections(blob)["velm"]
        at = s.offset + s.bytes // 2
        with pytest.raises(H.VVHipError) as e:
            ctx.loadCheckpoint(blob[:at] + bytes([blob[at] ^ 4]) + blob[at + 1:])
        assert e.value.code == H.ERR_INVALID and "velm" in e.value.message
        assert ctx.state_digest() == before
        for other, kw in (("W", {}), ("D", dict(prec="double")), ("D", dict(middle=False))):
            it2, ctx2 = K.make(other, **kw)
            try:
                before2 = ctx2.state_digest()
                with pytest.raises(H.VVHipError) as e:
                    ctx2.loadCheckpoint(blob)
                assert e.value.code == H.ERR_INVALID and "differs" in e.value.message, e.value.message
                assert ctx2.state_digest() == before2
            finally:
                ctx2.close()
        with pytest.raises(H.VVHipError) as e:
            ctx.createCheckpoint(1 << 12)
        assert e.value.code == H.ERR_INVALID
    finally:
        ctx.close()
    spec = K.system("D")
    mol = np.asarray(spec.mol_id)
    cut = int(np.nonzero(mol == mol[spec.num_atoms // 2])[0].min())
    it, ctx = K.make("D", shard=(0, cut))
    try:
        before = ctx.state_digest()
        part = ctx.createCheckpoint()                                              # save and digest work on a shard
        assert H.checkpoint_inspect(part).shard_end == cut
        with pytest.raises(H.VVHipError) as e:
            ctx.loadCheckpoint(part)
        assert e.value.code == H.ERR_UNSUPPORTED and "shard" in e.value.message
        assert ctx.state_digest() == before
    finally:
        ctx.close()
    assert _live() == start


# ------------------------------------------------------------------------------------------ 8. the reporter
class _Simulation:
    """The duck-typed simulation the reporters take: currentStep, context, integrator."""

    def __init__(self, it, ctx):
        self.integrator, self.context, self.currentStep = it, ctx, 0

    def step(self, n, reporters_):
        while n > 0:
            k = min([n] + [r.describeNextReport(self)[0] for r in reporters_])
            self.integrator.step(k)
            self.currentStep += k
            n -= k
            for r in reporters_:
                if self.currentStep % r._reportInterval == 0:
                    r.report(self, None)


def test_checkpoint_reporter_keeps_the_latest_three(tmp_path):
    it, ctx = K.make("D")
    try:
        sim = _Simulation(it, ctx)
        rep = reporters.CheckpointReporter(str(tmp_path / "cpt"), 10)
        sim.step(50, [rep])
        assert sorted(os.listdir(tmp_path)) == ["cpt_30", "cpt_40", "cpt_50"]
        blobs = {f: open(tmp_path / f, "rb").read() for f in os.listdir(tmp_path)}
        for f, b in blobs.items():
            assert H.checkpoint_inspect(b).cursor.step_count == int(f.split("_")[1])
        it.step(9)
        whole = K.state(ctx)
    finally:
        ctx.close()
    for f in ("cpt_30", "cpt_40", "cpt_50"):
        it, ctx = K.make("D")
        try:
            ctx.loadCheckpoint(blobs[f])                                           # each is loadable
            if f == "cpt_50":
                it.step(9)
                K.assert_same(whole, K.state(ctx), "from the newest file")
        finally:
            ctx.close()
