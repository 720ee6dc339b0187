"""Who owns the plan's memory (csrc/vv_devmem.hpp): every device buffer, pinned word and hipIpc mapping of a plan is held by an owner that
frees it, and vvhip_debug_live_buffers counts what the owners of this process hold.  Here: a plan gives everything back when it is destroyed
(also one whose bind failed), restarts of a series / a mailbox replace their buffers, and the recovery snapshot follows a re-bind to a
larger random buffer.  The counters, not the device's free memory: that moves under other processes' work."""
import ctypes as C
import gc
import importlib

import numpy as np
import pytest

pkg = importlib.import_module("openmm-velocityverlet_amd")
H, I, systems = pkg.vvhip, pkg.integrator, pkg.systems


def _live(settle=False):
    """settle: first let go of the contexts earlier tests dropped without closing them (a collection in the middle of a test would move the counters)"""
    if settle:
        gc.collect()
    n, b = C.c_int64(-1), C.c_int64(-1)
    assert H.lib.vvhip_debug_live_buffers(C.byref(n), C.byref(b)) == H.OK
    return n.value, b.value


def _integrator():
    it = I.VVIntegrator(333.0, 10.0, 1.0, 40.0, 0.001)
    it.setMaxDrudeDistance(0.02)
    return it


def _ion_pairs():
    return systems.drude_il(cells=(1, 1, 1), pairs_per_cell=8, seed=11)        # 8 Drude ion pairs


def test_live_buffers_is_exported_and_validates_its_arguments():
    assert "vvhip_debug_live_buffers" in H.EXPORTS
    n = C.c_int64()
    assert H.lib.vvhip_debug_live_buffers(None, C.byref(n)) == H.ERR_INVALID
    assert H.lib.vvhip_debug_live_buffers(C.byref(n), None) == H.ERR_INVALID


def test_a_bind_without_a_device_leaves_nothing_behind():
    if H.device_count() > 0:
        pytest.skip("a HIP device is present: vvhip_bind succeeds here (the GPU tests below cover that side)")
    plan, _, keep = I.create_plan(_ion_pairs(), _integrator(), "mixed")
    try:
        # (pointers that are never followed: the call stops at the missing device)
        fake = [C.create_string_buffer(64) for _ in range(4)]
        buf = H.Buffers(*[C.addressof(f) for f in fake], None, None, 0, None)
        assert H.lib.vvhip_bind(plan, C.byref(buf)) == H.ERR_NO_DEVICE
        assert _live() == (0, 0)
    finally:
        H.lib.vvhip_plan_destroy(plan)
    assert _live() == (0, 0)


# ------------------------------------------------------------------------------------------ on the device
def _context(spec, **kw):
    return I.Context(spec, _integrator(), precision="mixed", force_provider="tether", **kw)


def _state_bits(ctx):
    """positions (+ correction), velocities and the thermostat's state as bytes"""
    ctx.synchronize()
    parts = [ctx.getPosq(), ctx.getPosqCorrection(), ctx.getVelm()]
    return [np.ascontiguousarray(a).tobytes() for a in parts] + [bytes(ctx.getNHState())]


@pytest.mark.gpu
def test_a_destroyed_plan_has_returned_everything():
    spec = _ion_pairs()
    base = _live(settle=True)
    seen = []
    for _ in range(3):
        ctx = _context(spec)
        try:
            assert _live()[0] > base[0]
            ctx.series_start(8, capacity=32, drude=True, thermostat=True)
            ctx.remove_cm_motion_every(10)
            ctx.run_graph(64, steps_per_graph=64)              # (>= 64 steps: a run call worth a recovery snapshot, with its series and CM copies)
            ctx.synchronize()
            flags, out = C.c_uint32(0), (C.c_double * 8)()
            H.check(H.lib.vvhip_debug_fused_flags(ctx.plan, 1, C.byref(flags)), ctx.plan)
            rc = H.lib.vvhip_debug_span(ctx.plan, 1, flags.value, 2, C.byref(out))
            assert rc in (H.OK, H.ERR_UNSUPPORTED), rc         # (the stamps and their buffer only exist in an instrumented build)
            ctx.remove_cm_motion()
            ctx.mailbox_connect(ctx.mailbox_create(1, 0))
            live = _live()
            print("live buffers / bytes with everything in use:", live, "before the plan:", base)
            assert live[0] > base[0] and live[1] > base[1]
            seen.append(live[0])
        finally:
            ctx.close()
        assert _live() == base
    assert seen[0] == seen[1] == seen[2]


@pytest.mark.gpu
def test_restarts_replace_their_buffers_and_leave_the_run_alone():
    spec = _ion_pairs()
    gc.collect()
    ctx, fresh = _context(spec), None
    try:
        bound = _live()
        ctx.series_start(8, capacity=32)
        first = _live()
        assert first[0] == bound[0] + 3                        # rows, cursor, scratch
        ctx.series_start(8, capacity=32)
        assert _live() == first
        ctx.remove_cm_motion_every(10)
        with_cmm = _live()
        ctx.remove_cm_motion_every(10)
        assert _live() == with_cmm
        handle = ctx.mailbox_create(1, 0)
        created = _live()
        assert created[0] == with_cmm[0] + 2                   # the box and its control words
        handle = ctx.mailbox_create(1, 0)
        assert _live() == created
        ctx.mailbox_connect(handle)
        connected = _live()
        assert connected[0] == created[0] + 1                  # the peer table (one rank: no mapping of another process's box)
        ctx.mailbox_connect(handle)
        assert _live() == connected
        ctx.series_stop()
        ctx.remove_cm_motion_stop()
        ctx.mailbox_destroy()
        # What the three calls keep, from csrc/vv_observe.cpp and vv_exchange.cpp: vvhip_series_stop frees the series' three buffers (series_release) and
        # vvhip_mailbox_destroy the box, the control words and the peer table (mailbox_release) -- nothing stays.  vvhip_cm_motion_stop only
        # switches the schedule off: the removal's scratch words ([CMM_WORDS = 8] int64), its two records (2 x CmmDevRecord = 2 x 40 bytes) and
        # the pinned 3 doubles of the one-off call stay for vvhip_remove_cm_motion and the next schedule (cmm_ensure allocates them once).
        kept = (3, 8 * 8 + 2 * 40 + 3 * 8)
        assert _live() == (bound[0] + kept[0], bound[1] + kept[1])
        fresh = _context(spec)
        for c in (ctx, fresh):
            c.run_graph(64, steps_per_graph=64)
        assert _state_bits(ctx) == _state_bits(fresh)
    finally:
        ctx.close()
        if fresh is not None:
            fresh.close()


@pytest.mark.gpu
def test_the_snapshot_follows_a_rebind_to_a_larger_random_buffer():
    """Runs on this branch only: before the owners, the second snapshot copied 4R float4 into the R allocated for the first."""
    spec = systems.edl_slab(num_ion_pairs=2, num_electrode=60, seed=9)        # 60 Langevin electrode atoms, 2 Drude ion pairs, their images
    R = 4096                                                                   # 64 steps x (60 + 2) float4 per step fit: no refill inside a run

    def make(rows):
        it = _integrator()
        it.setMirrorLocation(float(spec.box[2]) / 2)
        ctx = I.Context(spec, it, precision="mixed", force_provider="tether", random=np.zeros((rows, 4), np.float32))
        H.check(H.lib.vvhip_set_random_seed(ctx.plan, 12345), ctx.plan)       # (the graphs refill the buffer from the device generator)
        return ctx

    gc.collect()
    a, b, big = make(R), None, None
    try:
        if not a.fused_status()[0]:
            pytest.skip("the one-launch step is not active for this plan on this device: no recovery snapshot is taken")
        a.run_graph(64, steps_per_graph=64)
        a.synchronize()
        before = _live()
        big = H.DeviceArray.from_host(np.zeros((4 * R, 4), np.float32))
        buf = H.Buffers(a.velm.ptr, a.posq.ptr, a.posq_corr.ptr, a.force.ptr, a.pos_delta.ptr, big.ptr, 4 * R, a.stream)
        H.check(H.lib.vvhip_bind(a.plan, C.byref(buf)), a.plan)
        a.run_graph(64, steps_per_graph=64)
        a.synchronize()
        after = _live()
        print("live bytes before / after the re-bind's snapshot:", before[1], after[1])
        assert after[1] - before[1] >= 3 * R * 16
        b = make(4 * R)
        b.run_graph(64, steps_per_graph=64)
        b.run_graph(64, steps_per_graph=64)
        assert _state_bits(a) == _state_bits(b)
    finally:
        a.close()
        if b is not None:
            b.close()
