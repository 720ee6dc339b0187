// vv_barostat.cpp -- the device half of a Monte Carlo barostat attempt (include/vvhip.h: "Monte Carlo barostat"): every molecule moved
// rigidly with the box (vv_dev_barostat.inc), a backup that undoes the proposal bit for bit, the plan's box kept in step.  The decision
// itself -- a few host scalars per attempt and the host's potential energy, which this library does not own -- stays with the caller
// (openmm-velocityverlet_amd/barostat.py).  Host-driven between run calls, never captured, not a scheduled rider.
#include "vv_plan.hpp"

static int baro_ensure(vvhip_plan* p) {
    vvhip_plan::Barostat& B = p->baro;
    const vv::HostPlan& hp = p->hp;
    if (B.d_words && B.h_bad) return VVHIP_OK;
    HIP_TRY(p, vv::upload(B.d_lane_mol, hp.baro_lane_mol, 16));
    HIP_TRY(p, vv::upload(B.d_laneless, hp.baro_laneless, 16));
    HIP_TRY(p, vv::upload(B.d_mol_count, hp.baro_mol_count, 16));
    HIP_TRY(p, B.h_bad.alloc(sizeof(unsigned long long)));
    HIP_TRY(p, B.d_words.alloc((vv::BARO_HEAD + 3 * hp.baro_mol_count.size()) * sizeof(unsigned long long)));
    return VVHIP_OK;
}

extern "C" {

int vvhip_barostat_scale(vvhip_plan* p, const double scale[3]) {
    if (!p || !scale) return VVHIP_ERR_INVALID;
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(scale[k]) || !(scale[k] > 0))
            return fail(p, VVHIP_ERR_INVALID, std::string("barostat: scale[") + std::to_string(k) + "] = " + std::to_string(scale[k]) + " must be finite and > 0");
    if (p->hp.has_images && scale[2] != 1.0)
        return fail(p, VVHIP_ERR_UNSUPPORTED, "barostat: the System has image pairs and scale[2] != 1: the mirror plane would have to move with the box");
    if (!p->hp.baro_unsupported.empty()) return fail(p, VVHIP_ERR_UNSUPPORTED, "barostat: " + p->hp.baro_unsupported);
    NEED_BOUND(p);
    // (the library's own captures, and a host that is capturing the plan's stream itself: the call has to block for its bad word)
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (p->capturing || (hipStreamIsCapturing(p->stream, &capture) == hipSuccess && capture != hipStreamCaptureStatusNone))
        return fail(p, VVHIP_ERR_INVALID, "barostat: not inside a graph capture");
    TRY(vvhip_synchronize(p));      // (a missed rendezvous is repaired here; a sticky word ends the call: a void state is never scaled)
    TRY(baro_ensure(p));
    vvhip_plan::Barostat& B = p->baro;
    const vv::HostPlan& hp = p->hp;
    const size_t pos_bytes = (size_t) (hp.shard_end - hp.shard_begin) * 4 * sizeof_real(hp.precision);
    const bool mixed = hp.precision == VVHIP_MIXED;
    // a second scale while one is pending overwrites the backup: the implicit accept
    B.pending = false;
    HIP_TRY(p, B.posq.ensure(pos_bytes));
    HIP_TRY(p, hipMemcpyAsync(B.posq.get(), p->buf.posq, pos_bytes, hipMemcpyDeviceToDevice, p->stream));
    if (mixed) {
        HIP_TRY(p, B.corr.ensure(pos_bytes));
        HIP_TRY(p, hipMemcpyAsync(B.corr.get(), p->buf.posq_correction, pos_bytes, hipMemcpyDeviceToDevice, p->stream));
    }
    vv::BarostatArgs a{};
    a.posq = p->buf.posq; a.corr = posq_corr(p);
    a.slots = p->d_slots.get(); a.lane_mol = B.d_lane_mol.get(); a.laneless = B.d_laneless.get(); a.mol_count = B.d_mol_count.get();
    a.words = B.d_words.get();
    a.nwaves = hp.info.num_waves; a.nlaneless = (int32_t) (hp.baro_laneless.size() / 2); a.nmol = (int32_t) hp.baro_mol_count.size();
    a.frac_bits = hp.baro_frac_bits;
    a.scale = std::ldexp(1.0, hp.baro_frac_bits); a.inv_scale = std::ldexp(1.0, -hp.baro_frac_bits);
    for (int k = 0; k < 3; k++) a.e[k] = scale[k] - 1.0;
    HIP_TRY(p, hipMemsetAsync(B.d_words.get(), 0, B.d_words.bytes(), p->stream));
    HIP_TRY(p, vv::launch_barostat(hp.precision, a, p->block_threads, p->grid_cap_a, p->stream));
    HIP_TRY(p, hipMemcpyAsync(B.h_bad.get(), B.d_words.get() + vv::BARO_BAD, sizeof(unsigned long long), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    if (B.h_bad[0] != 0)
        return fail(p, VVHIP_ERR_OVERFLOW, "barostat: a position is not finite or beyond 2^22 nm; nothing was moved and the box stays");
    TRY(origins_dead(p, Rewrote::POSITIONS));
    for (int k = 0; k < 3; k++) { B.box_before[k] = p->box[k]; p->box[k] *= scale[k]; B.box_after[k] = p->box[k]; }
    drop_graphs(p);                 // the box is baked into the captured kernel arguments
    p->rec.valid = false;           // (a snapshot from before the scale would put the old positions back under the new box)
    p->rec.runs.clear();
    B.step_at_scale = p->cur.step_count;
    B.scales++;
    B.pending = true;
    return VVHIP_OK;
}

int vvhip_barostat_restore(vvhip_plan* p) {
    NEED_BOUND(p);
    vvhip_plan::Barostat& B = p->baro;
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "barostat: not inside a graph capture");
    if (!B.pending)
        return fail(p, VVHIP_ERR_INVALID, "barostat: no scale to undo (none done, already restored, or vvhip_set_box / vvhip_bind / vvhip_checkpoint_load came after it)");
    if (p->cur.step_count != B.step_at_scale) {
        B.pending = false;
        return fail(p, VVHIP_ERR_INVALID, "barostat: steps were taken since the scale: the backup no longer belongs to the state");
    }
    const vv::HostPlan& hp = p->hp;
    const size_t pos_bytes = (size_t) (hp.shard_end - hp.shard_begin) * 4 * sizeof_real(hp.precision);
    TRY(settle_recovery(p));
    HIP_TRY(p, hipMemcpyAsync(p->buf.posq, B.posq.get(), pos_bytes, hipMemcpyDeviceToDevice, p->stream));
    if (hp.precision == VVHIP_MIXED) HIP_TRY(p, hipMemcpyAsync(p->buf.posq_correction, B.corr.get(), pos_bytes, hipMemcpyDeviceToDevice, p->stream));
    TRY(origins_dead(p, Rewrote::POSITIONS));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    for (int k = 0; k < 3; k++) p->box[k] = B.box_before[k];
    drop_graphs(p);
    p->rec.valid = false;
    p->rec.runs.clear();
    B.pending = false;
    B.restores++;
    return VVHIP_OK;
}

int vvhip_barostat_read(vvhip_plan* p, vvhip_barostat_record* out) {
    if (!p || !out) return VVHIP_ERR_INVALID;
    const vvhip_plan::Barostat& B = p->baro;
    vvhip_barostat_record r{};
    r.molecules = (int64_t) p->hp.baro_mol_count.size();
    r.scales = B.scales; r.restores = B.restores;
    r.pending = B.pending && p->cur.step_count == B.step_at_scale ? 1 : 0;
    r.frac_bits = p->hp.baro_frac_bits;
    for (int k = 0; k < 3; k++) { r.box_before[k] = B.box_before[k]; r.box_after[k] = B.box_after[k]; }
    *out = r;
    return VVHIP_OK;
}

}  // extern "C"
