// vv_debug.cpp -- test hooks and timing probes of the ABI, among them the four probes of the instrumented build (-DVV_KERNEL_TIMESTAMPS).
#include "vv_plan.hpp"

#include <algorithm>

namespace vv { unsigned vv_last_grid_value = 0; }      // grid of the most recent A / B launch, written by the launchers (vv_kernels.hip)

#ifdef VV_KERNEL_TIMESTAMPS
// The shader-clock stamps of one block (vvhip_debug_timestamps*): the buffer zeroed and aimed at `block` / read back once the stream has drained
static int arm_stamps(vvhip_plan* p, int block) {
    HIP_TRY(p, p->d_dbg.ensure(128 * sizeof(long long)));
    HIP_TRY(p, hipMemsetAsync(p->d_dbg.get(), 0, 128 * sizeof(long long), p->stream));
    p->dbg_block = block;
    return VVHIP_OK;
}
static int read_stamps(vvhip_plan* p, long long out[128]) {
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    HIP_TRY(p, hipMemcpy(out, p->d_dbg.get(), 128 * sizeof(long long), hipMemcpyDeviceToHost));
    return VVHIP_OK;
}
// The wall-clock spans of the waves (vvhip_debug_span, vvhip_debug_step_spans): six launches' worth of rows, one (entry, exit) pair per row
constexpr size_t kSpanRows = (size_t) 4096 * 8, kSpanWords = 6 * kSpanRows * 2;
// the non-zero (entry, exit) pairs of rows [r0, r1) of the host copy `h`; `which` takes r - r0 of each
static void span_pairs(const std::vector<long long>& h, size_t r0, size_t r1, std::vector<long long>& in, std::vector<long long>& ex, std::vector<size_t>* which = nullptr) {
    for (size_t r = r0; r < r1; r++) {
        const long long a0 = h[r * 2], a1 = h[r * 2 + 1];
        if (a0 && a1) { in.push_back(a0); ex.push_back(a1); if (which) which->push_back(r - r0); }
    }
}
#endif

// FNV-1a 64 over the host tables a recorder's start built (tests/test_recorder_tables.py pins them): per vector its size as uint64, then
// its bytes; scalars and arrays of scalars as their bytes.  The order is the one stated in include/vvhip.h, not the structs' declarations.
// Host only: an unbound plan keeps the description of a start that passed its checks.  0: nothing described.
namespace {
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void* q, size_t n) {
        const unsigned char* b = (const unsigned char*) q;
        for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    }
    template <class T> void scalar(const T& v) { static_assert(std::is_arithmetic<T>::value, "scalars only: a struct has padding"); bytes(&v, sizeof(T)); }
    template <class T, size_t N> void array(const T (&a)[N]) { static_assert(std::is_arithmetic<T>::value, "arrays of scalars only"); bytes(a, sizeof(a)); }
    void flag(bool b) { scalar((unsigned char) (b ? 1 : 0)); }
    // (the item structs of vv_args.hpp / vv_layout.h state their padding as zeroed members: bytes)
    template <class T> void vec(const std::vector<T>& v) { scalar((uint64_t) v.size()); if (!v.empty()) bytes(v.data(), v.size() * sizeof(T)); }
};
template <class U> void digest_units(Fnv& f, const U& u) { f.flag(u.grouped); f.vec(u.index); f.vec(u.first); f.vec(u.weight); f.vec(u.total); f.vec(u.group); }
}  // namespace

extern "C" {

// The stage bits vvhip_step_middle launches kernel A (kernel = 0) / kernel B with for this plan (timing and probe entry points)
int vvhip_debug_launch_shape(const vvhip_plan* p, int32_t shape[4]) {
    if (!p || !shape) return VVHIP_ERR_INVALID;
    shape[0] = p->block_threads; shape[1] = p->grid_cap_a; shape[2] = p->grid_cap_b;
    shape[3] = fused_shape_ok(p) ? p->block_threads / 64 : 0;
    return VVHIP_OK;
}
int vvhip_debug_fused_flags(vvhip_plan* p, int kernel, uint32_t* flags) {
    NEED_BOUND(p);
    if (!flags) return VVHIP_ERR_INVALID;
    const ThermoApp t = middle_application(p);
    // Phase 0's kernel A and the last phase's kernel B.  This accessor has never reported the load of a stale forceExtra, the cos(kz) store of a
    // plan without NH particles or the mailbox bit: the probes and bench.py time the sets without them, so they are masked out here.
    if (kernel == 0) *flags = t.a[0].flags & ~(vv::A_FE_LOAD | (t.mode == ThermoMode::NO_NH ? vv::A_CZ_STORE : 0u));
    else *flags = t.b | (t.mode == ThermoMode::NO_NH ? 0u : chain_in_b(p) & ~vv::B_MAILBOX);
    return VVHIP_OK;
}
int vvhip_time_kernel(vvhip_plan* p, int kernel, uint32_t flags, int reps, double* ms_per_launch) {
    NEED_BOUND(p);
    if (reps < 1 || !ms_per_launch) return VVHIP_ERR_INVALID;
    if (flags == 0xFFFFFFFFu) TRY(vvhip_debug_fused_flags(p, kernel, &flags));     // the stage bits vvhip_step_middle uses for this plan
    hipEvent_t e0, e1;
    HIP_TRY(p, hipEventCreate(&e0));
    HIP_TRY(p, hipEventCreate(&e1));
    const int parity = p->cur.parity;
    const bool was_timing = p->timing;
    p->timing = false;
    int rc = VVHIP_OK;
    for (int i = 0; i < 3 && rc == VVHIP_OK; i++) { p->cur.parity = parity; rc = kernel == 0 ? run_a(p, flags, 0) : run_b(p, flags); }
    HIP_TRY(p, hipEventRecord(e0, p->stream));
    for (int i = 0; i < reps && rc == VVHIP_OK; i++) { p->cur.parity = parity; rc = kernel == 0 ? run_a(p, flags, 0) : run_b(p, flags); }
    HIP_TRY(p, hipEventRecord(e1, p->stream));
    p->cur.parity = parity;
    p->timing = was_timing;
    if (rc != VVHIP_OK) return rc;
    HIP_TRY(p, hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(p, hipEventElapsedTime(&ms, e0, e1));
    (void) hipEventDestroy(e0);
    (void) hipEventDestroy(e1);
    *ms_per_launch = (double) ms / reps;
    return VVHIP_OK;
}

// Instrumented build (-DVV_KERNEL_TIMESTAMPS): one launch of kernel B with `flags`, shader-clock stamps of block `block`:
// out[w*16 + k] for tile waves w = 0.. (k = 0 entry, 1 loads arrived, 2 prep done, 3 scales received, 4 compute done, 5 stores
// drained) and w = 7 for the thermostat wave (0 entry, 1 accumulators folded, 2 chain done, 3 after the barrier).
int vvhip_debug_timestamps(vvhip_plan* p, uint32_t flags, int block, long long out[128]) {
    // bit 31 of `flags` selects kernel A (stamps: 0 entry, 1 velm arrived, 2 kicked + stored, 3 tile loop done, 4 sums added)
    NEED_BOUND(p);
#ifndef VV_KERNEL_TIMESTAMPS
    (void) flags; (void) block; (void) out;
    return fail(p, VVHIP_ERR_UNSUPPORTED, "not an instrumented build");
#else
    TRY(arm_stamps(p, block));
    const int parity = p->cur.parity;
    int rc = (flags & 0x80000000u) ? run_a(p, flags & 0x7FFFFFFFu, 0) : run_b(p, flags);
    p->cur.parity = parity;
    if (rc != VVHIP_OK) return rc;
    return read_stamps(p, out);
#endif
}

// Instrumented build: ONE real step of the one-launch path (it advances the state), shader-clock stamps of block `block`: tile waves
// w = 0..6: 0 entry, 6 loads arrived + extra forces, 7 kick + sums done, 8 partials in LDS, 9 behind barrier 1, 1 / 2 preparation, 3 scales
// received, 4 compute done, 5 stores drained; thermostat wave (w = 7): 0 entry, 6 at barrier 1, 7 behind it, 8 published, 9 all blocks' words
// held, 10 = poll rounds (a count, not a time), 1 folded, 4 ke2, 5 released, 2 chain done, 3 state stored.
int vvhip_debug_timestamps_fused(vvhip_plan* p, int block, long long out[128]) {
    NEED_BOUND(p);
#ifndef VV_KERNEL_TIMESTAMPS
    (void) block; (void) out;
    return fail(p, VVHIP_ERR_UNSUPPORTED, "not an instrumented build");
#else
    TRY(arm_stamps(p, block));
    bool taken = false;
    if (p->hp.params.use_middle_scheme && p->hp.info.constraints_fused) TRY(run_application_fused(p, middle_application(p), 0, &taken));
    if (!taken) return fail(p, VVHIP_ERR_UNSUPPORTED, "the plan does not take the one-launch step");
    return read_stamps(p, out);
#endif
}

// Instrumented build: `reps` back-to-back launches of kernel A (kernel = 0) or B (1) with `flags`; every wave stamps the 100 MHz
// wall clock at entry and (after draining its memory operations) at exit.  out[0] = first entry -> last exit of the last launch,
// out[1] = last exit of the launch before -> first entry of the last launch, out[2] = median wave entry - first entry,
// out[3] = median wave lifetime (all ns).
int vvhip_debug_span(vvhip_plan* p, int kernel, uint32_t flags, int reps, double out[8]) {
    NEED_BOUND(p);
#ifndef VV_KERNEL_TIMESTAMPS
    (void) kernel; (void) flags; (void) reps; (void) out;
    return fail(p, VVHIP_ERR_UNSUPPORTED, "not an instrumented build");
#else
    HIP_TRY(p, p->d_dbg_span.ensure(kSpanWords * sizeof(long long)));
    HIP_TRY(p, hipMemsetAsync(p->d_dbg_span.get(), 0, kSpanWords * sizeof(long long), p->stream));
    const int parity = p->cur.parity;
    int rc = VVHIP_OK;
    for (int i = 0; i < reps && rc == VVHIP_OK; i++) { p->cur.parity = parity; p->dbg_parity = i & 1; rc = kernel == 0 ? run_a(p, flags, 0) : run_b(p, flags); }
    p->cur.parity = parity;
    const int last = (reps - 1) & 1;
    p->dbg_parity = 0;
    if (rc != VVHIP_OK) return rc;
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    std::vector<long long> h(2 * kSpanRows * 2);
    HIP_TRY(p, hipMemcpy(h.data(), p->d_dbg_span.get(), h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    // the launch of parity q stamped the first 8 rows per block of its 4096 * 8: the non-zero pairs among them
    std::vector<long long> in[2], ex[2];
    std::vector<size_t> row[2];
    const size_t grid = vv::vv_last_grid_value;
    for (int q = 0; q < 2; q++) span_pairs(h, q * kSpanRows, q * kSpanRows + grid * 8, in[q], ex[q], &row[q]);
    if (in[0].empty() || in[1].empty()) return fail(p, VVHIP_ERR_INVALID, "no stamps recorded");
    const int L = last, P = 1 - last;
    const long long first_in = *std::min_element(in[L].begin(), in[L].end()), last_out = *std::max_element(ex[L].begin(), ex[L].end());
    const long long prev_out = *std::max_element(ex[P].begin(), ex[P].end());
    std::vector<long long> rel, life;
    for (size_t k = 0; k < in[L].size(); k++) { rel.push_back(in[L][k] - first_in); life.push_back(ex[L][k] - in[L][k]); }
    size_t worst = 0;
    for (size_t k = 0; k < in[L].size(); k++) if (ex[L][k] > ex[L][worst]) worst = k;
    out[6] = (double) (row[L][worst] / 8); out[7] = (double) (in[L][worst] - first_in) * 10.0;
    std::sort(rel.begin(), rel.end()); std::sort(life.begin(), life.end());
    out[4] = (double) life[life.size() * 9 / 10] * 10.0; out[5] = (double) life.back() * 10.0;
    out[0] = (double) (last_out - first_in) * 10.0; out[1] = (double) (first_in - prev_out) * 10.0;
    out[2] = (double) rel[rel.size() / 2] * 10.0; out[3] = (double) life[life.size() / 2] * 10.0;
    return VVHIP_OK;
#endif
}

// Instrumented build: `nsteps` consecutive fused steps enqueued from here (force provider -> kernel A -> kernel B; middle scheme), every wave
// of the LAST TWO steps stamping the 100 MHz wall clock at entry and (memory operations drained) at exit.  For the six launches
// (provider, A, B of the step before the last; provider, A, B of the last) out[l*6 ..] = first wave in, median wave in, last wave in,
// first wave out, median wave out, last wave out, in ns after the first entry of the first of them.  What a kernel costs IN ITS PLACE:
// ramp, body, tail and the gap to its neighbours, none of which a profiler's per-kernel duration separates.
int vvhip_debug_step_spans(vvhip_plan* p, int nsteps, const void* site, double k_tether, double k_drude, double out[36]) {
    NEED_BOUND(p);
#ifndef VV_KERNEL_TIMESTAMPS
    (void) nsteps; (void) site; (void) k_tether; (void) k_drude; (void) out;
    return fail(p, VVHIP_ERR_UNSUPPORTED, "not an instrumented build");
#else
    if (nsteps < 2 || !site || !out || !p->hp.params.use_middle_scheme || vvhip_step_middle_phases(p) != 2) return VVHIP_ERR_INVALID;
    const ForceProvider fp{site, k_tether, k_drude};
    HIP_TRY(p, p->d_dbg_span.ensure(kSpanWords * sizeof(long long)));
    TRY(ensure_mass_table(p));
    for (int i = 0; i < nsteps - 2; i++) TRY(plan_step(p, fp, false));      // warm: same launches, rows overwritten below
    HIP_TRY(p, hipMemsetAsync(p->d_dbg_span.get(), 0, kSpanWords * sizeof(long long), p->stream));
    p->dbg_seq = 0;
    int rc = VVHIP_OK;
    const long long fused_before = p->fused_launches;
    for (int i = 0; i < 2 && rc == VVHIP_OK; i++) rc = plan_step(p, fp, false);
    p->dbg_seq = -1;
    if (rc != VVHIP_OK) return rc;
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    std::vector<long long> h(kSpanWords);
    HIP_TRY(p, hipMemcpy(h.data(), p->d_dbg_span.get(), h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    long long t0 = 0;
    // (the one-launch step: provider + one kernel per step, four launches; rows 4 and 5 stay zero)
    const int nlaunch = p->fused_launches > fused_before ? 4 : 6;
    for (int l = 0; l < 36; l++) out[l] = 0;
    for (int l = 0; l < nlaunch; l++) {
        std::vector<long long> in, ex;
        span_pairs(h, l * kSpanRows, (l + 1) * kSpanRows, in, ex);
        if (in.empty()) return fail(p, VVHIP_ERR_INVALID, "no stamps recorded for one of the launches");
        std::sort(in.begin(), in.end()); std::sort(ex.begin(), ex.end());
        if (l == 0) t0 = in.front();
        const long long v[6] = {in.front(), in[in.size() / 2], in.back(), ex.front(), ex[ex.size() / 2], ex.back()};
        for (int k = 0; k < 6; k++) out[l * 6 + k] = (double) (v[k] - t0) * 10.0;
    }
    return VVHIP_OK;
#endif
}

// ------------------------------------------------------------------------------------------ test hooks
int vvhip_debug_launch(vvhip_plan* p, int kernel, uint32_t flags, uint32_t random_index) {
    NEED_BOUND(p);
    if (kernel == 0) return run_a(p, flags, random_index);
    if (kernel == 1) return run_b(p, flags);
    if (kernel == 2) return run_chain(p, flags);
    return VVHIP_ERR_INVALID;
}
int vvhip_debug_read_accumulators(vvhip_plan* p, double out[4], int zero_after) {
    NEED_BOUND(p);
    static long long raw[vv::NUM_ACC * vv::ACC_SLOTS];
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    HIP_TRY(p, hipMemcpy(raw, p->d_acc.get() + p->cur.parity * acc_stride(p), 4 * vv::ACC_SLOTS * sizeof(long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; i++) {                 // the ABI hands out the three group sums and the bias moment
        long long s = 0;
        for (int j = 0; j < vv::ACC_SLOTS; j++) s += raw[i * vv::ACC_SLOTS + j];
        out[i] = (double) s * p->acc_inv_scale[i];
    }
    if (zero_after) HIP_TRY(p, hipMemsetAsync(p->d_acc.get() + p->cur.parity * acc_stride(p), 0, 4 * vv::ACC_SLOTS * sizeof(long long), p->stream));
    return VVHIP_OK;
}
int vvhip_debug_set_scales(vvhip_plan* p, const double scales[4]) {
    NEED_BOUND(p);
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    HIP_TRY(p, hipMemcpy(p->d_nh.get()[p->cur.parity].scales, scales, 4 * sizeof(double), hipMemcpyHostToDevice));
    return VVHIP_OK;
}

int vvhip_debug_old_delta(vvhip_plan* p, void** device_ptr) {
    NEED_BOUND(p);
    if (!device_ptr) return VVHIP_ERR_INVALID;
    *device_ptr = p->d_old_delta.get();
    return VVHIP_OK;
}
int vvhip_debug_live_buffers(int64_t* count, int64_t* bytes) {
    if (!count || !bytes) return VVHIP_ERR_INVALID;
    *count = (int64_t) vv::live_buffers.load();
    *bytes = (int64_t) vv::live_bytes.load();
    return VVHIP_OK;
}
int vvhip_debug_series_guard(vvhip_plan* p, int32_t* intact) {
    NEED_BOUND(p);
    if (!intact) return VVHIP_ERR_INVALID;
    if (!p->series.on) return fail(p, VVHIP_ERR_INVALID, "series: none started (vvhip_series_start)");
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    HIP_TRY(p, p->series.ring.guard_intact(intact));
    return VVHIP_OK;
}
int vvhip_debug_frames_guard(vvhip_plan* p, int32_t* intact) {
    NEED_BOUND(p);
    if (!intact) return VVHIP_ERR_INVALID;
    if (!p->frames.on) return fail(p, VVHIP_ERR_INVALID, "frames: none started (vvhip_frames_start)");
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    HIP_TRY(p, p->frames.ring.guard_intact(intact));
    return VVHIP_OK;
}
int vvhip_debug_recover(vvhip_plan* p) {
    NEED_BOUND(p);
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "vvhip_debug_recover: not inside a graph capture");
    if (!p->rec.valid || p->rec.replaying) return fail(p, VVHIP_ERR_INVALID, "vvhip_debug_recover: no unverified snapshot (a run call of at least recover_min_steps steps since the last synchronisation)");
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    return recover_rendezvous(p, true);
}
// The digest of one recorder's host tables (Fnv, digest_units: the top of the file; include/vvhip.h states the order)
int vvhip_debug_recorder_digest(const vvhip_plan* p, const char* name, uint64_t* out) {
    if (!p || !name || !out) return VVHIP_ERR_INVALID;
    const std::string which(name);
    Fnv f;
    bool described = false;
    if (which == "profile") {
        const vvhip_plan::Profile& R = p->profile;
        described = R.described;
        f.flag(R.grouped); f.vec(R.index); f.vec(R.group); f.vec(R.mass);
    } else if (which == "msd") {
        described = p->msd.described;
        digest_units(f, p->msd);
    } else if (which == "acf") {
        described = p->acf.described;
        digest_units(f, p->acf);
    } else if (which == "vanhove") {
        described = p->vanhove.described;
        digest_units(f, p->vanhove);
        f.vec(p->vanhove.e2);
    } else if (which == "rdf") {
        const vvhip_plan::Rdf& R = p->rdf;
        described = R.described;
        f.vec(R.index); f.vec(R.mol); f.vec(R.items); f.scalar((int32_t) R.max_jsites);
    } else if (which == "vanhove_distinct") {
        const vvhip_plan::Vhd& R = p->vhd;
        described = R.described;
        f.vec(R.index); f.vec(R.mol); f.vec(R.items); f.scalar((int32_t) R.max_jsites);
    } else if (which == "sdf") {
        const vvhip_plan::Sdf& R = p->sdf;
        described = R.described;
        f.vec(R.index); f.vec(R.mol); f.vec(R.frames); f.vec(R.fmol); f.vec(R.fgroup); f.vec(R.items); f.scalar((int32_t) R.max_jsites);
    } else if (which == "current") {
        const vvhip_plan::Current& R = p->current;
        described = R.described;
        f.flag(R.two_level); f.vec(R.index); f.vec(R.weight); f.vec(R.group);
    } else if (which == "modes") {
        const vvhip_plan::Modes& R = p->modes;
        described = R.described;
        f.vec(R.index); f.vec(R.weight); f.vec(R.modes); f.vec(R.items);
    } else if (which == "contacts") {
        const vvhip_plan::Contacts& R = p->contacts;
        const vv::ContactsLayout& G = R.geo;
        described = R.described;
        f.array(R.first); f.vec(R.index); f.vec(R.mol); f.vec(R.mask_items); f.vec(R.corr_items);
        f.array(G.rows_padded); f.array(G.col_words); f.array(G.class_words); f.array(G.class_offset);
        f.scalar(G.sample_words); f.scalar(G.num_origins); f.scalar(G.ord_words); f.scalar(G.table_words); f.scalar(G.ring_words);
        f.scalar(G.words_bytes); f.scalar(G.scratch_bytes); f.scalar(G.total_bytes);
    } else return VVHIP_ERR_INVALID;
    *out = described ? f.h : 0;
    return VVHIP_OK;
}

}  // extern "C"
