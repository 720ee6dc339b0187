// vv_steps.cpp -- the step entry points: a thermostat application with the stages that ride on it, composed in one place
// (compose_application) and launched as one, two or three kernels; the split (kernel-interface) entry points; what the step must move.
#include "vv_plan.hpp"

// The fused middle step without a velm round trip between its kernels: kernel A keeps the kicked velocities in registers, kernel B
// repeats the kick from velm + force (vv_args.hpp: A_NOSTORE / B_KICK).  Needs what A adds to the velocities beyond the plain
// kick to be absent or cheap to repeat: no Langevin subset and no field (kernel B repeats the cos force from the cached cos(kz), in
// the two-launch moment form only), no in-kernel velocity constraints; and a thermostat, i.e. the A -> B pair of one step
// (test hook "rekick" = 0 switches it off: comparison runs).
static bool use_rekick(const vvhip_plan* p) {
    const uint32_t ex = extra_flags(p);
    const bool extra_ok = ex == 0 || (ex == vv::A_COS && thermo_mode(p) == ThermoMode::COS_MOMENTS);
    const bool stale_extra = ex == 0 && stale_fextra(p) != 0;      // the kick must add what forceExtra holds
    return p->rekick && p->hp.has_nh && extra_ok && !stale_extra && !shake_on(p) && p->hp.num_big == 0;
}

// `a_first` rides in front of the sums (kick, extra forces, velocity constraints), `b_extra` behind the scaling (drift, hard wall, sites,
// images, position constraints, the classic half kick).  `elide` = the kicked velocities need not travel from kernel A to kernel B
// through velm: B repeats the kick (use_rekick).
static ThermoApp compose_application(ThermoMode mode, uint32_t a_first, uint32_t b_extra, bool elide) {
    ThermoApp t;
    t.mode = mode;
    t.fe_virtual = (a_first & (vv::A_COS | vv::A_LD | vv::A_EF | vv::A_FE_STORE)) == vv::A_COS;
    t.a[0].flags = a_first;
    t.b = b_extra;
    if (mode == ThermoMode::NO_NH) return t;
    const bool cos = mode != ThermoMode::PLAIN;
    uint32_t front = a_first, back = vv::B_SCALE | b_extra;      // kernel A in front of the sums; kernel B from the scale factors on
    if (cos) { front |= vv::A_BIAS | vv::A_CZ_STORE; back |= vv::B_UNBIAS; }
    // (the per-lane cos(kz) travels from kernel A to kernel B: letting kernel B evaluate its own -- no 8-byte store / load per lane, ~45
    // more instructions per wave in B -- measured 74.5 k against 74.9 k steps/s at C4, profiles/r04b_ab_C4_cos_variants.txt)
    if (mode == ThermoMode::COS_MOMENTS) { front |= vv::A_KE_MOM; back |= vv::B_KE_MOM; }      // bias moment and group moments in one launch
    // the hand-over between the launches: the kick through velm or repeated, the cos(kz) cache
    const uint32_t hand_a = elide ? vv::A_NOSTORE : 0u, hand_b = (elide ? vv::B_KICK : 0u) | (cos ? vv::B_CZ_LOAD : 0u);
    t.b = back | hand_b;
    t.with_bias = cos;
    if (mode == ThermoMode::COS_THREE_LAUNCH) {      // API:252-259: bias -> remove -> scale -> restore; the sums wait for the bias moment's exchange
        t.phases = 3;
        t.a[0] = {front | hand_a, false};
        t.a[1] = {vv::A_KE | vv::A_UNBIAS_ACC | vv::A_CZ_LOAD, true};      // (the bias launch of this step cached cos(kz))
        return t;
    }
    t.phases = 2;
    t.a[0] = {front | vv::A_KE | hand_a, true};
    t.one_launch = true;
    t.fused_a = front | vv::A_KE;
    t.fused_b = back;
    return t;
}

static int run_application_phase(vvhip_plan* p, const ThermoApp& t, int phase, uint32_t random_index) {
    if (phase < 0 || phase >= t.phases) return fail(p, VVHIP_ERR_INVALID, "phase out of range");
    if (phase == 0 && t.fe_virtual) p->cur.fextra_virtual = true;
    if (t.mode == ThermoMode::NO_NH) {
        if (t.a[0].flags) TRY(run_a(p, t.a[0].flags, random_index));
        return t.b ? run_b(p, t.b) : VVHIP_OK;
    }
    if (phase == t.phases - 1) return run_chain_and_b(p, t.b, t.with_bias);
    const uint32_t ri = phase == 0 ? random_index : 0;
    return t.a[phase].sums ? run_ke(p, t.a[phase].flags, ri) : run_a(p, t.a[phase].flags, ri);
}
// One launch where the application and the plan allow it (bit for bit the phases)
int run_application_fused(vvhip_plan* p, const ThermoApp& t, uint32_t random_index, bool* taken) {
    *taken = false;
    if (!t.one_launch) return VVHIP_OK;
    TRY(run_fused(p, t.fused_a, t.fused_b, random_index, taken));
    if (*taken && t.fe_virtual) p->cur.fextra_virtual = true;      // as phase 0 of the launches
    return VVHIP_OK;
}
static int run_application(vvhip_plan* p, const ThermoApp& t, uint32_t random_index, bool exchange = true) {
    bool taken = false;
    TRY(run_application_fused(p, t, random_index, &taken));
    if (taken) return VVHIP_OK;
    for (int ph = 0; ph < t.phases; ph++) {
        TRY(run_application_phase(p, t, ph, random_index));
        if (exchange && ph < t.phases - 1) TRY(exchange_accumulators(p, ph));
    }
    return VVHIP_OK;
}

// The middle scheme's step (API:237-268) is one application: the full kick in front of the sums, the drift behind the scaling.
ThermoApp middle_application(const vvhip_plan* p) {
    const ThermoMode mode = thermo_mode(p);
    // with sources of extra forces they are formed on the fly and the forceExtra array is out of date from here on
    const uint32_t ex = extra_flags(p);
    uint32_t kick = vv::A_KICK_FULL | (ex ? ex : stale_fextra(p)) | cons_a(p);
    // (without NH particles the kick caches cos(kz) all the same: vvhip_set_params rebuilds the stale forceExtra from it)
    if (mode == ThermoMode::NO_NH && cos_on(p)) kick |= vv::A_CZ_STORE;
    return compose_application(mode, kick, vv::B_DRIFT_MIDDLE | tail_flags(p) | cons_b(p), use_rekick(p));
}

// NH half-step used by the classic scheme (API:295-304, 327-336); `b_extra` is fused into the scaling kernel.
static int nh_half(vvhip_plan* p, uint32_t a_first, uint32_t random_index, uint32_t b_extra) {
    return run_application(p, compose_application(thermo_mode(p), a_first, b_extra, false), random_index);
}

extern "C" {

// ------------------------------------------------------------------------------------------ fused path
int vvhip_step_middle_phases(const vvhip_plan* p) {
    if (!p) return VVHIP_ERR_INVALID;
    const ThermoMode mode = thermo_mode(p);
    return mode == ThermoMode::NO_NH ? 1 : mode == ThermoMode::COS_THREE_LAUNCH ? 3 : 2;
}

// (the last phase completes the step: it is counted, and takes its series row)
int vvhip_step_middle_phase(vvhip_plan* p, int phase, uint32_t random_index) {
    NEED_BOUND(p);
    NEED_FUSABLE(p);
    if (phase == 0) TRY(step_begin(p));
    const ThermoApp t = middle_application(p);
    TRY(run_application_phase(p, t, phase, random_index));
    return phase == t.phases - 1 ? step_done(p) : VVHIP_OK;
}
int vvhip_step_middle(vvhip_plan* p, uint32_t random_index) {
    NEED_BOUND(p);
    if (!p->hp.params.use_middle_scheme) return fail(p, VVHIP_ERR_INVALID, "plan was created for the classic scheme");
    NEED_FUSABLE(p);
    TRY(step_begin(p));
    TRY(run_application(p, middle_application(p), random_index));
    return step_done(p);
}

int vvhip_step_vv_first(vvhip_plan* p) {                   // API:295-310 (forces for the old positions are in `force`)
    NEED_BOUND(p);
    NEED_FUSABLE(p);
    TRY(step_begin(p));
    return nh_half(p, 0, 0, vv::B_VV_KICK | tail_flags(p) | cons_b(p));
}

int vvhip_step_vv_second(vvhip_plan* p, uint32_t random_index) {   // API:316-336 (forces for the new positions)
    NEED_BOUND(p);
    uint32_t ex = extra_flags(p);
    if (ex) { ex |= vv::A_FE_STORE; p->cur.fextra_dirty = true; }   // the first half of the NEXT step kicks with these (API:316-323)
    else ex = stale_fextra(p);
    NEED_FUSABLE(p);
    TRY(nh_half(p, vv::A_KICK_HALF | ex | cons_a(p), random_index, 0));
    return step_done(p);
}

// ------------------------------------------------------------------------------------------ kernel-interface level
int vvhip_reset_extra_force(vvhip_plan* p) {               // K/middle.cu:227-231
    NEED_BOUND(p);
    if (!stale_fextra(p)) return VVHIP_OK;   // already zero (bind zeroes it; nothing has added to it since the last reset)
    p->cur.fextra_dirty = false;
    ScopedTimer t(p, T_OTHER);
    const size_t nloc = (size_t) (p->hp.shard_end - p->hp.shard_begin);
    HIP_TRY(p, hipMemsetAsync(p->d_fextra.get(), 0, nloc * 3 * sizeof_real(p->hp.precision), p->stream));
    return VVHIP_OK;
}
int vvhip_middle_kick(vvhip_plan* p) { NEED_BOUND(p); return run_a(p, stale_fextra(p) | vv::A_KICK_FULL, 0); }
int vvhip_middle_half_drift1(vvhip_plan* p) { NEED_BOUND(p); return run_a(p, vv::A_POS1, 0); }
int vvhip_middle_half_drift2(vvhip_plan* p) { NEED_BOUND(p); return run_b(p, vv::B_POS2); }
int vvhip_middle_finish(vvhip_plan* p) { NEED_BOUND(p); return run_b(p, vv::B_POS3 | after_positions(p)); }
int vvhip_vv_half_kick(vvhip_plan* p, int update_pos_delta) {
    NEED_BOUND(p);
    return run_a(p, stale_fextra(p) | vv::A_KICK_HALF | (update_pos_delta ? vv::A_POSDELTA_VV : 0), 0);
}
int vvhip_vv_positions(vvhip_plan* p) { NEED_BOUND(p); return run_b(p, vv::B_VV_POS | after_positions(p)); }
int vvhip_scale_velocity(vvhip_plan* p) {                  // HOST:670-754 without the download/upload
    NEED_BOUND(p);
    if (!p->hp.has_nh) return VVHIP_OK;
    // (the reference's kernel: the plain application whatever the cos perturbation -- its host removes and restores the bias around it --, and no exchange between the ranks)
    return run_application(p, compose_application(ThermoMode::PLAIN, 0, 0, false), 0, false);
}
int vvhip_apply_langevin_force(vvhip_plan* p, uint32_t random_index) {
    NEED_BOUND(p);
    if (!p->hp.has_ld) return VVHIP_OK;
    p->cur.fextra_dirty = true;
    return run_a(p, vv::A_FE_LOAD | vv::A_LD | vv::A_FE_STORE, random_index);
}
int vvhip_apply_electric_force(vvhip_plan* p) {
    NEED_BOUND(p);
    if (!p->hp.has_ef) return VVHIP_OK;
    p->cur.fextra_dirty = true;
    return run_a(p, vv::A_FE_LOAD | vv::A_EF | vv::A_FE_STORE, 0);
}
int vvhip_apply_cosine_force(vvhip_plan* p) {
    NEED_BOUND(p);
    p->cur.fextra_dirty = true;
    p->cur.fextra_virtual = false;      // the array holds this step's cos force itself
    return run_a(p, vv::A_FE_LOAD | vv::A_COS | vv::A_FE_STORE, 0);
}
int vvhip_calc_velocity_bias(vvhip_plan* p) {              // HOST:1061-1082
    NEED_BOUND(p);
    TRY(run_a(p, vv::A_BIAS, 0));
    return run_chain(p, vv::C_BIAS);
}
int vvhip_remove_velocity_bias(vvhip_plan* p) { NEED_BOUND(p); return run_b(p, vv::B_BIAS_REMOVE); }
int vvhip_restore_velocity_bias(vvhip_plan* p) { NEED_BOUND(p); return run_b(p, vv::B_BIAS_RESTORE); }
int vvhip_calc_viscosity(vvhip_plan* p, double* v_max, double* inv_vis) {   // HOST:1112-1134, 8-byte download instead of N values
    NEED_BOUND(p);
    double v = 0;
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    HIP_TRY(p, hipMemcpy(&v, &p->d_nh.get()[p->cur.parity].s.v_bias, sizeof(double), hipMemcpyDeviceToHost));
    if (p->hp.precision == VVHIP_SINGLE) v = (double) (float) v;             // vMaxBuffer is `mixed`
    const double vol = p->box[0] * p->box[1] * p->box[2];
    if (v_max) *v_max = v;
    if (inv_vis)
        *inv_vis = v * vol * p->hp.info.inv_mass_total / p->hp.params.cos_acceleration * (2 * 3.1415926 / p->box[2]) *
                   (2 * 3.1415926 / p->box[2]);
    return VVHIP_OK;
}
int vvhip_compute_kinetic_energy(vvhip_plan* p, double* kinetic_energy) {   // HOST:233-235 delegates this to OpenMM; stand-alone hosts get it here
    NEED_BOUND(p);
    if (!kinetic_energy) return VVHIP_ERR_INVALID;
    // uses accumulator 0 of the current copy between two steps (it is zero there) and leaves it zero again
    TRY(run_a(p, vv::A_KE_PLAIN, 0));
    double acc[4];
    TRY(vvhip_debug_read_accumulators(p, acc, 1));
    *kinetic_energy = 0.5 * acc[0];
    return VVHIP_OK;
}

// Algorithmic bytes per particle that kernel A / kernel B of the fused middle step must move (SURVEY section 8d's accounting: particle
// arrays + 6 bytes of index per pass): what bench.py prices the launches with.  Where a kernel takes the arithmetic work-item layout
// it loads no slot words, so no index bytes are counted for it; with the cos perturbation kernel A also reads posq (16 / 32 bytes) and
// the per-lane cos(kz) handed from kernel A to kernel B is counted on both sides (8 + 8 bytes: the step's design moves them).  With
// in-kernel constraints kernel A reads the positions of the cluster MEMBERS (their share of the particles, rounded to whole bytes) and
// both kernels read the cluster word and parameters (4 + 16 bytes per lane) wherever those come from memory, i.e. not in the
// arithmetic layout, where they are pattern rows in LDS.
// Not in these numbers: the removal of the centre-of-mass motion, a pair of kernels of its own in front of every f-th step (vv_dev_cmm.inc).
// Per particle in mixed / double precision: sum = R velm 32 + slot 8 + mass 8 = 48 bytes, subtract = R velm 32 + W velm 32 + slot 8 + mass 8
// = 80 bytes, 128 for the pair (single: velm is 16 bytes, 32 + 48 = 80); divide by f for the share of a step.
int vvhip_algorithmic_bytes(const vvhip_plan* p, int32_t* bytes_a, int32_t* bytes_b) {
    if (!p || !bytes_a || !bytes_b) return VVHIP_ERR_INVALID;
    const int v = p->hp.precision == VVHIP_SINGLE ? 16 : 32;                       // velm: mixed4
    const int x = p->hp.precision == VVHIP_SINGLE ? 16 : 32;                       // posq (+ posqCorrection in mixed mode; double4 in double mode)
    const int xr = p->hp.precision == VVHIP_DOUBLE ? 32 : 16;                      // posq alone
    if (fused_active(p)) {
        // the one-launch step: everything is read once and written once -- R velm, R force, R position, W velm, W position + 6 bytes of
        // index; the cos perturbation and the constrained positions read nothing more (the positions are there), constraint clusters
        // their word and parameters, a virtual site its word.  (The cos(kz) the kernel keeps for vvhip_set_params is a hand-off of this
        // implementation, not counted: the figure stays a lower bound of what the step must move.)
        *bytes_a = 0;
        *bytes_b = v + 24 + x + v + x + 6;
        if (shake_on(p)) *bytes_b += 20;
        if (!p->hp.slot_vsite.empty()) *bytes_b += 8;
        return VVHIP_OK;
    }
    const bool per = p->hp.per.enabled && p->periodic_kernels;
    const bool per_a = per && (p->periodic_a || shake_on(p)), per_b = periodic_b(p);      // as run_a / run_b decide
    const int ia = per_a ? 0 : 6, ib = per_b ? 0 : 6;
    if (use_rekick(p)) { *bytes_a = v + 24 + ia; *bytes_b = v + 24 + x + v + x + ib; }    // A: R velm, R force;  B: R velm, R force, R pos, W velm, W pos
    else { *bytes_a = v + 24 + v + ia; *bytes_b = v + x + v + x + ib; }                   // A: R velm, R force, W velm;  B: R velm, R pos, W velm, W pos
    if (cos_on(p)) { *bytes_a += xr; if (thermo_mode(p) == ThermoMode::COS_MOMENTS) { *bytes_a += 8; *bytes_b += 8; } }
    if (shake_on(p)) {
        long members = 0;
        for (size_t i = 0; i < p->hp.slots.size() / 2; i++)
            if (p->hp.slots[2 * i] >= 0 && ((uint32_t) p->hp.slots[2 * i + 1] & vv::META_SHAKE)) members++;
        const long n = std::max<long>(1, (long) (p->hp.shard_end - p->hp.shard_begin));
        *bytes_a += (int32_t) ((x * members + n / 2) / n);
        if (!per_a) *bytes_a += 20;
        if (!per_b) *bytes_b += 20;
    }
    if (!p->hp.slot_vsite.empty()) *bytes_b += 8;      // the site word of every lane (the 96-byte record of a site lane itself: well below a byte per particle)
    return VVHIP_OK;
}

int vvhip_accumulators(vvhip_plan* p, int phase, void** device_ptr, int32_t* count) {
    NEED_BOUND(p);
    if (!device_ptr || !count) return VVHIP_ERR_INVALID;
    unsigned long long* acc = p->d_acc.get() + p->cur.parity * acc_stride(p);
    if (thermo_mode(p) == ThermoMode::COS_MOMENTS) { *device_ptr = acc; *count = vv::NUM_ACC * vv::ACC_SLOTS; }   // everything kernel A produced
    else if (cos_on(p) && phase == 0) { *device_ptr = acc + 3 * vv::ACC_SLOTS; *count = vv::ACC_SLOTS; }        // bias moment slots only
    else { *device_ptr = acc; *count = 3 * vv::ACC_SLOTS; }                                                   // the three 2KE sums
    return VVHIP_OK;
}

int vvhip_update_image_positions(vvhip_plan* p) {          // HOST:904-934
    NEED_BOUND(p);
    if (!p->hp.has_images) return VVHIP_OK;
    TRY(settle_recovery(p));
    ScopedTimer t(p, T_OTHER);
    HIP_TRY(p, vv::launch_image_pairs(p->hp.precision, p->buf.posq, p->buf.posq_correction, p->d_image_pairs.get(),
                                      (int) p->hp.image_pairs.size() / 2, p->hp.params.mirror_location, p->stream));
    return VVHIP_OK;
}
int vvhip_force_extra(vvhip_plan* p, void** device_ptr) {
    NEED_BOUND(p);
    if (!device_ptr) return VVHIP_ERR_INVALID;
    p->fextra_external = true;
    *device_ptr = p->d_fextra.get();
    return VVHIP_OK;
}

}  // extern "C"
