// vv_launch.cpp -- how the plan launches its kernels: fixed-point scales, launch shape, kernel arguments, the launch wrappers (run_a, run_b,
// run_chain, run_fused) with the timing and tracing around them, and the rules that pick a thermostat application's mode and stage bits.
#include "vv_plan.hpp"

#include <dlfcn.h>
#include <unistd.h>

namespace {
// roctx ranges around every launch group (rocprofv3 --marker-trace): resolved lazily, only if VVHIP_ROCTX=1 or vvhip_set_trace(plan, 1)
struct RoctxApi {
    bool tried = false;
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
};
RoctxApi& roctx_api() {
    static RoctxApi r;
    if (r.tried) return r;
    r.tried = true;
    for (const char* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
        void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (!h) continue;
        r.push = (int (*)(const char*)) dlsym(h, "roctxRangePushA");
        r.pop = (int (*)()) dlsym(h, "roctxRangePop");
        if (r.push && r.pop) break;
        r.push = nullptr; r.pop = nullptr;
    }
    return r;
}
}  // namespace

// 2^k fixed-point scale leaving `headroom` x `bound` below 2^62
static double pick_scale(double bound, double headroom) {
    double top = std::ldexp(1.0, 62) / (std::max(bound, 1.0) * headroom);
    int k = (int) std::floor(std::log2(top));
    k = std::max(0, std::min(k, 40));
    return std::ldexp(1.0, k);
}

void fill_scales(vvhip_plan* p) {
    // One common power-of-two scale for the three 2KE sums, sized on the TOTAL thermostat target with 1024x
    // headroom: a cold group (Drude, 1 K) may transiently be orders of magnitude hotter than its own target
    // without getting anywhere near overflow, and resolution stays ~1e-13 of even the smallest group.
    const vvhip_plan_info& in = p->hp.info;
    const double total = in.nkbt[0] + in.nkbt[1] + in.nkbt[2];
    for (int g = 0; g < 3; g++) {
        p->acc_scale[g] = pick_scale(total, 1024.0);
        p->acc_inv_scale[g] = 1.0 / p->acc_scale[g];
    }
    p->acc_scale[3] = pick_scale(40.0 / in.inv_mass_total, 4.0);  // |sum m vx 2cos| <= 2 M |v|max, |v|max ~ 20 nm/ps
    p->acc_inv_scale[3] = 1.0 / p->acc_scale[3];
    // moments of the cos perturbation (ThermoMode::COS_MOMENTS): Sbb = sum m b^2 <= M (|cos| <= 1, |b| <= 2), |Sab| <= sqrt(Saa Sbb)
    const double mass = 1.0 / in.inv_mass_total;
    for (int g = 0; g < 3; g++) {
        p->acc_scale[4 + g] = pick_scale(std::sqrt(total * 1024.0 * 4.0 * mass), 4.0);
        p->acc_scale[7 + g] = pick_scale(4.0 * mass, 4.0);
        p->acc_inv_scale[4 + g] = 1.0 / p->acc_scale[4 + g];
        p->acc_inv_scale[7 + g] = 1.0 / p->acc_scale[7 + g];
    }
}

// Launch shape.  Measured on MI355X (256 CUs): what matters at the latency-bound sizes is that every CU gets the SAME number of
// blocks -- a CU with one block more than its neighbours finishes ~1.3 us later (its thermostat waves share the fp64 pipe), and the
// kernel ends with its slowest CU.  C3, 1 752 tiles: 876 blocks of 2 tiles (3.4 per CU) 69.4 k steps/s; 251 blocks of 7 tiles (one
// per CU) 74.3 k.  So: k blocks per CU, T tile waves per block (+1 thermostat wave in kernel B, whose 140 VGPRs allow 12 waves
// per CU), chosen to maximise the fill of the last pass; fewer blocks per CU and larger blocks win ties.
// Waves per CU a shape may ask for: kernel B's stage sets without the cos perturbation and without hydrogen-type / general constraint
// clusters are built with 128 VGPRs (four waves per SIMD, 16 per CU), the others with 144-162 (three per SIMD, 12 per CU); kernel A fits
// either.  Round 4 (tools/probes/shape_sweep.py, profiles/r04v_shape_sweep.txt): with 12 everywhere, 2 628 / 2 920 / 3 504 tile waves
// (166-222 k particles) ran in two passes, 66.8 / 65.7 / 64.0 k steps/s; two blocks of 6-7 tile waves per CU hold them in one, 73.3 / 70.9 /
// 67.0 k.
void pick_launch_shape(vvhip_plan* p) {
    // cus = what the bound device reports (256 on an MI355X in SPX mode; 32 per XCD partition in CPX mode); before vvhip_bind the
    // plan assumes a whole MI355X.
    const int nw = p->hp.info.num_waves, cus = p->num_cus;
    // The cos perturbation's one-launch step collects ten rows in its rendezvous, shared by the waves of a block: three tile waves per block
    // (a third of the words to poll, four waves to share the rows) beat one or two up to 3 x CUs tile waves -- one rank's eighth / quarter of C4
    // 89.1 -> 92.8 k / 89.5 -> 91.1 k steps/s; with three rows the plan's choice below stays the best (profiles/r05j_small_shape.txt)
    // (round 6: that rule is gone with the shared-out polling it served -- one tile wave per block again, C4 / 8 9.70 against 9.92 us per step,
    // profiles/r06w_c4_shard_shapes.txt)
    if (nw <= cus) { p->block_threads = 64; p->grid_cap_a = p->grid_cap_b = cus; return; }
    // bandwidth-bound regime (the chain runs as its own launch there, kernel B fits 6 waves per SIMD): tuned at 8.9 M particles
    // (kernel B: two blocks per CU, not four -- round 4, three alternating runs: 2.66 M particles 7 330 -> 7 540 steps/s, 4.4 M 4 226 -> 4 326,
    // 8.9 M 1 970 -> 2 042; kernel A's eight blocks per CU against four: 7 540 / 7 547, 4 326 / 4 272, 2 042 / 2 074)
    // Round 5 (tools/probes/large_n_shape.py, profiles/r05j_large_n_shape.txt, three rotations each on two boxes): kernel A holds 74 VGPRs = six
    // waves per SIMD, so eight blocks of four waves per CU run as one round and a third; four per CU from 5 M particles: 5.5 M 3 350 -> 3 456
    // steps/s, 8.9 M 2 116 -> 2 248 (the other box 2 032 -> 2 060), 3.3 M 6 273 -> 6 253 (eight stay there); three or two per CU lose again.
    if (nw >= p->split_chain_waves) { p->block_threads = 256; p->grid_cap_a = (nw >= 80000 ? 4 : 8) * cus; p->grid_cap_b = 2 * cus; return; }
    const int max_waves = (p->hp.params.cos_acceleration != 0 || p->hp.info.num_shake_clusters > 0 || p->hp.info.num_general_constraints > 0 ||
                           p->hp.info.num_virtual_sites > 0) ? 12 : 16;
    double best = -1;
    int bk = 1, bt = 1;
    for (int k = 1; k <= 4; k++)
        for (int t = 1; t <= 7; t++) {
            if (k * (t + 1) > max_waves) continue;
            const long cap = (long) cus * k * t;
            const long passes = (nw + cap - 1) / cap;
            // fill of the last pass; once several passes are needed, shapes with fewer than 8 tile waves per CU in flight are
            // marked down (they leave memory-level parallelism unused)
            const double fill = (double) nw / (double) (cap * passes) * (passes > 1 ? std::min(1.0, k * t / 8.0) : 1.0);
            if (fill > best + 1e-9 || (fill > best - 1e-9 && (k < bk || (k == bk && t > bt)))) { best = fill; bk = k; bt = t; }
        }
    // Past what two blocks of seven tile waves per CU hold in one pass: that very shape, strided.  The fill rule above prefers shapes whose
    // last pass is fuller, and measured they lose: 5 256 / 7 008 / 10 512 tile waves 51.0 / 39.0 / 27.0 k steps/s against 46.8 / 36.5-37.6 /
    // 26.2-26.6 k for the runners-up; with the 12-wave stage sets as well (7 008 tile waves with HBonds 28.3 k against the rule's 24.7 k, with
    // the cos perturbation 31.6 against 29.3 k; 5 256: 36.7 / 35.8 k and 41.0 / 40.4 k) (profiles/r04zd_mid_sizes.txt).
    if (nw > (long) cus * 14) { bk = 2; bt = 7; }
    // The 12-wave stage sets between 2 048 and 3 072 tile waves: the fill rule ties one block of seven with two of four and takes the former;
    // measured the latter wins (HBonds 2 628 / 2 920 tile waves 54.9 / 53.8 k against 51.3 / 50.4 k steps/s, cos 60.2 / 58.6 against 59.3 / 58.2 k)
    else if (max_waves == 12 && nw > (long) cus * 8 && nw <= (long) cus * 12) { bk = 2; bt = 4; }
    p->block_threads = 64 * bt;
    p->grid_cap_a = p->grid_cap_b = cus * bk;
}

static vv::NHConst make_chain(vvhip_plan* p, uint32_t flags) {
    const vvhip_params& q = p->hp.params;
    const vvhip_plan_info& in = p->hp.info;
    vv::NHConst c{};
    std::memcpy(c.eta_mass, in.eta_mass, sizeof(c.eta_mass));
    for (int g = 0; g < 3; g++)
        for (int i = 0; i < VVHIP_MAX_CHAINS; i++) c.inv_eta_mass[g][i] = in.eta_mass[g][i] > 0 ? 1.0 / in.eta_mass[g][i] : 0.0;
    for (int g = 0; g < 3; g++) {
        c.nkbt[g] = in.nkbt[g];
        c.temperature[g] = g == 2 ? q.drude_temperature : q.temperature;                        // HOST:728
    }
    c.step_size = q.step_size;
    c.inv_mass_total = in.inv_mass_total;
    for (int i = 0; i < vv::NUM_ACC; i++) c.acc_inv_scale[i] = p->acc_inv_scale[i];
    c.num_chains = q.num_nh_chains;
    c.loops_per_step = q.loops_per_step;
    c.num_tg = in.num_temp_groups;
    c.flags = flags;
    return c;
}

vv::KArgs make_args(vvhip_plan* p, uint32_t flags, uint32_t random_index) {
    const vvhip_params& q = p->hp.params;
    vv::KArgs a{};
    a.velm = p->buf.velm;
    a.posq = p->buf.posq;
    a.corr = posq_corr(p);
    a.force = (const long long*) p->buf.force;
    a.fextra = p->d_fextra.get();
    a.pos_delta = p->buf.pos_delta ? p->buf.pos_delta : p->d_pos_delta.get();
    a.old_delta = p->d_old_delta.get();
    a.comv = p->d_comv.get();
    a.comw = p->d_comw.get();
    a.seg_mass = p->d_seg_mass.get();
    a.seg_base = p->d_seg_base.get();
    a.cosz = p->d_cosz.get();
    a.slots = p->d_slots.get();
    a.slot_m = p->d_slot_m.get();
    a.slot_f = p->d_slot_f.get();
    a.slot_image = p->d_slot_image.get();
    a.slot_rand = p->d_slot_rand.get();
    a.slot_shake = p->d_slot_shake.get();
    a.slot_shake_param = p->d_slot_shake_param.get();
    a.slot_vsite = p->d_slot_vsite.get();
    a.vsite_params = p->d_vsite_params.get();
    a.vsite_atom = p->d_vsite_atom.get();
    a.shake_tol = q.constraint_tolerance > 0 ? q.constraint_tolerance : 1e-5;
    a.slot_big = p->d_slot_big.get();
    a.bigacc = p->d_bigacc.get();
    a.big_scale = p->hp.big_scale;
    a.big_inv_scale = 1.0 / p->hp.big_scale;
    a.random = (const float4*) p->buf.random;
    a.acc = p->d_acc.get() + p->cur.parity * acc_stride(p);
    a.acc_next = p->d_acc.get() + (p->cur.parity ^ 1) * acc_stride(p);
    a.nh = p->d_nh.get() + p->cur.parity;
    a.nh_next = p->d_nh.get() + (p->cur.parity ^ 1);
    a.chain = make_chain(p, 0);
    a.lane_const = p->d_lane_const.get();
    a.mb.local = p->mb_local.get();
    a.mb.peers = p->d_mb_peers.get();
    a.mb.ctl = p->d_mb_ctl.get();
    a.mb.ranks = p->mb_ranks;
    a.mb.rank = p->mb_rank;
    a.status = p->d_status;
    a.dbg = p->d_dbg.get();
    a.dbg_block = p->dbg_block;
    a.dbg_span = p->d_dbg_span.get();
    a.dbg_parity = p->dbg_seq >= 0 ? p->dbg_seq++ % 6 : p->dbg_parity;
    a.padded = p->hp.padded_num_atoms;
    a.gc_colors = p->hp.gc_colors;
    a.gc_omega = p->hp.gc_omega;
    {   // posq / posqCorrection as a buffer resource (kernel A's member-only position fetch): 32-bit sizes and offsets
        const unsigned long long bytes = (unsigned long long) (p->hp.shard_end - p->hp.shard_begin) * (p->hp.precision == VVHIP_DOUBLE ? 32ull : 16ull);
        a.pos_bytes = bytes < 0xFFFFFFE0ull ? (uint32_t) bytes : 0u;
    }
    a.nwaves = p->hp.info.num_waves;
    a.acc_rows = p->hp.params.cos_acceleration != 0 ? vv::NUM_ACC : 4;
    a.acc_exclusive = p->acc_store ? 1 : 0;
    a.flags = flags;
    a.random_index = random_index;
    a.per = vv::periodic_args(p->hp.per);
    a.dt = q.step_size;
    // the same IEEE quotients the kernels used to form per lane: (mixed) 1 / (mixed) dt and 1.0 / (mixed) dt
    a.inv_dt_mixed = p->hp.precision == VVHIP_SINGLE ? (double) (1.0f / (float) q.step_size) : 1.0 / q.step_size;
    a.inv_dt_double = p->hp.precision == VVHIP_SINGLE ? 1.0 / (double) (float) q.step_size : 1.0 / q.step_size;
    a.fscale_vv = 0.5 * q.step_size / (double) 0x100000000;                                    // HOST:306
    a.drag = q.friction;                                                                        // HOST:835-839
    a.randf = std::sqrt(2.0 * kBoltz * q.temperature * q.friction / q.step_size);
    a.drag_drude = q.drude_friction;
    a.randf_drude = std::sqrt(2.0 * kBoltz * q.drude_temperature * q.drude_friction / q.step_size);
    a.efscale = q.electric_field * kAvogadro;                                                   // HOST:978
    a.cos_accel = q.cos_acceleration;
    a.inv_box_z = 1.0 / p->box[2];
    a.max_drude = q.max_drude_distance;
    a.hw_scale = std::sqrt(kBoltz * q.drude_temperature);                                       // HOST:190
    a.mirror = q.mirror_location;
    a.inv_mass_total = p->hp.info.inv_mass_total;
    for (int i = 0; i < vv::NUM_ACC; i++) { a.acc_scale[i] = p->acc_scale[i]; a.acc_inv_scale[i] = p->acc_inv_scale[i]; }
    return a;
}

// Chain constants per temperature group for kernel B's thermostat wave; the temperatures are read live (HOST:728), so this is
// refreshed whenever the parameters change.
int upload_lane_const(vvhip_plan* p) {
    if (!p->d_lane_const) return VVHIP_OK;
    const vvhip_params& q = p->hp.params;
    const vvhip_plan_info& in = p->hp.info;
    vv::ChainLaneBlock b[VVHIP_NUM_TG] = {};
    for (int g = 0; g < VVHIP_NUM_TG; g++) {
        for (int i = 0; i < 4; i++) {
            b[g].eta_mass[i] = in.eta_mass[g][i];
            b[g].inv_eta_mass[i] = in.eta_mass[g][i] > 0 ? 1.0 / in.eta_mass[g][i] : 0.0;
        }
        b[g].nkbt = in.nkbt[g];
        b[g].kT = kBoltz * (g == 2 ? q.drude_temperature : q.temperature);
        b[g].acc_inv_scale = p->acc_inv_scale[g];
        b[g].active = (g < in.num_temp_groups && in.eta_mass[g][0] > 0) ? 1.0 : 0.0;
        b[g].dt2 = q.step_size / q.loops_per_step / 2;                            // API:343-345
        b[g].dt4 = b[g].dt2 / 2;
        b[g].dt8 = b[g].dt4 / 2;
    }
    // hosts re-send their parameters every step (the reference re-reads the getters every step): only a real change costs a copy
    if (p->lane_const_valid && std::memcmp(p->lane_const_host, b, sizeof(b)) == 0) return VVHIP_OK;
    (void) hipStreamSynchronize(p->stream);
    hipError_t e = hipMemcpy(p->d_lane_const.get(), b, sizeof(b), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(p, e, "hipMemcpy(chain constants)");
    std::memcpy(p->lane_const_host, b, sizeof(b));
    p->lane_const_valid = true;
    return VVHIP_OK;
}

// ScopedTimer: a roctx range and / or a pair of events around one launch group
static hipEvent_t take_event(vvhip_plan* p) {
    hipEvent_t e = nullptr;
    if (!p->event_pool.empty()) { e = p->event_pool.back(); p->event_pool.pop_back(); }
    else (void) hipEventCreate(&e);
    return e;
}
ScopedTimer::ScopedTimer(vvhip_plan* p_, int cls_, bool dispatch_)
    : p(p_), cls(cls_), on(p_->timing && !p_->capturing && (cls_ != T_OTHER || !p_->timing_kernels_only)), dispatch(dispatch_) {
    if (p->trace && !p->capturing) {
        static const char* names[3] = {"vvhip kernel A (kick / extra forces / sums)", "vvhip kernel B (thermostat / drift / hard wall)", "vvhip other"};
        if (roctx_api().push) { roctx_api().push(names[cls]); ranged = true; }
    }
    if (on) {
        e0 = take_event(p);
        e1 = take_event(p);
        if (!dispatch) (void) hipEventRecord(e0, p->stream);
    }
}
ScopedTimer::~ScopedTimer() {
    if (ranged) roctx_api().pop();
    if (on) {
        if (!dispatch) (void) hipEventRecord(e1, p->stream);
        p->events[cls].emplace_back(e0, e1);
    }
}

static inline void debug_stall(vvhip_plan* p) {
    if (p->stall_us > 0 && !p->capturing && ++p->stall_count % p->stall_period == 0) usleep((useconds_t) p->stall_us);
}
// A launch that found neither a compiled nor a run-time kernel for its stage set and ran the generic one (15-20 % slower): counted per
// plan (vvhip_generic_launches); VVHIP_WARN_GENERIC=1 also prints one line per plan, kernel and stage set.
static void note_generic_launch(vvhip_plan* p, int kernel, uint32_t flags) {
    p->generic_launches[kernel]++;
    // (two stage sets that alternate -- a classic step's halves -- would print on every launch if only the last one were remembered)
    bool seen = false;
    for (uint32_t f : p->generic_seen[kernel]) seen = seen || f == flags;
    if (!seen && p->generic_seen[kernel].size() < 64) p->generic_seen[kernel].push_back(flags);
    p->generic_flags[kernel] = flags;
    static const bool warn = std::getenv("VVHIP_WARN_GENERIC") != nullptr;
    if (warn && !seen) std::fprintf(stderr, "vvhip: kernel %c runs stage set 0x%x on the generic kernel (no compiled specialisation)\n", kernel == 0 ? 'A' : 'B', flags);
}
// Ranks that SHARE a device (test set-ups; found out by vvhip_mailbox_connect) exchange through kernel B's polling thermostat waves: the
// ranks' kernels must be resident together, or the one that got the device first polls until its bounded waits run out while the
// others' launches cannot start (measured round 4, two ranks on one MI355X, 0.44 M / 0.89 M particles: device-filling grids time out
// with either work-item layout, grids of <= half the CUs per rank never do -- tools/probes/mailbox_periodic.sh).  Every rank then
// takes its share of the CUs, one block per CU.  Ranks on devices of their own keep the plan's launch shape.
static int shared_device_cap(const vvhip_plan* p, int cap) {
    if (!(p->mb_on && p->mb_shared_device) || p->launch_shape_forced) return cap;
    return std::max(1, std::min(cap, p->num_cus / std::max(1, p->mb_device_ranks)));
}
// The static mass tables are filled lazily, right in front of the first stage launch that reads them (by then velm.w is what the
// host integrates with); inside a graph capture that would record the fill into every replay, so the capture entry points call this first.
int ensure_mass_table(vvhip_plan* p) {
    if (!(p->mass_tab_a || p->mass_tab_b) || p->mass_tab_valid) return VVHIP_OK;
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "internal: mass tables must be filled before a graph capture starts");
    HIP_TRY(p, vv::launch_mass_table(p->hp.precision, p->buf.velm, p->d_slots.get(), p->hp.info.num_waves, p->d_slot_m.get(), p->d_slot_f.get(), p->stream));
    p->mass_tab_valid = true;
    return VVHIP_OK;
}
int run_a(vvhip_plan* p, uint32_t flags, uint32_t random_index) {
    TRY(settle_recovery(p));
    if (p->mass_tab_a) { flags |= vv::A_MTAB; TRY(ensure_mass_table(p)); }
    // (kernel A takes the arithmetic path where it also saves the 20 bytes per lane of constraint tables; else it does not gain, see periodic_a)
    if (p->hp.per.enabled && p->periodic_kernels && (p->periodic_a || (flags & vv::A_CONS))) flags |= vv::A_PERIODIC;
    if ((flags & vv::A_SHAKE_V) && p->shake_mode == 0) flags |= vv::A_SHAKE_GS;
    debug_stall(p);
    ScopedTimer t(p, T_A, true);
    int route = vv::ROUTE_COMPILED;
    HIP_TRY(p, vv::launch_a(p->hp.precision, make_args(p, flags, random_index), p->block_threads, shared_device_cap(p, p->grid_cap_a), p->stream, t.e0, t.e1, &route));
    if (route == vv::ROUTE_GENERIC) note_generic_launch(p, 0, flags);
    return VVHIP_OK;
}
// Kernel B takes the arithmetic layout whenever the plan has one, also next to the mailbox exchange (round 3 kept them apart after time-outs
// with two ranks on one GPU; round 4 found the cause in device-filling grids of polling waves, whatever the layout: shared_device_cap)
int run_b(vvhip_plan* p, uint32_t flags) {
    TRY(settle_recovery(p));
    if (p->mass_tab_b) { flags |= vv::B_MTAB; TRY(ensure_mass_table(p)); }
    if (periodic_b(p)) flags |= vv::B_PERIODIC;
    if ((flags & vv::B_SHAKE) && p->shake_mode == 0) flags |= vv::B_SHAKE_GS;
    debug_stall(p);
    ScopedTimer t(p, T_B, true);
    int route = vv::ROUTE_COMPILED;
    HIP_TRY(p, vv::launch_b(p->hp.precision, make_args(p, flags, 0), p->block_threads, shared_device_cap(p, p->grid_cap_b), p->stream, t.e0, t.e1, &route));
    if (route == vv::ROUTE_GENERIC) note_generic_launch(p, 1, flags);
    if (flags & vv::B_CHAIN) p->cur.parity ^= 1;     // the advanced thermostat state now lives in the other copy
    return VVHIP_OK;
}
int run_chain(vvhip_plan* p, uint32_t flags) {
    TRY(settle_recovery(p));
    debug_stall(p);
    ScopedTimer t(p, T_OTHER);
    HIP_TRY(p, vv::launch_chain(make_chain(p, flags), p->d_nh.get() + p->cur.parity, p->d_acc.get() + p->cur.parity * acc_stride(p), p->stream));
    return VVHIP_OK;
}

ThermoMode thermo_mode(const vvhip_plan* p) {
    if (!p->hp.has_nh) return ThermoMode::NO_NH;           // API:251: no NH particles, nothing to reduce
    if (!cos_on(p)) return ThermoMode::PLAIN;
    const bool moments = p->hp.num_big == 0 && p->hp.params.num_nh_chains <= 4 && p->hp.info.num_waves < p->split_chain_waves && !p->no_moments;
    return moments ? ThermoMode::COS_MOMENTS : ThermoMode::COS_THREE_LAUNCH;
}
// The mailbox carries the totals between the ranks' kernel-B heads (inline chain): the three kinetic-energy sums, and with the cos
// perturbation in its moment form also the bias moment and the six group moments -- everything kernel A produced, one exchange per
// thermostat application.  The three-launch cos sequence (its bias moment is consumed by another kernel A) and the stand-alone
// chain kernel still go through the collective.
bool use_mailbox(const vvhip_plan* p) {
    return p->mb_on && p->hp.params.num_nh_chains <= 4 && (!cos_on(p) || thermo_mode(p) == ThermoMode::COS_MOMENTS);
}

// The launch(es) that end in the per-group kinetic energies: `flags` = A_KE, the unbias bits in front of it (the three-launch cos
// sequence) and the stage bits that run before the KE on the same launch if possible (kick, extra forces).  Molecules larger than a
// wave need their COM summed across waves first (A_COMPART, its own launch after a memset of the small accumulator), so there the
// stages are split.
int run_ke(vvhip_plan* p, uint32_t flags, uint32_t random_index) {
    if (p->hp.num_big == 0) return run_a(p, flags, random_index);
    const uint32_t ub = flags & (vv::A_UNBIAS_ACC | vv::A_CZ_LOAD), first = flags & ~(vv::A_KE | ub);
    if (first) TRY(run_a(p, first, random_index));
    HIP_TRY(p, hipMemsetAsync(p->d_bigacc.get(), 0, (size_t) p->hp.num_big * 4 * sizeof(unsigned long long), p->stream));
    TRY(run_a(p, vv::A_COMPART | ub, 0));
    return run_a(p, vv::A_KE | ub, 0);
}

// Scaling kernel with the chain in its head (chain length <= 4), or the stand-alone chain launch in front of it.
// chain_in_b: the bits kernel B takes when the chain runs in its head, 0 when it runs as its own launch.
uint32_t chain_in_b(const vvhip_plan* p) {
    // Large systems: the chain registers cost kernel B half its occupancy (140 vs 74 VGPRs), which matters once the kernel is
    // bandwidth bound; there the chain runs as its own one-wave launch and B only reads the scale factors.
    const bool split = p->hp.info.num_waves >= p->split_chain_waves && !use_mailbox(p);
    if (p->hp.params.num_nh_chains > 4 || split) return 0;
    return vv::B_CHAIN | (use_mailbox(p) ? vv::B_MAILBOX : 0u);
}
int run_chain_and_b(vvhip_plan* p, uint32_t bflags, bool with_bias) {
    const uint32_t chain = chain_in_b(p);
    if (!chain) TRY(run_chain(p, vv::C_CHAIN | (with_bias ? vv::C_BIAS : 0)));
    return run_b(p, chain | bflags);
}

// ---- the one-launch step (vv_device.inc: "fused step")
// Shape: the plan's own (pick_launch_shape) when it gives every tile a wave of its own on at most ACC_SLOTS blocks, one block per CU.
bool fused_shape_ok(const vvhip_plan* p) {
    const int tiles = p->block_threads / 64, nw = p->hp.info.num_waves;
    if (tiles < 1 || tiles > 7) return false;
    const int blocks = (nw + tiles - 1) / tiles;
    return blocks >= 1 && blocks <= vv::ACC_SLOTS && blocks <= std::min(p->grid_cap_b, p->grid_cap_a) && blocks <= p->num_cus;
}
// What the plan's state allows, before any kernel is looked up.  The two halves must not need anything between them: no RCCL exchange
// (sharded runs with a communicator), no stand-alone chain launch (long chains, very large systems), no partial sums of molecules larger
// than a wave, no three-launch cos sequence; ranks that share this device (test set-ups) keep the two-launch step, whose kernels need
// not be resident together.
bool fused_state_ok(const vvhip_plan* p) {
    const vv::HostPlan& hp = p->hp;
    if (!p->fused || !hp.has_nh || hp.params.num_nh_chains > 4 || hp.num_big != 0) return false;
    if (hp.info.num_waves >= p->split_chain_waves) return false;
    // sharded runs: the xGMI mailbox exchanges the ranks' totals inside the thermostat wave, right behind the local rendezvous (one wait after
    // the other, no launch in between); an RCCL all-reduce needs the kernel boundary, and ranks that share this device cannot all be resident
    if ((p->comm && !use_mailbox(p)) || (p->mb_on && (!use_mailbox(p) || p->mb_shared_device))) return false;
    if (hp.params.cos_acceleration != 0 && (p->no_moments || hp.params.num_nh_chains > 4)) return false;
    if (p->mass_tab_a || !p->mass_tab_b || p->shake_mode == 0) return false;      // (comparison builds of the two-launch kernels)
    if (hp.per.enabled && p->periodic_kernels) return false;                      // the arithmetic layout belongs to the many-pass regime
    return fused_shape_ok(p);
}
void forget_fused_checks(vvhip_plan* p) {      // what the lookups found no longer holds (who shares the device, the "fused" hook)
    for (vvhip_plan::FusedCheck& c : p->fused_checks) c.b = 0;
    p->fused_last = -1;
}
int run_fused(vvhip_plan* p, uint32_t aflags, uint32_t bflags, uint32_t random_index, bool* taken) {
    *taken = false;
    if (!fused_state_ok(p)) return VVHIP_OK;
    bflags |= vv::B_CHAIN | vv::B_MTAB | (use_mailbox(p) ? vv::B_MAILBOX : 0u);
    // kernel and occupancy of this pair of stage sets on this launch shape: looked up once (an entry with b = 0 is empty: bflags never is)
    p->fused_last = -1;
    for (int i = 0; i < 4 && p->fused_last < 0; i++) {
        const vvhip_plan::FusedCheck& c = p->fused_checks[i];
        if (c.a == aflags && c.b == bflags && c.threads == p->block_threads && c.waves == p->hp.info.num_waves) p->fused_last = i;
    }
    if (p->fused_last < 0) {
        p->fused_last = p->fused_check_next++ & 3;
        vv::KArgs q = make_args(p, bflags, random_index);
        q.flags_a = aflags;
        int per_cu = 0;
        const hipError_t e = vv::launch_fused(p->hp.precision, q, p->block_threads, p->d_rv.get(), p->stream, nullptr, nullptr, nullptr, &per_cu);      // (asks only; launches nothing)
        const int tiles = p->block_threads / 64, blocks = (p->hp.info.num_waves + tiles - 1) / tiles;
        if (e != hipSuccess) (void) hipGetLastError();
        p->fused_checks[p->fused_last] = {aflags, bflags, p->block_threads, p->hp.info.num_waves, e == hipSuccess && per_cu >= 1 && (long) per_cu * p->num_cus >= blocks};
    }
    if (!p->fused_checks[p->fused_last].ok) return VVHIP_OK;
    TRY(settle_recovery(p));
    if (!p->fused) return VVHIP_OK;      // (settling may have pinned the plan to two launches)
    TRY(ensure_mass_table(p));
    debug_stall(p);
    ScopedTimer t(p, T_B, true);
    int route = vv::ROUTE_COMPILED;
    vv::KArgs q = make_args(p, bflags, random_index);
    q.flags_a = aflags;
    q.fused_poll_delay = p->fused_poll_delay;
    // the "a block polled twice" words of this step and of the one before (by thermostat parity), behind the two copies of the rendezvous words
    q.rv_late_cur = rv_late_row(p->d_rv.get(), p->cur.parity);
    q.rv_late_prev = rv_late_row(p->d_rv.get(), p->cur.parity ^ 1);
    q.fused_late_shift = p->fused_late_shift;
    HIP_TRY(p, vv::launch_fused(p->hp.precision, q, p->block_threads, rv_words(p->d_rv.get(), p->cur.parity), p->stream, t.e0, t.e1, &route, nullptr));
    p->cur.parity ^= 1;            // the advanced thermostat state now lives in the other copy
    p->fused_launches++;
    *taken = true;
    return VVHIP_OK;
}

uint32_t extra_flags(const vvhip_plan* p) {
    uint32_t f = 0;
    if (p->hp.has_ld) f |= vv::A_LD;
    if (p->hp.has_ef) f |= vv::A_EF;
    if (p->hp.params.cos_acceleration != 0) f |= vv::A_COS;
    return f;
}
// What follows a position update on the split path: the hard wall, and the sites described to the plan (they follow EVERY position
// update, HOST:203-214) ...
uint32_t after_positions(const vvhip_plan* p) {
    uint32_t f = 0;
    if (p->hp.params.max_drude_distance > 0 && p->hp.has_pairs) f |= vv::B_HARDWALL;
    if (!p->hp.slot_vsite.empty()) f |= vv::B_VSITE;
    return f;
}
// ... and in a whole step the image particles as well (HOST:203-212, API:266-268)
uint32_t tail_flags(const vvhip_plan* p) { return after_positions(p) | (p->hp.has_images ? vv::B_IMAGE : 0u); }

// Does vvhip_step_middle take the one-launch step for this plan as it stands?  (The kernel itself is looked up at the first step; a pair
// of stage sets already found wanting says so here.)
bool fused_active(const vvhip_plan* p) {
    if (!p->bound || !p->hp.params.use_middle_scheme || !p->hp.info.constraints_fused || !fused_state_ok(p) || thermo_mode(p) == ThermoMode::COS_THREE_LAUNCH) return false;
    return p->fused_last < 0 || p->fused_checks[p->fused_last].ok;
}

extern "C" {

int vvhip_set_trace(vvhip_plan* p, int enable) {
    if (!p) return VVHIP_ERR_INVALID;
    p->trace = enable != 0;
    return VVHIP_OK;
}
int vvhip_generic_launches(vvhip_plan* p, int64_t counts[2], uint32_t stage_sets[2]) {
    if (!p || !counts) return VVHIP_ERR_INVALID;
    for (int k = 0; k < 2; k++) { counts[k] = p->generic_launches[k]; if (stage_sets) stage_sets[k] = p->generic_flags[k]; }
    return VVHIP_OK;
}
int vvhip_rtc_mode(int mode) { return vv::set_rtc_mode(mode); }
int vvhip_rtc_stats(int64_t counts[3], double* compile_seconds) {
    if (!counts) return VVHIP_ERR_INVALID;
    counts[0] = (int64_t) vv::vv_rtc_compiled.load(); counts[1] = (int64_t) vv::vv_rtc_launches[0].load(); counts[2] = (int64_t) vv::vv_rtc_launches[1].load();
    if (compile_seconds) *compile_seconds = vv::vv_rtc_compile_seconds;
    return VVHIP_OK;
}
int vvhip_rtc_failures(int64_t* failed) {
    if (!failed) return VVHIP_ERR_INVALID;
    *failed = (int64_t) vv::vv_rtc_failed.load();
    return VVHIP_OK;
}
int vvhip_timing_enable(vvhip_plan* p, int enable) {
    if (!p) return VVHIP_ERR_INVALID;
    p->timing = enable != 0;
    p->timing_kernels_only = enable == 2;
    if (enable > 2) {                  // enable = n > 2: as 2, with n events prepared now (a timed run of n / 2 launches creates none)
        p->timing_kernels_only = true;
        for (int i = (int) p->event_pool.size(); i < enable; i++) { hipEvent_t e = nullptr; if (hipEventCreate(&e) == hipSuccess) p->event_pool.push_back(e); }
    }
    return VVHIP_OK;
}
int vvhip_timing_read(vvhip_plan* p, double* ms_a, double* ms_b, double* ms_other, int32_t* launches) {
    NEED_BOUND(p);
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    double tot[3] = {0, 0, 0};
    int32_t n[3] = {0, 0, 0};
    for (int c = 0; c < 3; c++) {
        for (auto& e : p->events[c]) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) { tot[c] += ms; n[c]++; }
            p->event_pool.push_back(e.first);
            p->event_pool.push_back(e.second);
        }
        p->events[c].clear();
    }
    if (ms_a) *ms_a = tot[0];
    if (ms_b) *ms_b = tot[1];
    if (ms_other) *ms_other = tot[2];
    if (launches) { launches[0] = n[0]; launches[1] = n[1]; launches[2] = n[2]; }
    return VVHIP_OK;
}

}  // extern "C"
