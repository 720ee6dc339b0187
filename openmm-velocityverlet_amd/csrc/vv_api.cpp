// vv_api.cpp -- the C ABI of include/vvhip.h on top of vv_host (analysis) and vv_kernels (HIP): a plan's life cycle, its status words and the
// caller-owned device memory and streams.  The other translation units of the ABI: see the map in vv_plan.hpp.
#include "vv_plan.hpp"

void drop_graphs(vvhip_plan* p) {
    for (auto& row : p->graph)
        for (auto& g : row)
            if (g.exec) { (void) hipGraphExecDestroy(g.exec); g.exec = nullptr; }
}

int fail(vvhip_plan* p, int code, const std::string& msg) {
    if (p) p->err = msg;
    return code;
}
int hip_fail(vvhip_plan* p, hipError_t e, const char* what) {
    return fail(p, e == hipErrorNoDevice || e == hipErrorInvalidDevice ? VVHIP_ERR_NO_DEVICE : VVHIP_ERR_HIP,
                std::string(what) + ": " + hipGetErrorString(e));
}
// Work on the plan from OUTSIDE the plan-driven loops while their snapshot is still unverified (a split entry point, a parameter change, a
// fill): the calls since the snapshot are settled first -- synchronised and, if their rendezvous failed, repeated -- because what comes
// now is not in the list a recovery would repeat.
int settle_recovery(vvhip_plan* p) {
    if (!p->rec.valid || p->rec.in_loop || p->rec.replaying || p->capturing) return VVHIP_OK;
    return vvhip_synchronize(p);
}
// Sticky failures the kernels reported through the pinned status word (no synchronisation: the word lives in host memory).
int check_exchange_health(vvhip_plan* p) {
    if (!p->h_status) return VVHIP_OK;
    const unsigned int mb = __atomic_load_n(&p->h_status[0], __ATOMIC_RELAXED), ov = __atomic_load_n(&p->h_status[1], __ATOMIC_RELAXED);
    const unsigned int rv = __atomic_load_n(&p->h_status[2], __ATOMIC_RELAXED), cs = __atomic_load_n(&p->h_status[3], __ATOMIC_RELAXED);
    if (mb) return fail(p, VVHIP_ERR_EXCHANGE, "multi-GPU mailbox: a wait on the peers' thermostat totals timed out; this rank went on with incomplete sums, the run is void");
    // (a missed rendezvous first: an overflowed accumulator or an unconverged cluster next to it is what steps on incomplete sums produce)
    if (rv) {
        // (the plan is pinned to two launches per step from here on whatever else happens: the next run does not meet the same fate)
        if (p->fused) {
            p->fused = false;
            if (p->bound) (void) hipStreamSynchronize(p->stream);      // (the word is read without synchronising: replays of the graphs about to go may still be in flight)
            drop_graphs(p);
        }
        return fail(p, VVHIP_ERR_RENDEZVOUS, "fused step: the blocks of the one-launch step did not meet within 0.2 s (not resident together: another process's kernels on the device?); the thermostat went on with incomplete sums and the state since the last good synchronisation is void.  The plan now takes two launches per step (vvhip_fused_status: active = 0); vvhip_status_clear + restoring the state continues the run.  Runs of >= 64 steps through vvhip_run_graph / vvhip_run_eager recover by themselves (vvhip_debug_tune \"recover\")");
    }
    // (an unconverged constraint cluster is reported before the overflow it usually causes a step or two later)
    if (cs) return fail(p, VVHIP_ERR_CONSTRAINT, "in-kernel constraints: a cluster reached the iteration cap without converging (a degenerate geometry, or a step that is too large); positions / velocities of that cluster are not within tolerance");
    if (ov) return fail(p, VVHIP_ERR_OVERFLOW, "a fixed-point accumulator overflowed (kinetic energy beyond 1024 x the thermostat target): the thermostat input is invalid");
    return VVHIP_OK;
}

extern "C" {

// ------------------------------------------------------------------------------------------ life cycle
int vvhip_plan_create(const vvhip_system_desc* system, const vvhip_params* params, int precision, vvhip_plan** plan_out,
                      char* errbuf, size_t errbuf_len) {
    auto report = [&](int code, const std::string& msg) {
        if (errbuf && errbuf_len) std::snprintf(errbuf, errbuf_len, "%s", msg.c_str());
        return code;
    };
    if (!system || !params || !plan_out) return report(VVHIP_ERR_INVALID, "null argument");
    try {
        vvhip_plan* p = new vvhip_plan();
        p->hp = vv::analyze(*system, *params, precision);
        fill_scales(p);
        if (const char* e = std::getenv("VVHIP_STALL")) {
            p->stall_us = std::atol(e);
            if (const char* c = std::strchr(e, ':')) p->stall_period = std::max(1L, std::atol(c + 1));
        }
        if (const char* e = std::getenv("VVHIP_SHAKE_MODE")) p->shake_mode = std::atoi(e) != 0 ? 1 : 0;
        if (const char* e = std::getenv("VVHIP_FUSED")) p->fused = std::atoi(e) != 0;
        if (const char* e = std::getenv("VVHIP_RECOVER")) p->rec.enabled = std::atoi(e) != 0;
        p->mass_tab_a = vv::sf_kernels_use_mass_table(0);
        p->mass_tab_b = vv::sf_kernels_use_mass_table(1);
        if (const char* e = std::getenv("VVHIP_ROCTX")) p->trace = std::atoi(e) != 0;
        pick_launch_shape(p);
        *plan_out = p;
        return VVHIP_OK;
    } catch (const vv::Error& e) {
        return report(e.code, e.what());
    } catch (const std::exception& e) {
        return report(VVHIP_ERR_INVALID, e.what());
    }
}

// Test / tuning hook (include/vvhip.h): the choices the measurements of TUNING_LOG.md settled, adjustable per plan so that tests can force
// code paths at sizes they can afford (the large-system launch shape on 10 000 particles, loaded instead of computed slot words, ...).
// The environment switches of rounds 1-3 (VVHIP_REKICK, VVHIP_CAP_A, ...) are gone: their experiments are closed.
int vvhip_debug_tune(vvhip_plan* p, const char* key, int value) {
    if (!p || !key) return VVHIP_ERR_INVALID;
    if (p->bound) TRY(settle_recovery(p));
    if (p->bound) HIP_TRY(p, hipStreamSynchronize(p->stream));
    const std::string k = key;
    if (k == "periodic_kernels") p->periodic_kernels = value != 0;          // 0: keep the arithmetic layout's slot order but load the slot words
    else if (k == "periodic_a") p->periodic_a = value != 0;                 // kernel A alone
    else if (k == "periodic_b") p->periodic_b = value != 0;                 // kernel B alone
    else if (k == "gc_omega_permille") p->hp.gc_omega = value / 1000.0;     // relaxation factor of the general clusters' sweeps (rate scans)
    else if (k == "rekick") p->rekick = value != 0;                         // 0: kernel A stores the kicked velocities, kernel B does not repeat the kick
    else if (k == "no_moments") p->no_moments = value != 0;                 // 1: cos perturbation as three launches (bias, sums, scale)
    else if (k == "fused") { p->fused = value != 0; forget_fused_checks(p); }
    else if (k == "recover") { p->rec.enabled = value != 0; p->rec.valid = false; p->rec.runs.clear(); }      // 0: a missed rendezvous stays fatal (VVHIP_ERR_RENDEZVOUS)
    else if (k == "recover_min_steps") p->rec.min_steps = std::max(1, value);
    else if (k == "fused_late_shift") p->fused_late_shift = std::max(0, std::min(value, 16));
    else if (k == "fused_poll_delay") p->fused_poll_delay = std::max(-1, std::min(value, 64));   // 0: the middle scheme's step as two launches (A, B) also where one would do
    else if (k == "mass_tab_a") p->mass_tab_a = value != 0;
    else if (k == "mass_tab_b") p->mass_tab_b = value != 0;
    else if (k == "acc_store") p->acc_store = value != 0;                   // 0: atomics also where a block owns its accumulator slot
    else if (k == "split_chain_waves") { p->split_chain_waves = value; if (!p->launch_shape_forced) pick_launch_shape(p); }
    else if (k == "block_threads") {
        if (value < 64 || value > 448 || value % 64) return fail(p, VVHIP_ERR_INVALID, "block_threads: a multiple of 64 in [64, 448]");
        p->block_threads = value; p->grid_cap_a = 2048; p->grid_cap_b = 1024; p->launch_shape_forced = true;
    }
    else if (k == "grid_cap_a") { if (value < 1) return VVHIP_ERR_INVALID; p->grid_cap_a = value; p->launch_shape_forced = true; }
    else if (k == "grid_cap_b") { if (value < 1) return VVHIP_ERR_INVALID; p->grid_cap_b = value; p->launch_shape_forced = true; }
    else if (k == "profile_grid_cap") { if (value < 1) return VVHIP_ERR_INVALID; p->profile_grid_cap = value; }      // (no launch shape of the step: nothing forced)
    else if (k == "msd_block_threads") { if (value != 0 && (value < 64 || value > 512 || value % 64)) return VVHIP_ERR_INVALID; p->msd_block_threads = value; }
    else if (k == "msd_wave_reduce") { if (value < 0 || value > 1) return VVHIP_ERR_INVALID; p->msd_wave_reduce = value; }
    else if (k == "current_two_level") { if (value < 0 || value > 1) return VVHIP_ERR_INVALID; p->current_two_level = value; }
    else if (k == "current_block_threads") { if (value != 0 && (value < 64 || value > 512 || value % 64)) return VVHIP_ERR_INVALID; p->current_block_threads = value; }
    else if (k == "modes_sites_per_thread") { if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8) return VVHIP_ERR_INVALID; p->modes_sites_per_thread = value; }      // (the three are read when a recorder starts: the work list is built there)
    else if (k == "modes_k_tile") { if (value < 0 || value > vv::MODES_MAX_K_TILE) return VVHIP_ERR_INVALID; p->modes_k_tile = value; }
    else if (k == "modes_block_threads") { if (value != 0 && (value < 64 || value > 512 || value % 64)) return VVHIP_ERR_INVALID; p->modes_block_threads = value; }
    else if (k == "contacts_rows_per_tile") { if (value < 64 || value > vv::CONTACTS_MAX_ROWS_PER_TILE || value % 64) return VVHIP_ERR_INVALID; p->contacts_rows_per_tile = value; }      // (the two are read when a recorder starts: the work list is built there)
    else if (k == "contacts_words_per_item") { if (value < 1 || value > 64) return VVHIP_ERR_INVALID; p->contacts_words_per_item = value; }
    else if (k == "contacts_skip_zero") { if (value < 0 || value > 1) return VVHIP_ERR_INVALID; p->contacts_skip_zero = value; }
    else if (k == "acf_block_threads") { if (value != 0 && (value < 64 || value > 512 || value % 64)) return VVHIP_ERR_INVALID; p->acf_block_threads = value; }
    else if (k == "acf_wave_reduce") { if (value < 0 || value > 1) return VVHIP_ERR_INVALID; p->acf_wave_reduce = value; }
    else if (k == "acf_slots_in_flight") { if (value < 1 || value > vv::ACF_MAX_SLOTS_IN_FLIGHT) return VVHIP_ERR_INVALID; p->acf_slots_in_flight = value; }
    else if (k == "vanhove_block_threads") { if (value != 0 && (value < 64 || value > 512 || value % 64)) return VVHIP_ERR_INVALID; p->vanhove_block_threads = value; }
    else if (k == "vanhove_lds") { if (value < 0 || value > 1) return VVHIP_ERR_INVALID; p->vanhove_lds = value; }
    else if (k == "vanhove_wave_reduce") { if (value < 0 || value > 1) return VVHIP_ERR_INVALID; p->vanhove_wave_reduce = value; }
    else if (k == "vhd_hist_copies") { if (value != 1 && value != 4) return VVHIP_ERR_INVALID; p->vhd_hist_copies = value; }
    else if (k == "vhd_items_target") { if (value < 1) return VVHIP_ERR_INVALID; p->vhd_items_target = value; }      // (read when a recorder starts: the work list is built there)
    else if (k == "vhd_lds") { if (value < 0 || value > 1) return VVHIP_ERR_INVALID; p->vhd_lds = value; }
    else if (k == "sdf_items_target") { if (value < 1) return VVHIP_ERR_INVALID; p->sdf_items_target = value; }      // (read when a recorder starts: the work list is built there)
    else if (k == "rdf_hist_copies") { if (value != 1 && value != 4) return VVHIP_ERR_INVALID; p->rdf_hist_copies = value; }
    else if (k == "rdf_items_target") { if (value < 1) return VVHIP_ERR_INVALID; p->rdf_items_target = value; }      // (read when a recorder starts: the work list is built there)
    else return fail(p, VVHIP_ERR_INVALID, "vvhip_debug_tune: unknown key " + k);
    if (k == "mass_tab_a" || k == "mass_tab_b") p->mass_tab_valid = false;
    drop_graphs(p);
    return VVHIP_OK;
}

void vvhip_plan_destroy(vvhip_plan* p) {
    if (!p) return;
    if (p->d_slots) (void) hipStreamSynchronize(p->stream);      // (the first thing vvhip_bind allocates: also a bind that failed half-way may have fills in flight)
    drop_graphs(p);
    if (p->comm) (void) rccl_api().commDestroy(p->comm);
    mailbox_release(p);
    for (auto& v : p->events)
        for (auto& e : v) { (void) hipEventDestroy(e.first); (void) hipEventDestroy(e.second); }
    for (hipEvent_t e : p->event_pool) (void) hipEventDestroy(e);
    delete p;      // the plan's buffers go with their owners (vv_devmem.hpp)
}

const char* vvhip_last_error(const vvhip_plan* p) { return p ? p->err.c_str() : "null plan"; }

int vvhip_plan_get_info(const vvhip_plan* p, vvhip_plan_info* info) {
    if (!p || !info) return VVHIP_ERR_INVALID;
    *info = p->hp.info;
    return VVHIP_OK;
}

const char* vvhip_plan_unfused_reason(const vvhip_plan* p) { return p ? p->hp.unfused_reason.c_str() : "null plan"; }

int vvhip_plan_get_slots(const vvhip_plan* p, int32_t* slots, int32_t capacity) {
    if (!p) return VVHIP_ERR_INVALID;
    const int32_t n = p->hp.info.num_waves * 64;
    if (slots) {
        if (capacity < n) return VVHIP_ERR_INVALID;
        std::memcpy(slots, p->hp.slots.data(), (size_t) n * 2 * sizeof(int32_t));
    }
    return n;
}

int vvhip_bind(vvhip_plan* p, const vvhip_buffers* b) {
    if (!p || !b) return VVHIP_ERR_INVALID;
    if (!b->velm || !b->posq || !b->force) return fail(p, VVHIP_ERR_INVALID, "velm, posq and force must be device pointers");
    if (p->hp.precision == VVHIP_MIXED && !b->posq_correction)
        return fail(p, VVHIP_ERR_INVALID, "mixed precision needs posq_correction (the reference's image kernel dereferences it too: quirk Q5)");
    if (p->hp.has_ld && (!b->random || b->random_size == 0))
        return fail(p, VVHIP_ERR_INVALID, "Langevin particles present but no random buffer bound");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(p, VVHIP_ERR_NO_DEVICE, "no HIP device: libvvhip has no CPU path");
    if (p->bound) TRY(settle_recovery(p));
    p->baro.pending = false;       // (the backup of a barostat scale belongs to the arrays bound when it was taken)
    if (p->bound) {
        // The captured graphs bake EVERY caller-owned pointer (make_args): a re-bind that swaps any of them must drop both
        // executables, or vvhip_run_graph would replay kernels on the old arrays without a word.  The stream is not part of a
        // captured node.  Only another velm array invalidates the mass tables (its inverse masses are re-read).
        const vvhip_buffers& o = p->buf;
        const bool same = b->velm == o.velm && b->posq == o.posq && b->posq_correction == o.posq_correction && b->force == o.force &&
                          b->pos_delta == o.pos_delta && b->random == o.random && b->random_size == o.random_size;
        if (b->velm != o.velm) p->mass_tab_valid = false;
        const Riders rd = riders(p);      // (a series row, a scheduled removal, a frame and a profile sample read velm through their captured arguments too; an MSD, RDF, density-mode or contact sample posq, a current sample all three, an autocorrelation sample velm or posq, a self or distinct van Hove or a spatial distribution sample posq)
        if (!same || std::any_of(rd.begin(), rd.end(), [](const Rider& r) { return r.on; })) drop_graphs(p);
    }
    // a re-bind that moves the plan to another stream: whatever the plan still has in flight on the old one (fills, steps) must be
    // complete before work enqueued on the new one can touch the same buffers
    if (p->bound && p->stream != (hipStream_t) b->stream) HIP_TRY(p, hipStreamSynchronize(p->stream));
    p->buf = *b;
    p->stream = (hipStream_t) b->stream;
    if (p->bound) return VVHIP_OK;      // re-binding only swaps the caller-owned pointers
    const vv::HostPlan& hp = p->hp;
    const size_t nloc = (size_t) (hp.shard_end - hp.shard_begin);
    const size_t nslots = (size_t) hp.info.num_waves * 64;
    const size_t rs = sizeof_real(hp.precision), ms = sizeof_mixed(hp.precision);
    HIP_TRY(p, vv::upload(p->d_slots, hp.slots));
    if (!hp.slot_image.empty()) {
        HIP_TRY(p, vv::upload(p->d_slot_image, hp.slot_image));
        if (!hp.image_pairs.empty()) HIP_TRY(p, vv::upload(p->d_image_pairs, hp.image_pairs));
    }
    if (!hp.slot_rand.empty()) HIP_TRY(p, vv::upload(p->d_slot_rand, hp.slot_rand));
    if (!hp.slot_shake.empty()) {
        HIP_TRY(p, vv::upload(p->d_slot_shake, hp.slot_shake));
        HIP_TRY(p, vv::upload(p->d_slot_shake_param, hp.slot_shake_param));
    }
    if (!hp.slot_vsite.empty()) {
        HIP_TRY(p, vv::upload(p->d_slot_vsite, hp.slot_vsite));
        HIP_TRY(p, vv::upload(p->d_vsite_params, hp.vsite_params));
        HIP_TRY(p, vv::upload(p->d_vsite_atom, hp.vsite_atom));
    }
    if (!hp.slot_big.empty()) {
        HIP_TRY(p, vv::upload(p->d_slot_big, hp.slot_big));
        HIP_TRY(p, vv::zeros(p->d_bigacc, (size_t) hp.num_big * 4 * sizeof(unsigned long long), p->stream));
    }
    // (the fills go into the PLAN's stream, not the null stream: see vv::zeros)
    HIP_TRY(p, vv::zeros(p->d_fextra, nloc * 3 * rs, p->stream));            // zero-initialised like HOST:79-89
    HIP_TRY(p, vv::zeros(p->d_old_delta, nloc * 4 * ms, p->stream));
    HIP_TRY(p, vv::zeros(p->d_cosz, nslots * sizeof(double), p->stream));
    const size_t nseg = std::max<size_t>(hp.seg_mass.size() / 2, 1);
    HIP_TRY(p, vv::zeros(p->d_comv, nseg * 4 * ms, p->stream));
    HIP_TRY(p, vv::upload(p->d_seg_base, hp.seg_base));
    HIP_TRY(p, vv::upload(p->d_seg_mass, hp.seg_mass));
    HIP_TRY(p, p->d_slot_m.alloc(nslots * sizeof(double)));      // (the mass tables are filled on the device: ensure_mass_table)
    HIP_TRY(p, p->d_slot_f.alloc(nslots * sizeof(double)));
    HIP_TRY(p, vv::zeros(p->d_comw, nseg * sizeof(double), p->stream));
    HIP_TRY(p, vv::zeros(p->d_pos_delta, nloc * 4 * ms, p->stream));
    HIP_TRY(p, vv::zeros(p->d_epoch, sizeof(unsigned long long), p->stream));
    HIP_TRY(p, vv::zeros(p->d_acc, 2 * kAccN * sizeof(unsigned long long), p->stream));
    // rendezvous words of the fused step: uncached (every block's thermostat wave polls what the other blocks -- on other XCDs, behind other
    // L2s -- have just stored); zero = "no step's word" (tags run from 1)
    // (the layout: vv_plan.hpp, kRvWords)
    HIP_TRY(p, vv::zeros(p->d_rv, (size_t) kRvWords * sizeof(unsigned long long), p->stream, true));
    std::vector<vv::NHDevState> init(2);
    for (int c = 0; c < 2; c++)
        for (int g = 0; g < 3; g++) { init[c].s.vscale[g] = 1.0; init[c].scales[g] = 1.0; }
    for (int c = 0; c < 2; c++) init[c].rv_delay = 6;      // where the wait of the fused step's rendezvous starts (it tunes itself from there)
    HIP_TRY(p, vv::upload(p->d_nh, init));
    HIP_TRY(p, p->d_lane_const.alloc(VVHIP_NUM_TG * sizeof(vv::ChainLaneBlock)));
    // Drude temperature report: tables (16 bytes at least: an empty table is still a pointer the kernels take) and scratch of its own
    HIP_TRY(p, vv::upload(p->d_rep_lane_mol, hp.report_lane_mol, 16));
    HIP_TRY(p, vv::upload(p->d_rep_lane_mass, hp.report_lane_mass, 16));
    HIP_TRY(p, vv::upload(p->d_rep_lane_mu, hp.report_lane_mu, 16));
    HIP_TRY(p, vv::upload(p->d_rep_mol_mass, hp.report_mol_mass, 16));
    HIP_TRY(p, vv::upload(p->d_rep_cross, hp.report_cross, 16));
    HIP_TRY(p, vv::upload(p->d_rep_cross_mu, hp.report_cross_mu, 16));
    HIP_TRY(p, p->d_rep.alloc((8 + 6 * hp.report_mol_mass.size()) * sizeof(long long)));
    HIP_TRY(p, p->h_rep.alloc(8 * sizeof(long long)));
    HIP_TRY(p, p->h_status.alloc(4 * sizeof(unsigned int), true));
    std::memset(p->h_status.get(), 0, 4 * sizeof(unsigned int));
    HIP_TRY(p, hipHostGetDevicePointer((void**) &p->d_status, p->h_status.get(), 0));
    {   // launch shape for the device this plan is bound to (one block per CU balancing needs the real CU count)
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 &&
            prop.multiProcessorCount != p->num_cus) {
            p->num_cus = prop.multiProcessorCount;
            if (!p->launch_shape_forced) pick_launch_shape(p);
        }
    }
    p->bound = true;
    TRY(upload_lane_const(p));
    // The fills above are ordered in the plan's stream only.  A host may take vvhip_force_extra() / the plan's pos_delta pointer
    // right after this call and write through a blocking copy or another stream: bind is not on the hot path, so it returns
    // with every fill complete.
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    return VVHIP_OK;
}

int vvhip_set_params(vvhip_plan* p, const vvhip_params* q) {
    if (!p || !q) return VVHIP_ERR_INVALID;
    TRY(settle_recovery(p));
    // topology-affecting choices are frozen at plan creation (the reference bakes them into its tables/JIT defines)
    vvhip_params n = *q;
    n.use_com_temp_group = p->hp.params.use_com_temp_group;
    n.num_nh_chains = p->hp.params.num_nh_chains;
    if (p->hp.params.auto_set_friction && q->auto_set_friction) n.friction = p->hp.params.friction;
    if ((q->cos_acceleration != 0) && p->hp.has_ld)
        return fail(p, VVHIP_ERR_TOPOLOGY, "Langevin thermostat and periodic perturbation shouldn't be used together");
    const bool cos_switch = (p->hp.params.cos_acceleration != 0) != (n.cos_acceleration != 0);
    if (cos_switch && n.cos_acceleration == 0 && p->bound && p->cur.fextra_virtual && !p->hp.has_ld && !p->hp.has_ef) {
        // forceExtra as the reference would have left it: the cos force of the last step, with the old acceleration (still in hp.params)
        // and the cos(kz) that step cached (K/cosineAccelerate.cu:9)
        TRY(run_a(p, vv::A_COS | vv::A_CZ_LOAD | vv::A_FE_STORE, 0));
        p->cur.fextra_dirty = true;
    }
    if (cos_switch) p->cur.fextra_virtual = false;
    p->hp.params = n;
    if (cos_switch && !p->launch_shape_forced) pick_launch_shape(p);      // (the cos stage sets of kernel B need more registers: another limit)
    drop_graphs(p);
    if (cos_switch && p->bound) {        // the accumulator copies are laid out by the rows in use: start the new layout from zeros
        HIP_TRY(p, hipStreamSynchronize(p->stream));
        HIP_TRY(p, hipMemsetAsync(p->d_acc.get(), 0, 2 * kAccN * sizeof(unsigned long long), p->stream));
    }
    return upload_lane_const(p);
}

int vvhip_set_box(vvhip_plan* p, const double box[3]) {
    if (!p || !box) return VVHIP_ERR_INVALID;
    p->baro.pending = false;                         // (the host has taken the box into its own hands: vvhip_barostat_restore refuses)
    if (p->box[0] == box[0] && p->box[1] == box[1] && p->box[2] == box[2]) return VVHIP_OK;      // hosts re-send it every step
    for (int i = 0; i < 3; i++) p->box[i] = box[i];
    drop_graphs(p);                                  // the box is baked into the captured kernel arguments
    return box_changed(p);                           // (an origin of pair distances under the old box has no minimum image with the new one)
}

int vvhip_masses_changed(vvhip_plan* p) {
    if (!p) return VVHIP_ERR_INVALID;
    p->mass_tab_valid = false;                       // refilled from velm.w in front of the next stage launch
    drop_graphs(p);
    return VVHIP_OK;
}

int vvhip_get_nh_state(vvhip_plan* p, vvhip_nh_state* out) {
    NEED_BOUND(p);
    TRY(settle_recovery(p));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    HIP_TRY(p, hipMemcpy(out, &p->d_nh.get()[p->cur.parity].s, sizeof(*out), hipMemcpyDeviceToHost));
    return VVHIP_OK;
}
int vvhip_set_nh_state(vvhip_plan* p, const vvhip_nh_state* in) {
    NEED_BOUND(p);
    TRY(settle_recovery(p));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    vvhip_nh_state st = *in;
    for (int g = 0; g < VVHIP_NUM_TG; g++)            // the chain's closing element is 0 by construction (API:340-376 never writes it)
        for (int i = std::max(0, std::min(p->hp.params.num_nh_chains, VVHIP_MAX_CHAINS)); i <= VVHIP_MAX_CHAINS; i++) st.eta_dot[g][i] = 0.0;
    HIP_TRY(p, hipMemcpy(&p->d_nh.get()[p->cur.parity].s, &st, sizeof(st), hipMemcpyHostToDevice));
    return VVHIP_OK;
}

// ------------------------------------------------------------------------------------------ stand-alone host support
int vvhip_device_count(int* count) {
    if (!count) return VVHIP_ERR_INVALID;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *count = e == hipSuccess ? n : 0;
    return VVHIP_OK;
}
int vvhip_set_device(int device) { return hipSetDevice(device) == hipSuccess ? VVHIP_OK : VVHIP_ERR_HIP; }
int vvhip_malloc(void** ptr, size_t bytes) { return hipMalloc(ptr, bytes ? bytes : 16) == hipSuccess ? VVHIP_OK : VVHIP_ERR_HIP; }
int vvhip_free(void* ptr) { return hipFree(ptr) == hipSuccess ? VVHIP_OK : VVHIP_ERR_HIP; }
int vvhip_memcpy_h2d(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? VVHIP_OK : VVHIP_ERR_HIP; }
int vvhip_memcpy_d2h(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? VVHIP_OK : VVHIP_ERR_HIP; }
int vvhip_memset(void* dst, int value, size_t bytes) {      // complete on return (hipMemset alone only enqueues on the null stream, which the plans' streams do not wait for)
    return hipMemset(dst, value, bytes) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess ? VVHIP_OK : VVHIP_ERR_HIP;
}
int vvhip_synchronize(vvhip_plan* p) {
    NEED_BOUND(p);
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    if (p->rec.valid && !p->rec.replaying) {
        // the run calls since the snapshot have ended: well (the snapshot is dropped), or in a missed rendezvous (they are repeated).  An overflowed
        // accumulator or an unconverged constraint cluster next to it is what steps on incomplete sums produce; if one of them was there before, the
        // repeat raises it again.
        if (__atomic_load_n(&p->h_status[2], __ATOMIC_RELAXED) != 0 && !__atomic_load_n(&p->h_status[0], __ATOMIC_RELAXED)) return recover_rendezvous(p);
        p->rec.valid = false;
        p->rec.runs.clear();
    }
    return check_exchange_health(p);      // a mailbox time-out / accumulator overflow of the work just finished surfaces here
}
int vvhip_recovery_count(vvhip_plan* p, int64_t* recoveries) {
    if (!p || !recoveries) return VVHIP_ERR_INVALID;
    *recoveries = p->rec.recoveries;
    return VVHIP_OK;
}
int vvhip_status(vvhip_plan* p, int32_t* mailbox_timed_out, int32_t* accumulator_overflow) {
    NEED_BOUND(p);
    if (mailbox_timed_out) *mailbox_timed_out = (int32_t) __atomic_load_n(&p->h_status[0], __ATOMIC_RELAXED);
    if (accumulator_overflow) *accumulator_overflow = (int32_t) __atomic_load_n(&p->h_status[1], __ATOMIC_RELAXED);
    return VVHIP_OK;
}
int vvhip_status_words(vvhip_plan* p, int32_t words[4]) {
    NEED_BOUND(p);
    if (!words) return VVHIP_ERR_INVALID;
    for (int i = 0; i < 4; i++) words[i] = (int32_t) __atomic_load_n(&p->h_status[i], __ATOMIC_RELAXED);
    return VVHIP_OK;
}
int vvhip_fused_status(vvhip_plan* p, int32_t* active, int64_t* launches, int32_t* wait_units) {
    // (see fused_active)
    NEED_BOUND(p);
    if (launches) *launches = p->fused_launches;
    if (wait_units) {                  // where the self-tuning wait of the rendezvous stands (blocks: it lives in the device-resident state)
        *wait_units = p->fused_poll_delay;
        if (p->fused_poll_delay < 0) {
            HIP_TRY(p, hipStreamSynchronize(p->stream));
            unsigned int d = 0;
            HIP_TRY(p, hipMemcpy(&d, &p->d_nh.get()[p->cur.parity].rv_delay, sizeof(d), hipMemcpyDeviceToHost));
            *wait_units = (int32_t) d;
        }
    }
    if (active) *active = fused_active(p) ? 1 : 0;
    return VVHIP_OK;
}
int vvhip_status_clear(vvhip_plan* p) {
    NEED_BOUND(p);
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    std::memset(p->h_status.get(), 0, 4 * sizeof(unsigned int));
    if (p->d_mb_ctl) HIP_TRY(p, hipMemsetAsync(p->d_mb_ctl.get(), 0, 4 * sizeof(unsigned int), p->stream));
    if (p->d_rv) HIP_TRY(p, hipMemsetAsync(rv_dead_tail(p->d_rv.get()), 0, kRvDeadTail * sizeof(unsigned long long), p->stream));      // "a rendezvous has failed" (vv_device.inc: rv_dead_word)
    p->rec.valid = false;          // (a snapshot from before the failure the caller has just acknowledged is nobody's to restore)
    p->rec.runs.clear();
    return VVHIP_OK;
}

int vvhip_stream_create(void** stream) {
    if (!stream) return VVHIP_ERR_INVALID;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return VVHIP_ERR_HIP;
    *stream = (void*) s;
    return VVHIP_OK;
}
int vvhip_stream_destroy(void* stream) { return hipStreamDestroy((hipStream_t) stream) == hipSuccess ? VVHIP_OK : VVHIP_ERR_HIP; }

}  // extern "C"
