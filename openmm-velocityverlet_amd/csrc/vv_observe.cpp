// vv_observe.cpp -- what rides beside the step, scheduled by the plan's step counter or called between steps: the Drude temperature report,
// the series of its rows, trajectory frames, profiles, mean-squared displacements, radial distribution functions, collective current
// correlations, density modes, contact lifetimes, autocorrelations, self and distinct van Hove functions, spatial distribution functions, the removal of the centre-of-mass motion, Maxwell-Boltzmann start velocities.  The scheduled ones are listed once (riders:
// when each is due is vv_schedule.hpp's business); step_begin / step_done enqueue them around a step.  The ten accumulating recorders
// share one life cycle (recorder_*) and the host-only pieces of their starts ("the shared pieces of a start": the lag schedule for seven,
// units for three, sites ordered by group for six, classes for three); origins_dead tells the six with origins that the state was rewritten.
#include "vv_plan.hpp"

#include <algorithm>

// The preamble of an entry point that works beside the steps: never inside a graph capture; the run calls since an unverified snapshot settled
// (a repaired run redoes its rows, frames and removals first); `sync`: the stream drained; `drop`: the captured graphs, which hold the riders'
// launches, gone.
int quiesce(vvhip_plan* p, const char* who, bool sync, bool drop) {
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, std::string(who) + ": not inside a graph capture");
    TRY(settle_recovery(p));
    if (sync && p->bound) HIP_TRY(p, hipStreamSynchronize(p->stream));
    if (drop) drop_graphs(p);
    return VVHIP_OK;
}

// ------------------------------------------------------------------------------------------ Drude temperature report
// The two passes' arguments on `scratch` ([8] result words, then [6 per molecule] momentum words; zero on entry)
static vv::ReportArgs report_args(const vvhip_plan* p, long long* scratch) {
    const vv::HostPlan& hp = p->hp;
    vv::ReportArgs a{};
    a.velm = p->buf.velm; a.slots = p->d_slots.get();
    a.lane_mol = p->d_rep_lane_mol.get(); a.lane_mass = p->d_rep_lane_mass.get(); a.lane_mu = p->d_rep_lane_mu.get();
    a.mol_mass = p->d_rep_mol_mass.get(); a.cross = p->d_rep_cross.get(); a.cross_mu = p->d_rep_cross_mu.get();
    a.out = scratch; a.mol_p = scratch ? scratch + 8 : nullptr;
    a.nwaves = hp.info.num_waves; a.nmol = (int) hp.report_mol_mass.size(); a.ncross = (int) hp.report_cross_mu.size();
    a.frac_bits = hp.report_frac_bits;
    a.unit = std::ldexp(1.0, hp.report_unit_bits); a.frac_scale = std::ldexp(1.0, hp.report_frac_bits);
    a.inv_unit = std::ldexp(1.0, -hp.report_unit_bits); a.inv_full = std::ldexp(1.0, -hp.report_unit_bits - hp.report_frac_bits);
    a.limit = hp.report_limit;
    return a;
}

// ------------------------------------------------------------------------------------------ series (vvhip_series_*)
// One row behind the step just enqueued (or captured): the report's passes on the series' scratch, then the append kernel, which also
// zeroes that scratch again.  Three kernel launches, no memset and no host synchronisation.
static int series_row(vvhip_plan* p) {
    vvhip_plan::Series& S = p->series;
    vv::SeriesArgs a{};
    if (S.mask & VVHIP_SERIES_DRUDE) {
        HIP_TRY(p, vv::launch_report(p->hp.precision, report_args(p, S.d_scratch.get()), p->block_threads, p->grid_cap_a, p->stream));
        a.rep_out = S.d_scratch.get(); a.rep_mol_p = S.d_scratch.get() + 8; a.rep_mol_words = 6 * (int64_t) p->hp.report_mol_mass.size();
    }
    if (S.mask & VVHIP_SERIES_THERMOSTAT) a.nh = &p->d_nh.get()[p->cur.parity].s;
    a.rows = (vvhip_series_row*) S.ring.d_items.get(); a.cursor = S.ring.d_cursor.get(); a.capacity = S.ring.capacity;
    for (int k = 0; k < 3; k++) a.box[k] = p->box[k];
    a.cos_acceleration = p->hp.params.cos_acceleration;
    HIP_TRY(p, vv::launch_series_append(a, p->grid_cap_a, p->stream));
    return VVHIP_OK;
}
// ------------------------------------------------------------------------------------------ frames (vvhip_frames_*)
// One frame behind the step just enqueued (or captured), and behind its series row: the streaming kernel and the one-thread kernel that
// writes the header and advances the cursor.  Two launches, no memset and no host synchronisation.
static int frame_enqueue(vvhip_plan* p) {
    const vvhip_plan::Frames& F = p->frames;
    vv::FrameArgs a{};
    a.posq = p->buf.posq; a.corr = posq_corr(p); a.velm = p->buf.velm;
    a.subset = F.has_subset ? F.d_subset.get() : nullptr;
    a.frames = F.ring.d_items.get(); a.cursor = F.ring.d_cursor.get();
    a.frame_bytes = F.frame_bytes; a.off_positions = F.off_positions; a.off_velocities = F.off_velocities;
    a.n = F.num_particles; a.plane_stride = F.plane_stride; a.capacity = F.ring.capacity;
    for (int k = 0; k < 3; k++) a.box[k] = p->box[k];
    HIP_TRY(p, vv::launch_frame(p->hp.precision, a, (F.mask & VVHIP_FRAMES_FLOAT64) != 0, p->grid_cap_a, p->stream));
    return VVHIP_OK;
}
// ------------------------------------------------------------------------------------------ profiles (vvhip_profile_*)
// One sample behind the step just enqueued (or captured), and behind its frame: the accumulating kernel and the one-thread kernel that
// counts the sample.  Two launches, no memset and no host synchronisation.
static int profile_enqueue(vvhip_plan* p) {
    const vvhip_plan::Profile& P = p->profile;
    const vvhip_profile_layout& L = P.lay;
    vv::ProfileArgs a{};
    a.posq = p->buf.posq; a.corr = posq_corr(p); a.velm = p->buf.velm;
    a.index = P.index.empty() ? nullptr : P.dev.index.get(); a.group = P.grouped ? P.dev.group.get() : nullptr; a.mass = P.dev.mass.get();
    a.words = P.d_words.get(); a.max_samples = L.max_samples;
    a.n = L.num_particles; a.nbins = L.nbins; a.axis = L.axis; a.mask = L.mask; a.rows = L.rows; a.table_words = (int32_t) L.words;
    a.inv_L = 1.0 / p->box[L.axis];
    for (int q = 0; q < 4; q++) { a.scale[q] = std::ldexp(1.0, L.frac_bits[q + 1]); a.limit[q] = L.limit[q + 1]; }
    HIP_TRY(p, vv::launch_profile(p->hp.precision, a, std::min(p->grid_cap_a, p->profile_grid_cap), p->stream));
    return VVHIP_OK;
}
// The threads per block of an MSD, current or autocorrelation sample's accumulating kernel (`pinned` != 0: a test hook's): 512 where they still make 128
// blocks, else the largest of 256, 128, 64 that does (64 at the least): few units in few blocks leave their gathers to a handful of CUs
// (TUNING_LOG.md)
static int block_threads_for(int pinned, int n) {
    int threads = pinned;
    if (threads == 0)
        for (threads = 512; threads > 64 && (n + threads - 1) / threads < 128; threads /= 2) {}
    return threads;
}
// ------------------------------------------------------------------------------------------ mean-squared displacements (vvhip_msd_*)
// One sample behind the step just enqueued (or captured), and behind its profile sample: the accumulating kernel and the one-thread kernel
// that advances the ordinal.  Two launches, no memset and no host synchronisation.
static int msd_enqueue(vvhip_plan* p) {
    const vvhip_plan::Msd& M = p->msd;
    const vvhip_msd_layout& L = M.lay;
    vv::MsdArgs a{};
    a.posq = p->buf.posq; a.corr = posq_corr(p);
    const bool molecules = M.molecules;
    a.index = M.index.empty() ? nullptr : M.dev.index.get();
    a.first = molecules ? M.dev.first.get() : nullptr; a.weight = molecules ? M.dev.weight.get() : nullptr; a.total = molecules ? M.dev.total.get() : nullptr;
    a.group = M.grouped ? M.dev.group.get() : nullptr;
    a.words = M.d_words.get(); a.ring = (double*) (M.d_words.get() + M.table_offset() + L.words);
    a.max_samples = L.max_samples;
    a.n = L.num_units; a.stride = M.stride(); a.num_lags = L.num_lags; a.origin_every = L.origin_every; a.num_origins = L.num_origins;
    a.table_words = (int32_t) L.words; a.wave_reduce = p->msd_wave_reduce;
    a.scale = std::ldexp(1.0, L.frac_bits); a.limit = L.limit;
    HIP_TRY(p, vv::launch_msd(p->hp.precision, a, block_threads_for(p->msd_block_threads, a.n), std::min(p->grid_cap_a, p->profile_grid_cap), p->stream));
    return VVHIP_OK;
}
// ------------------------------------------------------------------------------------------ radial distribution functions (vvhip_rdf_*)
// r against the box: one image per pair.  `what` names r in the refusal ("r_max = ", "the cutoff ")
static bool box_holds(const double box[3], double r) { return r <= std::min(box[0], std::min(box[1], box[2])) / 2; }
static int check_half_box(vvhip_plan* p, const char* name, const char* what, double r) {
    if (box_holds(p->box, r)) return VVHIP_OK;
    return fail(p, VVHIP_ERR_INVALID, std::string(name) + ": " + what + std::to_string(r) + " nm is above half the shortest edge of the box (" +
                                      std::to_string(std::min(p->box[0], std::min(p->box[1], p->box[2]))) + " nm): a pair would have more than one image in range");
}
// One sample behind the step just enqueued (or captured), and behind its MSD sample -- or behind what is queued (vvhip_rdf_sample): the
// gather, the pair kernel and the one-thread kernel that counts the sample.  Three launches, no memset and no host synchronisation.  The
// box and whether it still holds r_max are arguments: what changes the box drops the captured graphs.
static int rdf_enqueue(vvhip_plan* p) {
    const vvhip_plan::Rdf& R = p->rdf;
    const vvhip_rdf_layout& L = R.lay;
    vv::RdfArgs a{};
    a.posq = p->buf.posq; a.corr = posq_corr(p);
    a.index = R.dev.index.get(); a.mol = L.exclude_same_molecule ? R.dev.mol.get() : nullptr; a.items = R.dev.items.get();
    a.scratch = R.dev.scratch.get(); a.words = R.d_words.get();
    a.max_samples = L.max_samples;
    a.n = (int32_t) R.index.size(); a.stride = R.stride(); a.nbins = L.nbins; a.num_items = (int32_t) R.items.size();
    // (one histogram per wave only where all of them fit beside the staged tile)
    a.copies = p->rdf_hist_copies > 1 && vv::rdf_lds_bytes(L.nbins, vv::RDF_TILE / 64) <= vv::PROFILE_LDS_BYTES ? vv::RDF_TILE / 64 : 1;
    a.live = box_holds(p->box, L.r_max) ? 1 : 0;
    a.max_jsites = R.max_jsites;
    for (int k = 0; k < 3; k++) { a.L[k] = p->box[k]; a.inv_L[k] = 1.0 / p->box[k]; }
    a.dr = L.dr; a.cut2 = ((double) L.nbins * L.dr) * ((double) L.nbins * L.dr); a.inv_dr = (float) (1.0 / L.dr);
    a.inv_volume = 1.0 / ((p->box[0] * p->box[1]) * p->box[2]);
    HIP_TRY(p, vv::launch_rdf(p->hp.precision, a, p->grid_cap_a, p->stream));
    return VVHIP_OK;
}
// ------------------------------------------------------------------------------------------ collective current correlations (vvhip_current_*)
// One sample behind the step just enqueued (or captured), and behind its RDF sample: the reduce, the correlate and the one-wave kernel that
// stores the origin and counts the sample.  Three launches, no memset and no host synchronisation.  1 / V is an argument: what changes the
// box drops the captured graphs.
static int current_enqueue(vvhip_plan* p) {
    const vvhip_plan::Current& K = p->current;
    const vvhip_current_layout& L = K.lay;
    vv::CurrentArgs a{};
    a.posq = p->buf.posq; a.corr = posq_corr(p); a.velm = p->buf.velm;
    a.index = K.dev.index.get(); a.weight = K.dev.weight.get(); a.group = K.dev.group.get();
    a.words = K.d_words.get(); a.table = a.words + K.table_offset(); a.ring = a.table + L.words;
    a.hold = a.ring + (size_t) L.num_origins * K.sums_words();
    a.slabs = K.dev.slabs.get();    // (null: one level)
    a.max_samples = L.max_samples;
    a.n = L.num_particles; a.num_groups = L.num_groups; a.num_lags = L.num_lags; a.origin_every = L.origin_every;
    a.num_origins = L.num_origins; a.row_words = L.row_words;
    a.scale_p = std::ldexp(1.0, L.frac_bits_position); a.scale_v = std::ldexp(1.0, L.frac_bits_velocity);
    a.inv_scale_p = std::ldexp(1.0, -L.frac_bits_position); a.inv_scale_v = std::ldexp(1.0, -L.frac_bits_velocity);
    a.limit_p = L.limit_position; a.limit_v = L.limit_velocity;
    a.inv_volume = 1.0 / ((p->box[0] * p->box[1]) * p->box[2]);
    HIP_TRY(p, vv::launch_current(p->hp.precision, a, block_threads_for(p->current_block_threads, a.n), std::min(p->grid_cap_a, p->profile_grid_cap), p->stream));
    return VVHIP_OK;
}
// ------------------------------------------------------------------------------------------ density modes (vvhip_modes_*)
// One sample behind the step just enqueued (or captured), and behind its current sample: the gather, the mode kernel, the correlate and the
// one-wave kernel that stores the origin and counts the sample.  Four launches, no memset and no host synchronisation.  1 / L and the box
// are arguments: what changes the box drops the captured graphs, and the wave vectors follow the new box.
static int modes_enqueue(vvhip_plan* p) {
    const vvhip_plan::Modes& M = p->modes;
    const vvhip_modes_layout& L = M.lay;
    vv::ModesArgs a{};
    a.posq = p->buf.posq; a.corr = posq_corr(p);
    a.index = M.dev.index.get(); a.weight = M.dev.weight.get(); a.modes = M.dev.modes.get(); a.items = M.dev.items.get();
    a.turns = M.dev.turns.get();
    a.words = M.d_words.get(); a.table = a.words + M.table_offset(); a.ring = a.table + L.words;
    a.hold = a.ring + (size_t) L.num_origins * M.sums_words();
    a.max_samples = L.max_samples;
    a.n = L.num_particles; a.stride = M.stride(); a.num_groups = L.num_groups; a.num_modes = L.num_modes;
    a.num_lags = L.num_lags; a.origin_every = L.origin_every; a.num_origins = L.num_origins; a.row_words = L.row_words;
    a.num_items = L.num_items;
    for (int k = 0; k < 3; k++) { a.inv_L[k] = 1.0 / p->box[k]; a.box[k] = p->box[k]; }
    a.limit = L.limit_position;
    a.scale = std::ldexp(1.0, L.frac_bits); a.inv_scale = std::ldexp(1.0, -L.frac_bits);
    HIP_TRY(p, vv::launch_modes(p->hp.precision, a, L.sites_per_thread, L.block_threads, p->grid_cap_a, p->stream));
    return VVHIP_OK;
}
// ------------------------------------------------------------------------------------------ contact lifetime correlations (vvhip_contacts_*)
// One sample behind the step just enqueued (or captured), and behind its density-mode sample -- or behind what is queued
// (vvhip_contacts_sample): the gather, the mask kernel, the correlate kernel and the one-wave kernel that counts the sample.  Four launches,
// no memset and no host synchronisation.  The box and whether it still holds the largest cutoff are arguments: what changes the box drops
// the captured graphs.  A barostat move leaves the origins alone: a contact set belongs to a configuration, not to a displacement.
static int contacts_enqueue(vvhip_plan* p) {
    const vvhip_plan::Contacts& K = p->contacts;
    const vvhip_contacts_layout& L = K.lay;
    const vv::ContactsLayout& G = K.geo;
    vv::ContactsArgs a{};
    a.posq = p->buf.posq; a.corr = posq_corr(p);
    a.index = K.dev.index.get(); a.mol = L.exclude_same_molecule ? K.dev.mol.get() : nullptr;
    a.mask_items = K.dev.mask_items.get(); a.corr_items = K.dev.corr_items.get();
    a.scratch = K.dev.scratch.get(); a.mask = K.dev.mask.get();
    a.words = K.d_words.get(); a.table = a.words + K.table_offset(); a.ord = a.table + L.words;
    a.origin = (unsigned long long*) (a.ord + G.ord_words);
    a.cont = L.continuous ? a.origin + (size_t) G.num_origins * (size_t) G.sample_words : nullptr;
    a.max_samples = L.max_samples; a.sample_words = G.sample_words;
    a.n = (int32_t) K.index.size(); a.stride = K.stride();
    a.num_mask_items = L.num_mask_items; a.num_corr_items = L.num_corr_items;
    a.num_classes = L.num_classes; a.num_lags = L.num_lags; a.origin_every = L.origin_every; a.num_origins = L.num_origins;
    a.skip_zero = p->contacts_skip_zero; a.rows_per_tile = L.rows_per_tile;
    double largest = 0;
    for (int c = 0; c < L.num_classes; c++) {
        largest = std::max(largest, L.r_cut[c]);
        a.cut2[c] = L.r_cut[c] * L.r_cut[c];
        a.class_offset[c] = G.class_offset[c]; a.rows_padded[c] = (int32_t) G.rows_padded[c];
        a.rows[c] = L.rows[c]; a.cols[c] = L.cols[c];
        a.first_row[c] = K.first[L.classes[c][0]]; a.first_col[c] = K.first[L.classes[c][1]];
    }
    a.live = box_holds(p->box, largest) ? 1 : 0;
    for (int k = 0; k < 3; k++) { a.L[k] = p->box[k]; a.inv_L[k] = 1.0 / p->box[k]; }
    HIP_TRY(p, vv::launch_contacts(p->hp.precision, a, p->grid_cap_a, p->stream));
    return VVHIP_OK;
}
// ------------------------------------------------------------------------------------------ autocorrelations (vvhip_acf_*)
// One sample behind the step just enqueued (or captured), and behind its contact sample: the accumulating kernel and the one-thread kernel
// that advances the ordinal.  Two launches, no memset and no host synchronisation.
static int acf_enqueue(vvhip_plan* p) {
    const vvhip_plan::Acf& A = p->acf;
    const vvhip_acf_layout& L = A.lay;
    vv::AcfArgs a{};
    a.velm = p->buf.velm; a.posq = p->buf.posq; a.corr = posq_corr(p);
    const bool molecules = A.molecules;
    a.index = A.index.empty() ? nullptr : A.dev.index.get();
    a.first = molecules ? A.dev.first.get() : nullptr; a.weight = molecules ? A.dev.weight.get() : nullptr; a.total = molecules ? A.dev.total.get() : nullptr;
    a.group = A.grouped ? A.dev.group.get() : nullptr;
    a.words = A.d_words.get(); a.ring = (double*) (A.d_words.get() + A.table_offset() + L.words);
    a.max_samples = L.max_samples;
    a.n = L.num_units; a.stride = A.stride(); a.num_lags = L.num_lags; a.origin_every = L.origin_every; a.num_origins = L.num_origins;
    a.table_words = (int32_t) L.words; a.wave_reduce = p->acf_wave_reduce; a.slots_in_flight = p->acf_slots_in_flight;
    a.scale = std::ldexp(1.0, L.frac_bits); a.limit = L.limit;
    HIP_TRY(p, vv::launch_acf(p->hp.precision, a, L.mode, block_threads_for(p->acf_block_threads, a.n), std::min(p->grid_cap_a, p->profile_grid_cap), p->stream));
    return VVHIP_OK;
}
// ------------------------------------------------------------------------------------------ self van Hove functions (vvhip_vanhove_*)
// One sample behind the step just enqueued (or captured), and behind its autocorrelation sample: the accumulating kernel and the one-thread
// kernel that advances the ordinal.  Two launches, no memset and no host synchronisation.
static int vanhove_enqueue(vvhip_plan* p) {
    const vvhip_plan::VanHove& V = p->vanhove;
    const vvhip_vanhove_layout& L = V.lay;
    vv::VanHoveArgs a{};
    a.posq = p->buf.posq; a.corr = posq_corr(p);
    const bool molecules = V.molecules;
    a.index = V.index.empty() ? nullptr : V.dev.index.get();
    a.first = molecules ? V.dev.first.get() : nullptr; a.weight = molecules ? V.dev.weight.get() : nullptr; a.total = molecules ? V.dev.total.get() : nullptr;
    a.group = V.grouped ? V.dev.group.get() : nullptr;
    a.e2 = V.d_e2.get();
    a.words = V.d_words.get(); a.ring = (double*) (V.d_words.get() + V.table_offset() + L.words);
    a.max_samples = L.max_samples; a.head_words = L.head_words;
    a.n = L.num_units; a.stride = V.stride(); a.num_lags = L.num_lags; a.origin_every = L.origin_every; a.num_origins = L.num_origins;
    a.num_bins = L.num_bins; a.wave_reduce = p->vanhove_wave_reduce;
    a.lds_groups = p->vanhove_lds ? std::min(L.num_groups, vv::VANHOVE_LDS_WORDS / L.num_bins) : 0;
    a.scale2 = std::ldexp(1.0, L.frac2_bits); a.scale_hi = std::ldexp(1.0, L.r4_hi_bits); a.scale_lo = std::ldexp(1.0, L.r4_lo_bits); a.limit = L.limit;
    HIP_TRY(p, vv::launch_vanhove(p->hp.precision, a, block_threads_for(p->vanhove_block_threads, a.n), std::min(p->grid_cap_a, p->profile_grid_cap), p->stream));
    return VVHIP_OK;
}
// ------------------------------------------------------------------------------------------ distinct van Hove functions (vvhip_vanhove_distinct_*)
// One sample behind the step just enqueued (or captured), and behind its self van Hove sample: the gather into the planes of "now", the
// pair kernel over (work items) x (ring slots) and the one-thread kernel that counts the visits and advances the ordinal.  Three launches,
// no memset, no copy and no host synchronisation.  The box and whether it still holds r_max are arguments: what changes the box drops
// the captured graphs.
static int vhd_enqueue(vvhip_plan* p) {
    const vvhip_plan::Vhd& V = p->vhd;
    const vvhip_vanhove_distinct_layout& L = V.lay;
    vv::VhdArgs a{};
    a.posq = p->buf.posq; a.corr = posq_corr(p);
    a.index = V.dev.index.get(); a.mol = L.exclude_same_molecule ? V.dev.mol.get() : nullptr; a.items = V.dev.items.get();
    a.words = V.d_words.get(); a.ring = (double*) (V.d_words.get() + V.table_offset() + L.words);
    a.max_samples = L.max_samples; a.head_words = L.head_words;
    a.n = (int32_t) V.index.size(); a.stride = V.stride(); a.nbins = L.nbins; a.num_items = (int32_t) V.items.size();
    a.num_lags = L.num_lags; a.origin_every = L.origin_every; a.num_origins = L.num_origins;
    // (one histogram per wave only where all of them fit beside the staged tile)
    a.copies = p->vhd_lds && p->vhd_hist_copies > 1 && vv::rdf_lds_bytes(L.nbins, vv::RDF_TILE / 64) <= vv::PROFILE_LDS_BYTES ? vv::RDF_TILE / 64 : 1;
    a.live = box_holds(p->box, L.r_max) ? 1 : 0;
    a.max_jsites = V.max_jsites;
    for (int k = 0; k < 3; k++) { a.L[k] = p->box[k]; a.inv_L[k] = 1.0 / p->box[k]; }
    a.dr = L.dr; a.cut2 = ((double) L.nbins * L.dr) * ((double) L.nbins * L.dr); a.inv_dr = (float) (1.0 / L.dr);
    a.inv_volume = 1.0 / ((p->box[0] * p->box[1]) * p->box[2]);
    HIP_TRY(p, vv::launch_vhd(p->hp.precision, a, p->vhd_lds != 0, p->grid_cap_a, p->stream));
    return VVHIP_OK;
}
// ------------------------------------------------------------------------------------------ spatial distribution functions (vvhip_sdf_*)
// The cube against the box: its corners lie 3^(1/2) h from the frame's origin, and a sphere of that radius must hold one image per site
static bool box_holds_cube(const double box[3], double h) {
    const double half = std::min(box[0], std::min(box[1], box[2])) / 2;
    return 3.0 * (h * h) < half * half;
}
// One sample behind the step just enqueued (or captured), and behind its distinct van Hove sample -- or behind what is queued
// (vvhip_sdf_sample): the gather of sites and frames, the pair kernel and the one-thread kernel that counts the sample.  Three launches, no
// memset and no host synchronisation.  The box and whether it still holds the cube are arguments: what changes the box drops the
// captured graphs.
static int sdf_enqueue(vvhip_plan* p) {
    const vvhip_plan::Sdf& R = p->sdf;
    const vvhip_sdf_layout& L = R.lay;
    vv::SdfArgs a{};
    a.posq = p->buf.posq; a.corr = posq_corr(p);
    a.index = R.dev.index.get(); a.mol = L.exclude_same_molecule ? R.dev.mol.get() : nullptr;
    a.frames = R.dev.frames.get(); a.fmol = L.exclude_same_molecule ? R.dev.fmol.get() : nullptr; a.fgroup = R.dev.fgroup.get();
    a.items = R.dev.items.get(); a.scratch = R.dev.scratch.get(); a.words = R.d_words.get();
    a.max_samples = L.max_samples;
    a.n = (int32_t) R.index.size(); a.stride = R.stride(); a.nf = (int32_t) R.fgroup.size(); a.fstride = R.fstride();
    a.nbins = L.nbins; a.num_items = (int32_t) R.items.size();
    a.live = box_holds_cube(p->box, L.extent) ? 1 : 0;
    a.max_jsites = R.max_jsites;
    for (int k = 0; k < 3; k++) { a.L[k] = p->box[k]; a.inv_L[k] = 1.0 / p->box[k]; }
    a.h = L.extent; a.inv_w = (double) L.nbins / (2.0 * L.extent);
    a.cut2 = (3.0 * (L.extent * L.extent)) * (1.0 + 0x1p-20);
    a.inv_volume = 1.0 / ((p->box[0] * p->box[1]) * p->box[2]);
    HIP_TRY(p, vv::launch_sdf(p->hp.precision, a, p->grid_cap_a, p->stream));
    return VVHIP_OK;
}
// The positions or the velocities were rewritten outside the steps (vv_barostat.cpp; vvhip_set_velocities_to_temperature): the origins that
// the recorders of that quantity stored so far are dead.  Positions: msd, current, modes, vanhove, vhd, their floors raised in this order; velocities:
// acf, unless it records orientations.  A contact set belongs to a configuration, not to a displacement: contacts reacts to neither.
int origins_dead(vvhip_plan* p, Rewrote what) {
    if (what == Rewrote::POSITIONS) {
        if (p->msd.on) HIP_TRY(p, vv::launch_msd_floor(p->msd.d_words.get(), p->stream));
        if (p->current.on) HIP_TRY(p, vv::launch_current_floor(p->current.d_words.get(), p->stream));
        if (p->modes.on) HIP_TRY(p, vv::launch_modes_floor(p->modes.d_words.get(), p->stream));
        if (p->vanhove.on) HIP_TRY(p, vv::launch_vanhove_floor(p->vanhove.d_words.get(), p->stream));
        if (p->vhd.on) HIP_TRY(p, vv::launch_vhd_floor(p->vhd.d_words.get(), p->stream));
    } else if (p->acf.on && p->acf.lay.mode != VVHIP_ACF_ORIENTATION) HIP_TRY(p, vv::launch_acf_floor(p->acf.d_words.get(), p->stream));
    return VVHIP_OK;
}
// vvhip_set_box replaced the box with another one: the distinct van Hove recorder's origins have no minimum image with it.  (The recorders
// of displacements keep theirs: an unwrapped displacement does not depend on the box.)
int box_changed(vvhip_plan* p) {
    if (p->vhd.on && !p->capturing) HIP_TRY(p, vv::launch_vhd_floor(p->vhd.d_words.get(), p->stream));
    return VVHIP_OK;
}
// ------------------------------------------------------------------------------------------ centre-of-mass motion (vvhip_cm_motion_*)
static bool cmm_sharded(const vvhip_plan* p) { return p->hp.shard_begin != 0 || p->hp.shard_end != p->hp.num_atoms; }
static const char kCmmSharded[] = "centre-of-mass motion: a sharded plan holds a part of the momentum only (summing over the ranks is not implemented)";
static int cmm_ensure(vvhip_plan* p) {
    vvhip_plan::CmMotion& M = p->cmm;
    if (M.d_words && M.d_rec && M.h_v) return VVHIP_OK;
    HIP_TRY(p, vv::zeros(M.d_words, vv::CMM_WORDS * sizeof(long long), p->stream));
    HIP_TRY(p, vv::zeros(M.d_rec, 2 * sizeof(vv::CmmDevRecord), p->stream));
    HIP_TRY(p, M.h_v.alloc(3 * sizeof(double)));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    return VVHIP_OK;
}
// The pair of kernels behind what is queued (or captured); which = 0: a scheduled removal, 1: a one-off call (records of their own)
static int cmm_enqueue(vvhip_plan* p, int which) {
    TRY(settle_recovery(p));
    vv::CmmArgs a{};
    a.rep = report_args(p, nullptr);
    a.words = p->cmm.d_words.get();
    a.rec = p->cmm.d_rec.get() + which;
    a.inv_total_mass = p->hp.cm_total_mass > 0 ? 1.0 / p->hp.cm_total_mass : 0.0;
    HIP_TRY(p, vv::launch_cm_motion(p->hp.precision, a, p->block_threads, p->grid_cap_a, p->stream));
    return VVHIP_OK;
}
// A one-off removal behind what is queued, and its V: blocks (the call's one synchronisation).  NaN is what the subtract kernel records for
// a removal it skipped.
static int cmm_one_off(vvhip_plan* p, double v[3]) {
    TRY(cmm_enqueue(p, 1));
    HIP_TRY(p, hipMemcpyAsync(p->cmm.h_v.get(), p->cmm.d_rec.get()[1].last_v, 3 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    if (std::isnan(p->cmm.h_v[0]))
        return fail(p, VVHIP_ERR_OVERFLOW, "centre-of-mass motion: a momentum term is NaN or beyond the fixed-point range; nothing was subtracted");
    if (v) std::memcpy(v, p->cmm.h_v.get(), 3 * sizeof(double));
    return VVHIP_OK;
}
// ------------------------------------------------------------------------------------------ the step's scheduled riders
// In this order everywhere (item k of GraphKey::due, of Recovery::late), which is the order they ride in, each with its late words:
//   0 series row        behind its step; the ring's cursor while the series runs: a row written twice is the same row
//   1 removal of the centre-of-mass motion   in FRONT of its step; the schedule's record whenever it exists (one-off calls allocate it too)
//   2 trajectory frame  behind the row; the ring's cursor while the recorder runs: a frame written twice is the same frame
//   3 profile sample    behind the frame; ALL of d_words, counts and table: a sample added twice is not the same table
//   4 MSD sample        behind the profile sample; all of d_words, the ring of origins included: the repeat needs the origins it overwrote
//   5 RDF sample        behind the MSD sample; all of d_words, counts and table (its gather scratch is rewritten by every sample)
//   6 current sample    behind the RDF sample; all of d_words: head, sums, table, the ring of origins and the slots' words
//   7 density-mode sample   behind the current sample; all of d_words likewise (its turns are scratch, rewritten by every sample)
//   8 contact sample    behind the density-mode sample; all of d_words: head, table, the slots' ordinals and both rings (the sample's matrix and planes are scratch)
//   9 autocorrelation sample   behind the contact sample; all of d_words, the ring of origins included, as for the MSD
//  10 self van Hove sample   behind the autocorrelation sample; all of d_words likewise: head, histogram and the ring of origins
//  11 distinct van Hove sample   behind the self van Hove sample; all of d_words: counts, head, histogram, the ring of origins and the spare planes
//  12 spatial distribution sample   last; all of d_words, counts and table (its gather scratch is rewritten by every sample)
// Riders 3 .. 12 are the ten accumulating recorders: one descriptor shape (recorder_rider), bytes() of d_words as the late words.  Their
// host tables come from "the shared pieces of a start" below (units: 4, 9 and 10; sites ordered by group: 5 .. 8, 11 and 12; the lag schedule: 4, 6 .. 11),
// and origins_dead above reaches 4, 6, 7, 10, 11 (positions) and 9 (velocities).
template <class R>
static Rider recorder_rider(const R& r, int (*enqueue)(vvhip_plan*)) { return {r.on, r.when, false, r.on ? r.d_words.get() : nullptr, r.bytes(), enqueue}; }
Riders riders(vvhip_plan* p) {
    return {{{p->series.on, p->series.when, false, p->series.on ? p->series.ring.d_cursor.get() : nullptr, sizeof(unsigned long long[2]), series_row},
             {p->cmm.on, p->cmm.when, true, p->cmm.d_rec.get(), sizeof(vv::CmmDevRecord), [](vvhip_plan* q) { return cmm_enqueue(q, 0); }},
             {p->frames.on, p->frames.when, false, p->frames.on ? p->frames.ring.d_cursor.get() : nullptr, sizeof(unsigned long long[2]), frame_enqueue},
             recorder_rider(p->profile, profile_enqueue), recorder_rider(p->msd, msd_enqueue), recorder_rider(p->rdf, rdf_enqueue),
             recorder_rider(p->current, current_enqueue), recorder_rider(p->modes, modes_enqueue), recorder_rider(p->contacts, contacts_enqueue),
             recorder_rider(p->acf, acf_enqueue), recorder_rider(p->vanhove, vanhove_enqueue), recorder_rider(p->vhd, vhd_enqueue),
             recorder_rider(p->sdf, sdf_enqueue)}};
}
// A full step is about to be enqueued (or captured) / has been: the riders in front of it / the count, then the riders behind it.  The two
// hooks of every entry point that starts / ends a step.
static int enqueue_due(vvhip_plan* p, bool in_front) {
    for (const Rider& r : riders(p))
        if (r.on && r.in_front == in_front && due(r.when, p->cur.step_count)) TRY(r.enqueue(p));
    return VVHIP_OK;
}
int step_begin(vvhip_plan* p) { return enqueue_due(p, true); }
int step_done(vvhip_plan* p) {
    p->cur.step_count++;
    return enqueue_due(p, false);
}
// frexp's view of a positive finite x: the smallest power of two >= x / > x, and the exponent of a power of two
static double pow2_at_least(double x) { int e; const double f = std::frexp(x, &e); return f == 0.5 ? x : std::ldexp(1.0, e); }
static double pow2_above(double x) { int e; (void) std::frexp(x, &e); return std::ldexp(1.0, e); }
static int ceil_log2(long long n) { int k = 0; while (k < 62 && (1ll << k) < n) k++; return k; }      // smallest k with 2^k >= n (1 <= n <= 2^62)
// max_samples + more as the fixed point counts it: 2^62 at the most
static long long samples_plus(long long max_samples, long long more) { return max_samples < (1ll << 62) ? max_samples + more : (1ll << 62); }

// ------------------------------------------------------------------------------------------ the recorders' one life cycle
// What the series, the frame recorder and the ten accumulating recorders (vvhip_plan::Recorder) go through, stated once; `which` is the
// plan's member, `name` the prefix of its messages and the middle of its entry points' names.
// One that runs is settled and goes first (its rows, frames or samples may still be in flight); the description an unbound plan kept goes
// with it.  All of *_stop, and the front of a start over a running recorder.
template <class R>
static int recorder_stop(vvhip_plan* p, R vvhip_plan::* which, const char* name) {
    if (!p) return VVHIP_ERR_INVALID;
    if (p->capturing || (p->*which).on) TRY(quiesce(p, name, true, true));
    p->*which = R{};
    return VVHIP_OK;
}
// The tail of *_start, behind the host-only part that built `N` and every refusal of the description: the running recorder goes, the
// description moves in (an unbound plan keeps it, and is refused only then), the device tables follow.
template <class R>
static int recorder_install(vvhip_plan* p, R vvhip_plan::* which, const char* name, R& N, int32_t interval) {
    TRY(recorder_stop(p, which, name));
    R& rec = p->*which;
    rec = std::move(N);
    rec.when = {interval, SCHEDULE_LINEAR};
    rec.lay.start_step = p->cur.step_count;
    rec.described = true;
    NEED_BOUND(p);
    TRY(quiesce(p, name, true, true));
    size_t asked = 0;
    const hipError_t e = rec.alloc(p->stream, &asked);
    if (e != hipSuccess) {
        rec.d_words.reset(); rec.dev = {};
        (void) hipGetLastError();
        return fail(p, VVHIP_ERR_HIP, std::string(name) + ": allocating " + std::to_string((unsigned long long) asked) + " bytes failed: " + hipGetErrorString(e));
    }
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    rec.lay.start_step = p->cur.step_count;                 // (a settled recovery may have moved the counter)
    rec.on = true;
    return VVHIP_OK;
}
// The front of *_read: the refusals, then the stream drained and R::kHead count words in `head`, the table in `words_out`
template <class R>
static int recorder_fetch(vvhip_plan* p, R vvhip_plan::* which, const char* name, int64_t* words_out, int64_t capacity_words, long long* head) {
    NEED_BOUND(p);
    const R& rec = p->*which;
    if (!rec.on) return fail(p, VVHIP_ERR_INVALID, std::string(name) + ": none started (vvhip_" + name + "_start)");
    if (capacity_words < 0 || (capacity_words > 0 && !words_out) || (words_out && capacity_words < rec.lay.words))
        return fail(p, VVHIP_ERR_INVALID, std::string(name) + ": the table has " + std::to_string((long long) rec.lay.words) + " words; words_out must hold them all (or be NULL with capacity_words = 0)");
    TRY(quiesce(p, name, true, false));
    HIP_TRY(p, hipMemcpy(head, rec.d_words.get(), R::kHead * sizeof(long long), hipMemcpyDeviceToHost));
    if (words_out && rec.lay.words > 0) HIP_TRY(p, hipMemcpy(words_out, rec.d_words.get() + rec.table_offset(), (size_t) rec.lay.words * sizeof(long long), hipMemcpyDeviceToHost));
    return VVHIP_OK;
}
// ... and its end, behind the entry point's conversion of the count words: the reset, complete on return
template <class R>
static int recorder_reset(vvhip_plan* p, R& rec) {
    HIP_TRY(p, rec.reset(p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    return VVHIP_OK;
}
// *_info: `blank` (zeroes, but for a profile's row_of) until a description passed, then its layout
template <class R, class L>
static int recorder_info(const vvhip_plan* p, R vvhip_plan::* which, L* out, L blank = L{}) {
    if (!p || !out) return VVHIP_ERR_INVALID;
    const R& rec = p->*which;
    if (rec.described) { blank = rec.lay; blank.active = rec.on; }
    *out = blank;
    return VVHIP_OK;
}

// ------------------------------------------------------------------------------------------ the shared pieces of a start
// The host-only part of the accumulating recorders' *_start, stated once; `name` is the prefix of the messages.  What a recorder still
// writes itself: its own argument checks, its layout, its fixed point (but for units_frac_bits), its work list, its enqueue.
//   check_groups, check_max_samples   all ten                 check_lags            msd, acf, vanhove, vhd, current, modes, contacts
//   num_origins_of                    msd, acf, vanhove, vhd, current, modes; check_origins       msd, acf, vanhove, vhd, contacts
//   plan_units, fill_units   msd, acf, vanhove; units_frac_bits   msd, acf        sites_by_group        rdf, vhd, sdf, current, modes, contacts
//   check_classes, check_half_box (beside box_holds)   rdf, vhd, contacts;   check_pair_count, no_pairs_across_shards   these and sdf;   no_sums_across_shards   current, modes
// group[i] of every particle of the System (or, count >= 0, of `count` entries) against [-1, num_groups) (group = null: everything in group 0)
static int check_groups(vvhip_plan* p, const char* name, const signed char* group, int32_t num_groups, int32_t count = -1) {
    for (int32_t i = 0; group && i < (count < 0 ? p->hp.num_atoms : count); i++)
        if (group[i] < -1 || group[i] >= num_groups)
            return fail(p, VVHIP_ERR_INVALID, std::string(name) + ": group[" + std::to_string(i) + "] = " + std::to_string((int) group[i]) + " is outside [-1, num_groups = " + std::to_string(num_groups) + ")");
    return VVHIP_OK;
}
static int check_max_samples(vvhip_plan* p, const char* name, int64_t max_samples) {
    return max_samples < 1 ? fail(p, VVHIP_ERR_INVALID, std::string(name) + ": max_samples must be >= 1") : VVHIP_OK;
}
// weight[i] of every particle of the System (current, modes)
static int check_weights(vvhip_plan* p, const char* name, const double* weight) {
    for (int32_t i = 0; i < p->hp.num_atoms; i++)
        if (!std::isfinite(weight[i])) return fail(p, VVHIP_ERR_INVALID, std::string(name) + ": weight[" + std::to_string(i) + "] is not finite");
    return VVHIP_OK;
}
// The lag schedule: a sample every `interval` steps, lags 0 .. num_lags - 1 of them, every origin_every-th sample an origin.  min_lags = 0
// (density modes): no lags, no origins, the equal-time table alone.  (max_samples is checked behind the recorder's group and class counts.)
static int check_lags(vvhip_plan* p, const char* name, int32_t interval, int32_t num_lags, int32_t origin_every, int min_lags = 1) {
    const std::string n(name);
    if (interval < 1) return fail(p, VVHIP_ERR_INVALID, n + ": interval must be >= 1 step");
    if (num_lags < min_lags || num_lags > 4096) return fail(p, VVHIP_ERR_INVALID, n + ": num_lags must be in [" + std::to_string(min_lags) + ", 4096]");
    if (origin_every < 1 || origin_every > std::max(1, num_lags))
        return fail(p, VVHIP_ERR_INVALID, n + ": origin_every must be in " + (min_lags ? "[1, num_lags]" : "[1, max(1, num_lags)]"));
    return VVHIP_OK;
}
// ... its ring of ceil(num_lags / origin_every) slots, one per origin that is alive; the refusal of more than 1024 stands apart, because
// msd and acf refuse their fixed point in front of it
static int32_t num_origins_of(int32_t num_lags, int32_t origin_every) { return (num_lags + origin_every - 1) / origin_every; }
static int check_origins(vvhip_plan* p, const char* name, int32_t num_origins) {
    if (num_origins <= 1024) return VVHIP_OK;
    return fail(p, VVHIP_ERR_INVALID, std::string(name) + ": num_origins = ceil(num_lags / origin_every) = " + std::to_string(num_origins) + " is above 1024: raise origin_every");
}
// ---- units (msd, acf): the particles, or the molecules' massive members, of the description and of this shard.  A unit belongs to the
// plan when all of it lies in the shard, and its tables hold SHARD-RELATIVE particle indices (sites_by_group below: global ones).
struct Unit { int group; int32_t id; };          // id: the particle, the molecule, or (acf) the pair
struct PlanUnits {
    std::vector<Unit> units;                      // of this plan
    long long described = 0;                      // U: the units the DESCRIPTION records, of the whole System -- the fixed point follows these, not the shard
    std::vector<std::vector<int32_t>> members;    // molecules: per molecule id its massive particles, ascending
    bool cut = false;                             // the shard holds a part of some molecule (one that no group records too)
};
static int plan_units(vvhip_plan* p, const char* name, const signed char* group, bool molecules, PlanUnits& U) {
    const vv::HostPlan& hp = p->hp;
    auto group_of = [&](int32_t i) { return group ? (int) group[i] : 0; };
    auto in_shard = [&](int32_t i) { return i >= hp.shard_begin && i < hp.shard_end; };
    if (!molecules) {
        for (int32_t i = 0; i < hp.num_atoms; i++) {
            if (group_of(i) < 0) continue;
            U.described++;
            if (in_shard(i)) U.units.push_back({group_of(i), i});
        }
        return VVHIP_OK;
    }
    int32_t nmol = 0;
    for (int32_t i = 0; i < hp.num_atoms; i++) nmol = std::max(nmol, hp.mol_id[(size_t) i] + 1);
    U.members.resize((size_t) nmol);
    for (int32_t i = 0; i < hp.num_atoms; i++)
        if (hp.masses[(size_t) i] > 0) U.members[(size_t) hp.mol_id[(size_t) i]].push_back(i);
    for (int32_t m = 0; m < nmol; m++) {
        const std::vector<int32_t>& mem = U.members[(size_t) m];
        if (mem.empty()) continue;
        int here = 0;
        for (int32_t i : mem) {
            here += in_shard(i);
            if (group_of(i) != group_of(mem[0]))
                return fail(p, VVHIP_ERR_INVALID, std::string(name) + ": molecule " + std::to_string(m) + " has massive particles in different groups (particle " + std::to_string(mem[0]) + ": " +
                                                  std::to_string(group_of(mem[0])) + ", particle " + std::to_string(i) + ": " + std::to_string(group_of(i)) + ")");
        }
        U.cut = U.cut || (here != 0 && here != (int) mem.size());
        if (group_of(mem[0]) < 0) continue;
        U.described++;
        if (here == (int) mem.size()) U.units.push_back({group_of(mem[0]), m});
    }
    return VVHIP_OK;
}
// The fixed point of sums over the described units and the origins that max_samples samples store, of products below limit^2: at most 40
// fraction bits, refused below 8
static int units_frac_bits(vvhip_plan* p, const char* name, long long described, int64_t max_samples, int32_t origin_every, double limit, int32_t* frac_bits) {
    const long long max_origins = samples_plus(max_samples, origin_every - 1) / origin_every;
    *frac_bits = std::min(40, 62 - ceil_log2(described + 1) - ceil_log2(max_origins + 1) - 2 * std::ilogb(limit));
    if (*frac_bits >= 8) return VVHIP_OK;
    return fail(p, VVHIP_ERR_INVALID, std::string(name) + ": the sums would keep " + std::to_string(*frac_bits) + " fraction bits (< 8) with " + std::to_string(described) + " units, max_samples = " +
                                      std::to_string((long long) max_samples) + ", origin_every = " + std::to_string(origin_every) + " and limit " + std::to_string(limit) +
                                      ": lower max_samples or the limit");
}
// The units' tables, by group, then by id: index, and for molecules (N.molecules) first / weight / total; `pairs` (acf's orientation
// mode): head and tail of unit u instead
template <class R>
static void fill_units(const vv::HostPlan& hp, R& N, PlanUnits& U, const int32_t* pairs = nullptr) {
    std::stable_sort(U.units.begin(), U.units.end(), [](const Unit& x, const Unit& y) { return x.group < y.group; });
    for (const Unit& u : U.units) {
        if (N.grouped) N.group.push_back((unsigned char) u.group);
        if (pairs) { N.index.push_back(pairs[2 * u.id] - hp.shard_begin); N.index.push_back(pairs[2 * u.id + 1] - hp.shard_begin); continue; }
        if (!N.molecules) { N.index.push_back(u.id - hp.shard_begin); continue; }
        N.first.push_back((int32_t) N.index.size());
        double M = 0;
        for (int32_t i : U.members[(size_t) u.id]) {
            N.index.push_back(i - hp.shard_begin); N.weight.push_back(hp.masses[(size_t) i]);
            M = M + hp.masses[(size_t) i];
        }
        N.total.push_back(M);
    }
    if (N.molecules) N.first.push_back((int32_t) N.index.size());
    if (!N.molecules && !pairs && !N.grouped && (int32_t) U.units.size() == hp.shard_end - hp.shard_begin) N.index.clear();      // (every particle of the shard, in order: the thread's own index)
}
// ---- sites ordered by group (rdf, contacts, modes, current): every particle of the System with a group >= 0, by its GLOBAL index --
// these four record on unsharded plans only (no_pairs_ / no_sums_across_shards), where units hold shard-relative ones.  count[g] sites
// of group g from first[g] on; beside index, where asked for, the site's molecule, weight (and the largest |weight|) and group.
constexpr int kMaxSiteGroups = 16;
static_assert(vv::RDF_MAX_GROUPS <= kMaxSiteGroups && vv::CONTACTS_MAX_GROUPS <= kMaxSiteGroups && vv::CUR_MAX_GROUPS <= kMaxSiteGroups && vv::MODES_MAX_GROUPS <= kMaxSiteGroups, "");
struct Sites {
    int32_t count[kMaxSiteGroups] = {0}, first[kMaxSiteGroups + 1] = {0};
    std::vector<int32_t> index, mol;
    std::vector<double> weight;
    std::vector<unsigned char> group;
    double wmax = 0;
};
static Sites sites_by_group(const vv::HostPlan& hp, const signed char* group, int num_groups, bool with_mol, const double* weight, bool with_group) {
    Sites S;
    auto group_of = [&](int32_t i) { return group ? (int) group[i] : 0; };
    for (int32_t i = 0; i < hp.num_atoms; i++)
        if (group_of(i) >= 0) S.count[group_of(i)]++;
    for (int g = 0; g < num_groups; g++) S.first[g + 1] = S.first[g] + S.count[g];
    const size_t n = (size_t) S.first[num_groups];
    S.index.resize(n);
    if (with_mol) S.mol.resize(n);
    if (weight) S.weight.resize(n);
    if (with_group) S.group.resize(n);
    int32_t next[kMaxSiteGroups];
    std::copy(S.first, S.first + kMaxSiteGroups, next);
    for (int32_t i = 0; i < hp.num_atoms; i++) {      // ascending by particle inside every group
        const int g = group_of(i);
        if (g < 0) continue;
        const size_t s = (size_t) next[g]++;
        S.index[s] = i;
        if (with_mol) S.mol[s] = hp.mol_id[(size_t) i];
        if (weight) { S.weight[s] = weight[i]; S.wmax = std::max(S.wmax, std::fabs(weight[i])); }
        if (with_group) S.group[s] = (unsigned char) g;
    }
    return S;
}
// ---- classes of pairs of groups (rdf, contacts)
static int check_classes(vvhip_plan* p, const char* name, const int32_t* classes, int32_t num_classes, int32_t num_groups) {
    for (int32_t c = 0; c < num_classes; c++)
        for (int q = 0; q < 2; q++)
            if (classes[2 * c + q] < 0 || classes[2 * c + q] >= num_groups)
                return fail(p, VVHIP_ERR_INVALID, std::string(name) + ": classes[" + std::to_string(c) + "][" + std::to_string(q) + "] = " + std::to_string(classes[2 * c + q]) + " is outside [0, num_groups = " + std::to_string(num_groups) + ")");
    return VVHIP_OK;
}
// `pairs`: the most pairs a sample adds to one `word` ("bin", "word") of the table
static int check_pair_count(vvhip_plan* p, const char* name, int64_t pairs, int64_t max_samples, const char* word) {
    if ((unsigned __int128) pairs * (unsigned __int128) max_samples < ((unsigned __int128) 1 << 62)) return VVHIP_OK;
    return fail(p, VVHIP_ERR_INVALID, std::string(name) + ": " + std::to_string((long long) pairs) + " pairs per sample times max_samples = " + std::to_string((long long) max_samples) +
                                      " reaches 2^62: a " + word + " could overflow; lower max_samples");
}
// ---- a sharded plan: the two families' refusals (`table`: "histogram", "matrix")
static int no_pairs_across_shards(vvhip_plan* p, const char* name, const char* table) {
    if (!cmm_sharded(p)) return VVHIP_OK;
    return fail(p, VVHIP_ERR_UNSUPPORTED, std::string(name) + ": a sharded plan holds its own particles' positions only, so the pairs across shards exist on no device; "
                                          "a partial " + table + " is not recorded (run the analysis on an unsharded plan)");
}
static int no_sums_across_shards(vvhip_plan* p, const char* name) {
    if (!cmm_sharded(p)) return VVHIP_OK;
    return fail(p, VVHIP_ERR_UNSUPPORTED, std::string(name) + ": a sharded plan holds its own particles only: the shards' sums would have to be combined before the products "
                                          "are formed (an exchange of the sums is not implemented); record on an unsharded plan");
}

extern "C" {

int vvhip_drude_report_dof(const vvhip_plan* p, double dof[3]) {
    if (!p || !dof) return VVHIP_ERR_INVALID;
    for (int g = 0; g < 3; g++) dof[g] = p->hp.report_dof[g];
    return VVHIP_OK;
}
int vvhip_drude_report_raw(vvhip_plan* p, int64_t raw[6]) {
    NEED_BOUND(p);
    if (!raw) return VVHIP_ERR_INVALID;
    const vv::HostPlan& hp = p->hp;
    if (!hp.report_unsupported.empty()) return fail(p, VVHIP_ERR_UNSUPPORTED, "Drude temperature report: " + hp.report_unsupported);
    TRY(quiesce(p, "Drude temperature report", false, false));
    const int nmol = (int) hp.report_mol_mass.size();
    HIP_TRY(p, hipMemsetAsync(p->d_rep.get(), 0, (8 + 6 * (size_t) nmol) * sizeof(long long), p->stream));
    HIP_TRY(p, vv::launch_report(hp.precision, report_args(p, p->d_rep.get()), p->block_threads, p->grid_cap_a, p->stream));
    HIP_TRY(p, hipMemcpyAsync(p->h_rep.get(), p->d_rep.get(), vv::REP_WORDS * sizeof(long long), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    if (p->h_rep[vv::REP_FLAG])
        return fail(p, VVHIP_ERR_OVERFLOW, "Drude temperature report: a kinetic-energy or momentum term is NaN or beyond the fixed-point range; no numbers");
    std::memcpy(raw, p->h_rep.get(), 6 * sizeof(int64_t));
    return VVHIP_OK;
}
int vvhip_drude_report_combine(const vvhip_plan* p, const int64_t raw[6], double ke[3], double t[3]) {
    if (!p || !raw) return VVHIP_ERR_INVALID;
    const int F = p->hp.report_frac_bits, U = p->hp.report_unit_bits;
    auto join = [F, U](int64_t hi, int64_t lo) {        // (hi + lo 2^-F) 2^-U with the carry of lo (of either sign) moved into hi first
        const int64_t carry = lo >> F;                  // (arithmetic shift: floor)
        return (double) (hi + carry) * std::ldexp(1.0, -U) + (double) (lo - carry * ((int64_t) 1 << F)) * std::ldexp(1.0, -U - F);
    };
    const int T = vv::REP_TOTAL, D = vv::REP_DRUDE, M = vv::REP_COM;
    const double two_ke[3] = {join(raw[M], raw[M + 1]),
                              join(raw[T] - raw[M] - raw[D], raw[T + 1] - raw[M + 1] - raw[D + 1]),      // KE_Atom = KE_total - KE_COM - KE_Drude
                              join(raw[D], raw[D + 1])};
    constexpr double R = 8.31446261815324e-3;
    for (int g = 0; g < 3; g++) {
        const double k = 0.5 * two_ke[g], dof = p->hp.report_dof[g];
        if (ke) ke[g] = k;
        if (t) t[g] = dof > 0 ? 2 * k / (dof * R) : 0.0;
    }
    return VVHIP_OK;
}
int vvhip_drude_temperatures(vvhip_plan* p, double ke[3], double t[3]) {
    int64_t raw[6];
    TRY(vvhip_drude_report_raw(p, raw));
    return vvhip_drude_report_combine(p, raw, ke, t);
}

int vvhip_cm_motion_start(vvhip_plan* p, int32_t frequency) {
    if (!p) return VVHIP_ERR_INVALID;
    if (frequency < 1) return fail(p, VVHIP_ERR_INVALID, "centre-of-mass motion: frequency must be >= 1 step");
    if (!p->hp.has_cm_motion_remover)
        return fail(p, VVHIP_ERR_INVALID, "centre-of-mass motion: the plan was described without a CMMotionRemover (has_cm_motion_remover = 0), so the thermostat's "
                                          "degrees of freedom (DOF) still count the 3 of the centre of mass; describe the System with the remover to schedule removals");
    if (cmm_sharded(p)) return fail(p, VVHIP_ERR_UNSUPPORTED, kCmmSharded);
    NEED_BOUND(p);
    TRY(quiesce(p, "centre-of-mass motion", true, true));
    TRY(cmm_ensure(p));
    HIP_TRY(p, hipMemsetAsync(p->cmm.d_rec.get(), 0, sizeof(vv::CmmDevRecord), p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    p->cmm.on = true; p->cmm.when = {frequency, SCHEDULE_LINEAR};
    return VVHIP_OK;
}
int vvhip_cm_motion_stop(vvhip_plan* p) {
    if (!p) return VVHIP_ERR_INVALID;
    if (p->capturing || p->cmm.on) TRY(quiesce(p, "centre-of-mass motion", true, true));      // (nothing to settle for a schedule that is off)
    p->cmm.on = false; p->cmm.when = Schedule{};
    return VVHIP_OK;
}
int vvhip_remove_cm_motion(vvhip_plan* p, double v_removed[3]) {
    if (!p) return VVHIP_ERR_INVALID;
    if (cmm_sharded(p)) return fail(p, VVHIP_ERR_UNSUPPORTED, kCmmSharded);
    NEED_BOUND(p);
    TRY(quiesce(p, "centre-of-mass motion", false, false));
    TRY(cmm_ensure(p));
    return cmm_one_off(p, v_removed);
}
int vvhip_cm_motion_read(vvhip_plan* p, vvhip_cm_motion_record* out) {
    if (!p || !out) return VVHIP_ERR_INVALID;
    vvhip_cm_motion_record r{};
    r.frequency = p->cmm.on ? p->cmm.when.interval : 0;
    r.total_mass = p->hp.cm_total_mass;
    if (p->bound && p->cmm.d_rec) {
        TRY(quiesce(p, "centre-of-mass motion", true, false));
        vv::CmmDevRecord d{};
        HIP_TRY(p, hipMemcpy(&d, p->cmm.d_rec.get(), sizeof(d), hipMemcpyDeviceToHost));
        r.removals = d.removals; r.skipped = d.skipped;
        for (int k = 0; k < 3; k++) r.last_v[k] = d.last_v[k];
    }
    *out = r;
    if (r.skipped > 0)
        return fail(p, VVHIP_ERR_OVERFLOW, "centre-of-mass motion: " + std::to_string((long long) r.skipped) + " scheduled removal(s) skipped: a momentum term was NaN or beyond the fixed-point range");
    return VVHIP_OK;
}
// ------------------------------------------------------------------------------------------ Maxwell-Boltzmann start velocities
int vvhip_set_velocities_to_temperature(vvhip_plan* p, double temperature, double drude_temperature, uint64_t seed, uint32_t flags,
                                        vvhip_thermalize_record* out) {
    if (!p) return VVHIP_ERR_INVALID;
    if (!(temperature >= 0) || !std::isfinite(temperature))
        return fail(p, VVHIP_ERR_INVALID, "start velocities: the temperature must be finite and >= 0 K");
    if (std::isnan(drude_temperature) || (drude_temperature >= 0 && !std::isfinite(drude_temperature)))
        return fail(p, VVHIP_ERR_INVALID, "start velocities: the Drude temperature must be finite (>= 0 K), or negative for the plain draw");
    if (flags & ~(uint32_t) (VVHIP_THERMALIZE_NO_CONSTRAINTS | VVHIP_THERMALIZE_REMOVE_CM))
        return fail(p, VVHIP_ERR_INVALID, "start velocities: unknown flag bits");
    const bool remove_cm = (flags & VVHIP_THERMALIZE_REMOVE_CM) != 0;
    if (remove_cm && cmm_sharded(p)) return fail(p, VVHIP_ERR_UNSUPPORTED, kCmmSharded);
    NEED_BOUND(p);
    // (the library's own captures, and a host that is capturing the plan's stream itself: the call has to block for its record)
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (p->capturing || (hipStreamIsCapturing(p->stream, &capture) == hipSuccess && capture != hipStreamCaptureStatusNone))
        return fail(p, VVHIP_ERR_INVALID, "start velocities: not inside a graph capture");
    TRY(settle_recovery(p));
    const vv::HostPlan& hp = p->hp;
    if (!p->d_therm_laneless) HIP_TRY(p, vv::upload(p->d_therm_laneless, hp.therm_laneless, 16));
    if (remove_cm) TRY(cmm_ensure(p));
    constexpr double R = 8.31446261815324e-3;
    vv::ThermalizeArgs a{};
    a.velm = p->buf.velm; a.slots = p->d_slots.get(); a.lane_mass = p->d_rep_lane_mass.get();
    a.laneless = p->d_therm_laneless.get(); a.nwaves = hp.info.num_waves; a.nlaneless = (int32_t) hp.therm_laneless.size();
    a.shard_begin = hp.shard_begin; a.drude_aware = drude_temperature >= 0 ? 1 : 0;
    a.key[0] = (uint32_t) seed; a.key[1] = (uint32_t) (seed >> 32);
    a.kt = R * temperature; a.kt_drude = a.drude_aware ? R * drude_temperature : 0.0;
    HIP_TRY(p, vv::launch_thermalize(hp.precision, a, p->grid_cap_a, p->stream));
    vvhip_thermalize_record r{};
    r.drawn = hp.therm_massive; r.zeroed = hp.therm_massless; r.pairs_split = a.drude_aware ? hp.therm_pairs : 0;
    // OpenMM's applyVelocityConstraints after the draw: kernel A with the plan's constraint stages and nothing else
    if (!(flags & VVHIP_THERMALIZE_NO_CONSTRAINTS) && hp.info.constraints_fused && cons_a(p) != 0) {
        TRY(run_a(p, cons_a(p), 0));
        r.constrained = 1;
    }
    TRY(origins_dead(p, Rewrote::VELOCITIES));
    if (remove_cm) {      // (either way the call's one synchronisation)
        TRY(cmm_one_off(p, r.v_removed));
        r.cm_removed = 1;
    } else HIP_TRY(p, hipStreamSynchronize(p->stream));
    if (out) *out = r;
    return VVHIP_OK;
}
int vvhip_series_start(vvhip_plan* p, int32_t interval, int32_t capacity, int32_t mask) {
    if (!p) return VVHIP_ERR_INVALID;
    if (interval < 1) return fail(p, VVHIP_ERR_INVALID, "series: interval must be >= 1 step");
    if (capacity < 1) return fail(p, VVHIP_ERR_INVALID, "series: capacity must be >= 1 row");
    if (mask == 0 || (mask & ~(VVHIP_SERIES_DRUDE | VVHIP_SERIES_THERMOSTAT)))
        return fail(p, VVHIP_ERR_INVALID, "series: mask must be a non-empty set of VVHIP_SERIES_DRUDE / VVHIP_SERIES_THERMOSTAT");
    if ((mask & VVHIP_SERIES_DRUDE) && !p->hp.report_unsupported.empty())
        return fail(p, VVHIP_ERR_UNSUPPORTED, "Drude temperature report: " + p->hp.report_unsupported);
    NEED_BOUND(p);
    TRY(quiesce(p, "series", true, true));
    p->series = vvhip_plan::Series{};
    vvhip_plan::Series& S = p->series;
    size_t asked = 0;
    HIP_TRY(p, S.ring.alloc(sizeof(vvhip_series_row), capacity, p->stream, &asked));
    HIP_TRY(p, vv::zeros(S.d_scratch, (8 + 6 * p->hp.report_mol_mass.size()) * sizeof(long long), p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    S.on = true; S.when = {interval, SCHEDULE_LINEAR}; S.mask = mask;
    S.k0 = p->cur.step_count / interval + 1;               // the first multiple of interval after the current step
    return VVHIP_OK;
}
int vvhip_series_read(vvhip_plan* p, vvhip_series_row* rows_out, int32_t max_rows, int32_t* n_rows, int64_t* first_step, int64_t* dropped,
                      int32_t reset) {
    NEED_BOUND(p);
    if (max_rows < 0 || (max_rows > 0 && !rows_out)) return VVHIP_ERR_INVALID;
    vvhip_plan::Series& S = p->series;
    if (!S.on) return fail(p, VVHIP_ERR_INVALID, "series: none started (vvhip_series_start)");
    TRY(quiesce(p, "series", true, false));
    Ring::Count c;
    HIP_TRY(p, S.ring.fetch(&c));
    HIP_TRY(p, S.ring.copy_out(rows_out, std::min<long long>(c.stored, max_rows)));
    if (n_rows) *n_rows = (int32_t) c.stored;
    if (first_step) *first_step = (int64_t) S.when.interval * S.k0;
    if (dropped) *dropped = (int64_t) c.dropped;
    if (reset) {
        HIP_TRY(p, S.ring.reset_cursor(p->stream));
        S.k0 += c.counted;                              // (dropped rows included: their steps are gone)
    }
    return VVHIP_OK;
}
int vvhip_series_stop(vvhip_plan* p) { return recorder_stop(p, &vvhip_plan::series, "series"); }
int vvhip_series_info(const vvhip_plan* p, vvhip_series_layout* out) {
    if (!p || !out) return VVHIP_ERR_INVALID;
    vvhip_series_layout r{};
    r.row_bytes = (int32_t) sizeof(vvhip_series_row);
    r.off_drude_raw = (int32_t) offsetof(vvhip_series_row, drude_raw);
    r.off_nh = (int32_t) offsetof(vvhip_series_row, nh);
    r.off_box = (int32_t) offsetof(vvhip_series_row, box);
    r.active = p->series.on; r.interval = p->series.when.interval; r.capacity = p->series.ring.capacity; r.mask = p->series.mask;
    r.steps = p->cur.step_count;
    r.graph_captures = p->graph_captures;
    *out = r;
    return VVHIP_OK;
}

int vvhip_frames_schedule(int32_t interval, int32_t schedule, int64_t after_step, int32_t n, int64_t* steps_out) {
    if (interval < 1 || (schedule != VVHIP_FRAMES_LINEAR && schedule != VVHIP_FRAMES_LOG10) || after_step < 0 || n < 0 || (n > 0 && !steps_out))
        return VVHIP_ERR_INVALID;
    long long s = after_step;
    for (int32_t j = 0; j < n; j++) {
        if (s >= (1ll << 61)) return VVHIP_ERR_INVALID;      // (the logarithmic schedule grows tenfold every nine frames: no step beyond 2^62)
        steps_out[j] = s = next_due({interval, schedule}, s);
    }
    return VVHIP_OK;
}
int vvhip_frames_start(vvhip_plan* p, const vvhip_frames_desc* d) {
    if (!p) return VVHIP_ERR_INVALID;
    if (!d) return fail(p, VVHIP_ERR_INVALID, "frames: null description");
    if (d->interval < 1) return fail(p, VVHIP_ERR_INVALID, "frames: interval must be >= 1 step");
    if (d->capacity < 1) return fail(p, VVHIP_ERR_INVALID, "frames: capacity must be >= 1 frame");
    constexpr int kAll = VVHIP_FRAMES_POSITIONS | VVHIP_FRAMES_VELOCITIES | VVHIP_FRAMES_FLOAT64;
    if (!(d->mask & (VVHIP_FRAMES_POSITIONS | VVHIP_FRAMES_VELOCITIES)) || (d->mask & ~kAll))
        return fail(p, VVHIP_ERR_INVALID, "frames: mask must hold VVHIP_FRAMES_POSITIONS and / or VVHIP_FRAMES_VELOCITIES, and besides them VVHIP_FRAMES_FLOAT64 only");
    if (d->schedule != VVHIP_FRAMES_LINEAR && d->schedule != VVHIP_FRAMES_LOG10)
        return fail(p, VVHIP_ERR_INVALID, "frames: schedule must be VVHIP_FRAMES_LINEAR or VVHIP_FRAMES_LOG10");
    const vv::HostPlan& hp = p->hp;
    const bool has_subset = d->subset != nullptr || d->num_subset != 0;
    if (d->num_subset < 0 || (d->num_subset > 0 && !d->subset) || (d->subset && d->num_subset == 0))
        return fail(p, VVHIP_ERR_INVALID, "frames: subset and num_subset must both be given (or NULL / 0 for every particle)");
    for (int32_t j = 0; j < d->num_subset; j++) {
        if (d->subset[j] < 0 || d->subset[j] >= hp.num_atoms)
            return fail(p, VVHIP_ERR_INVALID, "frames: subset[" + std::to_string(j) + "] = " + std::to_string(d->subset[j]) + " is outside [0, num_atoms = " + std::to_string(hp.num_atoms) + ")");
        if (j > 0 && d->subset[j] <= d->subset[j - 1])
            return fail(p, VVHIP_ERR_INVALID, "frames: subset must be strictly ascending (subset[" + std::to_string(j) + "] = " + std::to_string(d->subset[j]) + " follows " + std::to_string(d->subset[j - 1]) + ")");
    }
    // ---- a recorder that runs is settled and goes first (its frames may still be in flight); then the description, host only
    TRY(recorder_stop(p, &vvhip_plan::frames, "frames"));
    vvhip_plan::Frames& F = p->frames;
    F.when = {d->interval, d->schedule}; F.capacity = d->capacity; F.mask = d->mask; F.has_subset = has_subset;
    if (has_subset) {
        const int32_t* lo = std::lower_bound(d->subset, d->subset + d->num_subset, hp.shard_begin);
        const int32_t* hi = std::lower_bound(lo, d->subset + d->num_subset, hp.shard_end);
        F.particles.assign(lo, hi);
        F.num_particles = (int) F.particles.size();
    } else {
        F.num_particles = hp.shard_end - hp.shard_begin;
    }
    F.component_bytes = (d->mask & VVHIP_FRAMES_FLOAT64) ? 8 : 4;
    F.plane_stride = (F.num_particles + 15) / 16 * 16;
    const long long quantity = 3ll * F.plane_stride * F.component_bytes;
    long long off = (long long) sizeof(vvhip_frame_header);
    if (d->mask & VVHIP_FRAMES_POSITIONS) { F.off_positions = off; off += quantity; }
    if (d->mask & VVHIP_FRAMES_VELOCITIES) { F.off_velocities = off; off += quantity; }
    F.frame_bytes = off;
    F.start_step = F.origin = p->cur.step_count;
    F.described = true;
    NEED_BOUND(p);
    TRY(quiesce(p, "frames", true, true));
    auto alloc_fail = [&](hipError_t e, size_t bytes) {
        F.ring = Ring{}; F.d_subset.reset();
        (void) hipGetLastError();
        return fail(p, VVHIP_ERR_HIP, std::string("frames: allocating ") + std::to_string((unsigned long long) bytes) + " bytes failed: " + hipGetErrorString(e));
    };
    size_t asked = 0;
    hipError_t e = F.ring.alloc((size_t) F.frame_bytes, F.capacity, p->stream, &asked);
    if (e != hipSuccess) return alloc_fail(e, asked);
    if (has_subset) {
        std::vector<int32_t> local(F.particles);
        for (int32_t& k : local) k -= hp.shard_begin;
        e = vv::upload(F.d_subset, local, 16);
        if (e != hipSuccess) return alloc_fail(e, std::max<size_t>(16, local.size() * sizeof(int32_t)));
    }
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    F.start_step = F.origin = p->cur.step_count;            // (a settled recovery may have moved the counter)
    F.on = true;
    return VVHIP_OK;
}
int vvhip_frames_read(vvhip_plan* p, void* frames_out, int64_t* steps_out, int32_t max_frames, int32_t* n_frames, int64_t* dropped, int32_t reset) {
    NEED_BOUND(p);
    if (max_frames < 0 || (max_frames > 0 && (!frames_out || !steps_out))) return VVHIP_ERR_INVALID;
    vvhip_plan::Frames& F = p->frames;
    if (!F.on) return fail(p, VVHIP_ERR_INVALID, "frames: none started (vvhip_frames_start)");
    TRY(quiesce(p, "frames", true, false));
    Ring::Count c;
    HIP_TRY(p, F.ring.fetch(&c));
    const long long copy = std::min<long long>(c.stored, max_frames);
    HIP_TRY(p, F.ring.copy_out(frames_out, copy));
    long long s = F.origin;
    for (long long j = 0; j < c.counted; j++) {             // (dropped frames included: their steps are gone)
        s = next_due(F.when, s);
        if (j >= copy) continue;
        steps_out[j] = s;
        vvhip_frame_header h;
        std::memcpy(&h, (const char*) frames_out + (size_t) j * (size_t) F.frame_bytes, sizeof(h));
        if (h.ordinal != j)
            return fail(p, VVHIP_ERR_HIP, "frames: frame " + std::to_string(j) + " carries ordinal " + std::to_string((long long) h.ordinal) + " in its header: the device-side cursor and the buffer disagree");
    }
    if (n_frames) *n_frames = (int32_t) c.stored;
    if (dropped) *dropped = (int64_t) c.dropped;
    if (reset) {
        HIP_TRY(p, F.ring.reset_cursor(p->stream));
        F.origin = s;
    }
    return VVHIP_OK;
}
int vvhip_frames_stop(vvhip_plan* p) { return recorder_stop(p, &vvhip_plan::frames, "frames"); }
int vvhip_frames_info(const vvhip_plan* p, vvhip_frames_layout* out) {
    if (!p || !out) return VVHIP_ERR_INVALID;
    const vvhip_plan::Frames& F = p->frames;
    vvhip_frames_layout r{};
    r.off_positions = r.off_velocities = -1;
    if (F.described) {
        r.active = F.on; r.interval = F.when.interval; r.schedule = F.when.kind; r.capacity = F.capacity; r.mask = F.mask;
        r.num_particles = F.num_particles; r.component_bytes = F.component_bytes; r.plane_stride = F.plane_stride;
        r.frame_bytes = F.frame_bytes; r.off_positions = F.off_positions; r.off_velocities = F.off_velocities;
        r.start_step = F.start_step;
    }
    *out = r;
    return VVHIP_OK;
}
int vvhip_frames_particles(const vvhip_plan* p, int32_t* global_indices, int32_t capacity) {
    if (!p || capacity < 0 || (capacity > 0 && !global_indices)) return VVHIP_ERR_INVALID;
    const vvhip_plan::Frames& F = p->frames;
    if (!F.described) return VVHIP_ERR_INVALID;
    const int32_t n = std::min<int32_t>(capacity, F.num_particles);
    for (int32_t j = 0; j < n; j++) global_indices[j] = F.has_subset ? F.particles[j] : p->hp.shard_begin + j;
    return VVHIP_OK;
}

int vvhip_profile_start(vvhip_plan* p, const vvhip_profile_desc* d) {
    if (!p) return VVHIP_ERR_INVALID;
    if (!d) return fail(p, VVHIP_ERR_INVALID, "profile: null description");
    if (d->interval < 1) return fail(p, VVHIP_ERR_INVALID, "profile: interval must be >= 1 step");
    if (d->axis < 0 || d->axis > 2) return fail(p, VVHIP_ERR_INVALID, "profile: axis must be 0, 1 or 2");
    if (d->nbins < 1 || d->nbins > 65536) return fail(p, VVHIP_ERR_INVALID, "profile: nbins must be in [1, 65536]");
    constexpr int kAll = VVHIP_PROFILE_COUNT | VVHIP_PROFILE_CHARGE | VVHIP_PROFILE_MASS | VVHIP_PROFILE_MOMENTUM | VVHIP_PROFILE_KINETIC;
    if (d->mask & ~kAll) return fail(p, VVHIP_ERR_INVALID, "profile: mask holds bits besides VVHIP_PROFILE_COUNT / CHARGE / MASS / MOMENTUM / KINETIC");
    if (d->num_groups < 1 || d->num_groups > 16) return fail(p, VVHIP_ERR_INVALID, "profile: num_groups must be in [1, 16]");
    TRY(check_max_samples(p, "profile", d->max_samples));
    static const char* const kQuantity[VVHIP_PROFILE_QUANTITIES] = {"count", "charge", "mass", "momentum", "kinetic"};
    for (int q = 0; q < 4; q++)
        if (!(d->limit[q] >= 0) || !std::isfinite(d->limit[q]))
            return fail(p, VVHIP_ERR_INVALID, std::string("profile: limit[") + std::to_string(q) + "] (" + kQuantity[q + 1] + ") must be finite and >= 0 (0: the default)");
    const vv::HostPlan& hp = p->hp;
    TRY(check_groups(p, "profile", d->group, d->num_groups));
    // ---- the particles this plan records, the layout and the fixed point, host only
    vvhip_plan::Profile N;
    vvhip_profile_layout& L = N.lay;
    N.grouped = d->group != nullptr;
    // (the fixed point and the default limits follow the particles the DESCRIPTION records, of the whole System: every shard then scales
    // its terms alike, and the shards' words add to the unsharded table)
    double largest_mass = 0;
    long long described = 0;
    for (int32_t i = 0; i < hp.num_atoms; i++) {
        if (d->group && d->group[i] < 0) continue;
        described++;
        largest_mass = std::max(largest_mass, hp.masses[(size_t) i]);
        if (i < hp.shard_begin || i >= hp.shard_end) continue;
        N.index.push_back(i - hp.shard_begin);
        if (N.grouped) N.group.push_back((unsigned char) d->group[i]);
        N.mass.push_back(hp.masses[(size_t) i]);
    }
    L.interval = d->interval; L.axis = d->axis; L.nbins = d->nbins; L.mask = d->mask | VVHIP_PROFILE_COUNT; L.num_groups = d->num_groups;
    L.num_particles = (int32_t) N.index.size(); L.max_samples = d->max_samples;
    if (L.num_particles == hp.shard_end - hp.shard_begin) N.index.clear();      // (every particle of the shard: the thread's own index)
    const int rows_of[VVHIP_PROFILE_QUANTITIES] = {1, 1, 1, 3, 1};
    for (int q = 0; q < VVHIP_PROFILE_QUANTITIES; q++) {
        L.row_of[q] = (L.mask & (1 << q)) ? L.rows : -1;
        if (L.mask & (1 << q)) L.rows += rows_of[q];
    }
    L.words = (int64_t) L.num_groups * L.rows * L.nbins;
    const double mass_limit = d->limit[1] > 0 ? pow2_at_least(d->limit[1]) : (largest_mass > 0 ? pow2_above(largest_mass) : 1.0);
    L.limit[VVHIP_PROFILE_Q_COUNT] = 1.0;
    L.limit[VVHIP_PROFILE_Q_CHARGE] = d->limit[0] > 0 ? pow2_at_least(d->limit[0]) : 16.0;
    L.limit[VVHIP_PROFILE_Q_MASS] = mass_limit;
    L.limit[VVHIP_PROFILE_Q_MOMENTUM] = d->limit[2] > 0 ? pow2_at_least(d->limit[2]) : mass_limit * 64.0;
    L.limit[VVHIP_PROFILE_Q_KINETIC] = d->limit[3] > 0 ? pow2_at_least(d->limit[3]) : mass_limit * 4096.0;
    const int head = 62 - ceil_log2(described + 1) - ceil_log2(samples_plus(L.max_samples, 1));
    for (int q = 1; q < VVHIP_PROFILE_QUANTITIES; q++) {
        L.frac_bits[q] = std::min(40, head - std::ilogb(L.limit[q]));
        if ((L.mask & (1 << q)) && L.frac_bits[q] < 8)
            return fail(p, VVHIP_ERR_INVALID, std::string("profile: the ") + kQuantity[q] + " rows would keep " + std::to_string(L.frac_bits[q]) + " fraction bits (< 8) with " +
                                              std::to_string(L.num_particles) + " particles, max_samples = " + std::to_string((long long) L.max_samples) + " and limit " +
                                              std::to_string(L.limit[q]) + ": lower max_samples or the limit");
    }
    return recorder_install(p, &vvhip_plan::profile, "profile", N, d->interval);
}
int vvhip_profile_read(vvhip_plan* p, int64_t* words_out, int64_t capacity_words, vvhip_profile_counts* out, int32_t reset) {
    long long head[vv::PROFILE_HEAD];
    TRY(recorder_fetch(p, &vvhip_plan::profile, "profile", words_out, capacity_words, head));
    if (out) *out = {head[vv::PROFILE_SAMPLES], head[vv::PROFILE_DROPPED], head[vv::PROFILE_OUT_OF_RANGE]};
    return reset ? recorder_reset(p, p->profile) : VVHIP_OK;
}
int vvhip_profile_stop(vvhip_plan* p) { return recorder_stop(p, &vvhip_plan::profile, "profile"); }
int vvhip_profile_info(const vvhip_plan* p, vvhip_profile_layout* out) {
    vvhip_profile_layout blank{};
    for (int q = 0; q < VVHIP_PROFILE_QUANTITIES; q++) blank.row_of[q] = -1;
    return recorder_info(p, &vvhip_plan::profile, out, blank);
}

int vvhip_msd_start(vvhip_plan* p, const vvhip_msd_desc* d) {
    if (!p) return VVHIP_ERR_INVALID;
    if (!d) return fail(p, VVHIP_ERR_INVALID, "msd: null description");
    TRY(check_lags(p, "msd", d->interval, d->num_lags, d->origin_every));
    if (d->mode != VVHIP_MSD_PARTICLES && d->mode != VVHIP_MSD_MOLECULES) return fail(p, VVHIP_ERR_INVALID, "msd: mode must be VVHIP_MSD_PARTICLES or VVHIP_MSD_MOLECULES");
    if (d->num_groups < 1 || d->num_groups > 16) return fail(p, VVHIP_ERR_INVALID, "msd: num_groups must be in [1, 16]");
    TRY(check_max_samples(p, "msd", d->max_samples));
    if (!(d->limit >= 0) || !std::isfinite(d->limit)) return fail(p, VVHIP_ERR_INVALID, "msd: limit must be finite and >= 0 (0: the default of 64 nm)");
    TRY(check_groups(p, "msd", d->group, d->num_groups));
    // ---- the units this plan records, the layout and the fixed point, host only
    vvhip_plan::Msd N;
    vvhip_msd_layout& L = N.lay;
    N.grouped = d->group != nullptr; N.molecules = d->mode == VVHIP_MSD_MOLECULES;
    PlanUnits U;
    TRY(plan_units(p, "msd", d->group, N.molecules, U));
    L.interval = d->interval; L.num_lags = d->num_lags; L.origin_every = d->origin_every; L.mode = d->mode; L.num_groups = d->num_groups;
    L.max_samples = d->max_samples;
    L.num_units = (int32_t) U.units.size();
    L.num_origins = num_origins_of(d->num_lags, d->origin_every);
    L.words = (int64_t) L.num_groups * L.num_lags * 4;
    L.limit = d->limit > 0 ? pow2_at_least(d->limit) : 64.0;
    L.ring_bytes = (int64_t) L.num_origins * 3 * N.stride() * (int64_t) sizeof(double);
    TRY(units_frac_bits(p, "msd", U.described, L.max_samples, L.origin_every, L.limit, &L.frac_bits));
    TRY(check_origins(p, "msd", L.num_origins));
    if (N.molecules && U.cut)
        return fail(p, VVHIP_ERR_UNSUPPORTED, "msd: the particle shard cuts a molecule: its centre of mass needs particles of another shard");
    fill_units(p->hp, N, U);
    return recorder_install(p, &vvhip_plan::msd, "msd", N, d->interval);
}
int vvhip_msd_read(vvhip_plan* p, int64_t* words_out, int64_t capacity_words, vvhip_msd_counts* out, int32_t reset) {
    long long head[vv::MSD_HEAD];
    TRY(recorder_fetch(p, &vvhip_plan::msd, "msd", words_out, capacity_words, head));
    if (out) *out = {head[vv::MSD_SAMPLES], head[vv::MSD_DROPPED], head[vv::MSD_OUT_OF_RANGE], head[vv::MSD_FLOOR]};
    return reset ? recorder_reset(p, p->msd) : VVHIP_OK;
}
int vvhip_msd_stop(vvhip_plan* p) { return recorder_stop(p, &vvhip_plan::msd, "msd"); }
int vvhip_msd_info(const vvhip_plan* p, vvhip_msd_layout* out) { return recorder_info(p, &vvhip_plan::msd, out); }

int vvhip_vanhove_start(vvhip_plan* p, const vvhip_vanhove_desc* d) {
    if (!p) return VVHIP_ERR_INVALID;
    if (!d) return fail(p, VVHIP_ERR_INVALID, "vanhove: null description");
    TRY(check_lags(p, "vanhove", d->interval, d->num_lags, d->origin_every));
    if (d->mode != VVHIP_VANHOVE_PARTICLES && d->mode != VVHIP_VANHOVE_MOLECULES) return fail(p, VVHIP_ERR_INVALID, "vanhove: mode must be VVHIP_VANHOVE_PARTICLES or VVHIP_VANHOVE_MOLECULES");
    if (d->num_groups < 1 || d->num_groups > 16) return fail(p, VVHIP_ERR_INVALID, "vanhove: num_groups must be in [1, 16]");
    TRY(check_max_samples(p, "vanhove", d->max_samples));
    if (!(d->limit >= 0) || !std::isfinite(d->limit)) return fail(p, VVHIP_ERR_INVALID, "vanhove: limit must be finite and >= 0 (0: the default of 16 nm)");
    TRY(check_groups(p, "vanhove", d->group, d->num_groups));
    if (d->num_bins < 1 || d->num_bins > vv::VANHOVE_MAX_BINS) return fail(p, VVHIP_ERR_INVALID, "vanhove: num_bins must be in [1, 1024]");
    if (!d->edges) return fail(p, VVHIP_ERR_INVALID, "vanhove: edges is null (num_bins + 1 bin edges in nm)");
    for (int32_t k = 0; k <= d->num_bins; k++) {
        if (!std::isfinite(d->edges[k]) || d->edges[k] < 0) return fail(p, VVHIP_ERR_INVALID, "vanhove: edges[" + std::to_string(k) + "] must be finite and >= 0");
        if (k > 0 && !(d->edges[k] > d->edges[k - 1])) return fail(p, VVHIP_ERR_INVALID, "vanhove: edges must ascend strictly (edges[" + std::to_string(k) + "] <= edges[" + std::to_string(k - 1) + "])");
    }
    // ---- the units this plan records, the layout and the fixed point, host only
    vvhip_plan::VanHove N;
    vvhip_vanhove_layout& L = N.lay;
    N.grouped = d->group != nullptr; N.molecules = d->mode == VVHIP_VANHOVE_MOLECULES;
    PlanUnits U;
    TRY(plan_units(p, "vanhove", d->group, N.molecules, U));
    L.interval = d->interval; L.num_lags = d->num_lags; L.origin_every = d->origin_every; L.mode = d->mode; L.num_groups = d->num_groups;
    L.num_bins = d->num_bins; L.max_samples = d->max_samples;
    L.num_units = (int32_t) U.units.size();
    L.num_origins = num_origins_of(d->num_lags, d->origin_every);
    L.head_words = (int64_t) L.num_groups * L.num_lags * vv::VANHOVE_ROW;
    L.hist_words = (int64_t) L.num_groups * L.num_lags * L.num_bins;
    L.words = L.head_words + L.hist_words;
    L.limit = d->limit > 0 ? pow2_at_least(d->limit) : 16.0;
    L.ring_bytes = (int64_t) L.num_origins * 3 * N.stride() * (int64_t) sizeof(double);
    // (r2 < 3 limit^2 < 2^(2 log2(limit) + 2), r2 r2 < 9 limit^4 < 2^(4 log2(limit) + 4), summed over at most U units and the origins that
    // max_samples samples store; the low word of r2 r2 is at most 2^r4_lo_bits per pair)
    const long long max_origins = samples_plus(L.max_samples, L.origin_every - 1) / L.origin_every;
    const int sum_bits = ceil_log2(U.described + 1) + ceil_log2(max_origins + 1), limit_bits = std::ilogb(L.limit);
    L.frac2_bits = std::min(40, 62 - sum_bits - 2 * limit_bits - 2);
    L.r4_hi_bits = std::min(40, 62 - sum_bits - 4 * limit_bits - 4);
    L.r4_lo_bits = std::min(52, 61 - sum_bits);
    const std::string with = " with " + std::to_string(U.described) + " units, max_samples = " + std::to_string((long long) L.max_samples) + ", origin_every = " + std::to_string(L.origin_every) +
                             " and limit " + std::to_string(L.limit) + ": lower max_samples or the limit";
    if (L.frac2_bits < 8) return fail(p, VVHIP_ERR_INVALID, "vanhove: the sums of r2 would keep frac2_bits = " + std::to_string(L.frac2_bits) + " fraction bits (< 8)" + with);
    if (L.r4_hi_bits < 0) return fail(p, VVHIP_ERR_INVALID, "vanhove: the sums of r2 r2 would keep r4_hi_bits = " + std::to_string(L.r4_hi_bits) + " fraction bits (< 0)" + with);
    if (L.words > VVHIP_VANHOVE_MAX_WORDS)
        return fail(p, VVHIP_ERR_INVALID, "vanhove: the table would have " + std::to_string((long long) L.words) + " words (num_groups * num_lags * (6 + num_bins)), above the cap of " +
                                          std::to_string((long long) VVHIP_VANHOVE_MAX_WORDS) + " (32 MiB): fewer lags, bins or groups");
    TRY(check_origins(p, "vanhove", L.num_origins));
    if (N.molecules && U.cut)
        return fail(p, VVHIP_ERR_UNSUPPORTED, "vanhove: the particle shard cuts a molecule: its centre of mass needs particles of another shard");
    fill_units(p->hp, N, U);
    N.e2.resize((size_t) L.num_bins + 1);
    for (int32_t k = 0; k <= L.num_bins; k++) N.e2[(size_t) k] = d->edges[k] * d->edges[k];
    return recorder_install(p, &vvhip_plan::vanhove, "vanhove", N, d->interval);
}
int vvhip_vanhove_read(vvhip_plan* p, int64_t* words_out, int64_t capacity_words, vvhip_vanhove_counts* out, int32_t reset) {
    long long head[vv::VANHOVE_HEAD];
    TRY(recorder_fetch(p, &vvhip_plan::vanhove, "vanhove", words_out, capacity_words, head));
    if (out) *out = {head[vv::VANHOVE_SAMPLES], head[vv::VANHOVE_DROPPED], head[vv::VANHOVE_OUT_OF_RANGE], head[vv::VANHOVE_FLOOR]};
    return reset ? recorder_reset(p, p->vanhove) : VVHIP_OK;
}
int vvhip_vanhove_stop(vvhip_plan* p) { return recorder_stop(p, &vvhip_plan::vanhove, "vanhove"); }
int vvhip_vanhove_info(const vvhip_plan* p, vvhip_vanhove_layout* out) { return recorder_info(p, &vvhip_plan::vanhove, out); }

int vvhip_vanhove_distinct_start(vvhip_plan* p, const vvhip_vanhove_distinct_desc* d) {
    if (!p) return VVHIP_ERR_INVALID;
    if (!d) return fail(p, VVHIP_ERR_INVALID, "vanhove_distinct: null description");
    TRY(check_lags(p, "vanhove_distinct", d->interval, d->num_lags, d->origin_every));
    if (!(d->r_max > 0) || !std::isfinite(d->r_max)) return fail(p, VVHIP_ERR_INVALID, "vanhove_distinct: r_max must be finite and > 0");
    if (d->nbins < 1 || d->nbins > 8192) return fail(p, VVHIP_ERR_INVALID, "vanhove_distinct: nbins must be in [1, 8192]");
    if (d->num_groups < 1 || d->num_groups > vv::RDF_MAX_GROUPS) return fail(p, VVHIP_ERR_INVALID, "vanhove_distinct: num_groups must be in [1, 16]");
    if (d->num_classes < 1 || d->num_classes > vv::RDF_MAX_CLASSES) return fail(p, VVHIP_ERR_INVALID, "vanhove_distinct: num_classes must be in [1, 32]");
    if (!d->classes) return fail(p, VVHIP_ERR_INVALID, "vanhove_distinct: classes must not be NULL");
    TRY(check_max_samples(p, "vanhove_distinct", d->max_samples));
    TRY(check_groups(p, "vanhove_distinct", d->group, d->num_groups));
    TRY(check_classes(p, "vanhove_distinct", d->classes, d->num_classes, d->num_groups));
    // ---- the sites, the layout and the pair kernel's work list, host only
    vvhip_plan::Vhd N;
    vvhip_vanhove_distinct_layout& L = N.lay;
    L.interval = d->interval; L.num_lags = d->num_lags; L.origin_every = d->origin_every; L.nbins = d->nbins;
    L.num_groups = d->num_groups; L.num_classes = d->num_classes;
    L.exclude_same_molecule = d->exclude_same_molecule != 0; L.tile = vv::RDF_TILE;
    L.num_origins = num_origins_of(d->num_lags, d->origin_every); L.num_rows = d->num_lags + 1;
    L.max_samples = d->max_samples;
    L.head_words = (int64_t) L.num_rows * vv::VHD_ROW;
    L.hist_words = (int64_t) d->num_classes * L.num_rows * d->nbins;
    L.words = L.head_words + L.hist_words;
    L.r_max = d->r_max; L.dr = d->r_max / (double) d->nbins;
    if (L.words > VVHIP_VANHOVE_DISTINCT_MAX_WORDS)
        return fail(p, VVHIP_ERR_INVALID, "vanhove_distinct: the table would have " + std::to_string((long long) L.words) + " words ((num_lags + 1) * (2 + num_classes * nbins)), above the cap of " +
                                          std::to_string((long long) VVHIP_VANHOVE_DISTINCT_MAX_WORDS) + " (32 MiB): fewer lags, bins or classes");
    TRY(check_origins(p, "vanhove_distinct", L.num_origins));
    Sites S = sites_by_group(p->hp, d->group, d->num_groups, L.exclude_same_molecule != 0, nullptr, false);
    std::copy(S.count, S.count + d->num_groups, L.num_sites);
    const int32_t* first = S.first;
    int64_t largest = 0;
    for (int32_t c = 0; c < d->num_classes; c++) {
        const int ga = d->classes[2 * c], gb = d->classes[2 * c + 1];
        const int64_t na = L.num_sites[ga], nb = L.num_sites[gb];
        L.classes[c][0] = ga; L.classes[c][1] = gb;
        L.pairs_per_sample[c] = ga == gb ? na * (na - 1) : na * nb;
        largest = std::max(largest, L.pairs_per_sample[c]);
    }
    TRY(check_pair_count(p, "vanhove_distinct", largest, d->max_samples, "bin"));
    TRY(check_half_box(p, "vanhove_distinct", "r_max = ", d->r_max));
    TRY(no_pairs_across_shards(p, "vanhove_distinct", "histogram"));
    N.index = std::move(S.index); N.mol = std::move(S.mol);
    L.ring_bytes = (int64_t) (L.num_origins + 2) * 3 * N.stride() * (int64_t) sizeof(double);
    // the work list: per class and i-tile the j-sites in runs of `max_jsites`, a multiple of 64, as for the RDF -- but all j-sites for a
    // class of one group with itself too (the pairs are ordered).  Every item runs once per ring slot, so the target counts items, not blocks
    constexpr int T = vv::RDF_TILE;
    long long runs = 0;                                     // of 64 j-sites, over all i-tiles
    for (int32_t c = 0; c < d->num_classes; c++) {
        const int64_t na = L.num_sites[L.classes[c][0]], nb = L.num_sites[L.classes[c][1]];
        runs += (na + T - 1) / T * ((nb + 63) / 64);
    }
    const int target = std::max(1, p->vhd_items_target);
    N.max_jsites = 64 * (int) std::max<long long>(1, std::min<long long>(4096, (runs + target - 1) / target));
    for (int32_t c = 0; c < d->num_classes; c++) {
        const int ga = L.classes[c][0], gb = L.classes[c][1];
        const int32_t na = L.num_sites[ga], nb = L.num_sites[gb];
        if (ga == gb && na < 2) continue;                  // (no pair)
        for (int32_t i0 = 0; i0 < na; i0 += T)
            for (int32_t j0 = 0; j0 < nb; j0 += N.max_jsites)
                N.items.push_back({c, ga == gb ? 1 : 0, first[ga] + i0, std::min(T, na - i0), first[gb], j0, std::min(nb, j0 + N.max_jsites), 0});
    }
    L.num_items = (int32_t) N.items.size();
    return recorder_install(p, &vvhip_plan::vhd, "vanhove_distinct", N, d->interval);
}
int vvhip_vanhove_distinct_read(vvhip_plan* p, int64_t* words_out, int64_t capacity_words, vvhip_vanhove_distinct_counts* out, int32_t reset) {
    long long head[vv::VHD_HEAD];
    TRY(recorder_fetch(p, &vvhip_plan::vhd, "vanhove_distinct", words_out, capacity_words, head));
    if (out) *out = {head[vv::VHD_SAMPLES], head[vv::VHD_DROPPED], head[vv::VHD_INVALID], head[vv::VHD_FLOOR]};
    return reset ? recorder_reset(p, p->vhd) : VVHIP_OK;
}
int vvhip_vanhove_distinct_stop(vvhip_plan* p) { return recorder_stop(p, &vvhip_plan::vhd, "vanhove_distinct"); }
int vvhip_vanhove_distinct_info(const vvhip_plan* p, vvhip_vanhove_distinct_layout* out) { return recorder_info(p, &vvhip_plan::vhd, out); }

int vvhip_rdf_start(vvhip_plan* p, const vvhip_rdf_desc* d) {
    if (!p) return VVHIP_ERR_INVALID;
    if (!d) return fail(p, VVHIP_ERR_INVALID, "rdf: null description");
    if (d->interval < 1) return fail(p, VVHIP_ERR_INVALID, "rdf: interval must be >= 1 step");
    if (!(d->r_max > 0) || !std::isfinite(d->r_max)) return fail(p, VVHIP_ERR_INVALID, "rdf: r_max must be finite and > 0");
    if (d->nbins < 1 || d->nbins > 8192) return fail(p, VVHIP_ERR_INVALID, "rdf: nbins must be in [1, 8192]");
    if (d->num_groups < 1 || d->num_groups > vv::RDF_MAX_GROUPS) return fail(p, VVHIP_ERR_INVALID, "rdf: num_groups must be in [1, 16]");
    if (d->num_classes < 1 || d->num_classes > vv::RDF_MAX_CLASSES) return fail(p, VVHIP_ERR_INVALID, "rdf: num_classes must be in [1, 32]");
    if (!d->classes) return fail(p, VVHIP_ERR_INVALID, "rdf: classes must not be NULL");
    TRY(check_max_samples(p, "rdf", d->max_samples));
    TRY(check_groups(p, "rdf", d->group, d->num_groups));
    TRY(check_classes(p, "rdf", d->classes, d->num_classes, d->num_groups));
    // ---- the sites, the layout and the pair kernel's work list, host only
    vvhip_plan::Rdf N;
    vvhip_rdf_layout& L = N.lay;
    L.interval = d->interval; L.nbins = d->nbins; L.num_groups = d->num_groups; L.num_classes = d->num_classes;
    L.exclude_same_molecule = d->exclude_same_molecule != 0; L.tile = vv::RDF_TILE;
    L.max_samples = d->max_samples; L.words = (int64_t) d->num_classes * d->nbins;
    L.r_max = d->r_max; L.dr = d->r_max / (double) d->nbins;
    Sites S = sites_by_group(p->hp, d->group, d->num_groups, L.exclude_same_molecule != 0, nullptr, false);
    std::copy(S.count, S.count + d->num_groups, L.num_sites);
    const int32_t* first = S.first;
    int64_t largest = 0;
    for (int32_t c = 0; c < d->num_classes; c++) {
        const int ga = d->classes[2 * c], gb = d->classes[2 * c + 1];
        const int64_t na = L.num_sites[ga], nb = L.num_sites[gb];
        L.classes[c][0] = ga; L.classes[c][1] = gb;
        L.pairs_per_sample[c] = ga == gb ? na * (na - 1) / 2 : na * nb;
        largest = std::max(largest, L.pairs_per_sample[c]);
    }
    TRY(check_pair_count(p, "rdf", largest, d->max_samples, "bin"));
    TRY(check_half_box(p, "rdf", "r_max = ", d->r_max));
    TRY(no_pairs_across_shards(p, "rdf", "histogram"));
    N.index = std::move(S.index); N.mol = std::move(S.mol);
    // the work list: per class and i-tile the j-sites in runs of `max_jsites`, a multiple of 64; a class of one group with itself from
    // the i-tile's first site on.  A small workload gets runs of 64, so that its blocks fill the device; beyond rdf_items_target blocks
    // a run grows, so that the flush of a block's histogram and its launch are shared (at most 2^18 sites: 2^26 pairs, far inside what
    // a private 32-bit word holds)
    constexpr int T = vv::RDF_TILE;
    long long runs = 0;                                     // of 64 j-sites, over all i-tiles
    for (int32_t c = 0; c < d->num_classes; c++) {
        const int64_t na = L.num_sites[L.classes[c][0]], nb = L.num_sites[L.classes[c][1]];
        for (int64_t i0 = 0; i0 < na; i0 += T) runs += (nb - (L.classes[c][0] == L.classes[c][1] ? i0 : 0) + 63) / 64;
    }
    const int target = std::max(1, p->rdf_items_target);
    N.max_jsites = 64 * (int) std::max<long long>(1, std::min<long long>(4096, (runs + target - 1) / target));
    for (int32_t c = 0; c < d->num_classes; c++) {
        const int ga = L.classes[c][0], gb = L.classes[c][1];
        const int32_t na = L.num_sites[ga], nb = L.num_sites[gb];
        if (ga == gb && na < 2) continue;                  // (no pair)
        for (int32_t i0 = 0; i0 < na; i0 += T)
            for (int32_t j0 = ga == gb ? i0 : 0; j0 < nb; j0 += N.max_jsites)
                N.items.push_back({c, ga == gb ? 1 : 0, first[ga] + i0, std::min(T, na - i0), first[gb], j0, std::min(nb, j0 + N.max_jsites), 0});
    }
    L.num_items = (int32_t) N.items.size();
    L.scratch_bytes = (int64_t) 3 * N.stride() * (int64_t) sizeof(double);
    return recorder_install(p, &vvhip_plan::rdf, "rdf", N, d->interval);
}
int vvhip_rdf_sample(vvhip_plan* p) {
    NEED_BOUND(p);
    if (!p->rdf.on) return fail(p, VVHIP_ERR_INVALID, "rdf: none started (vvhip_rdf_start)");
    TRY(quiesce(p, "rdf", false, false));
    return rdf_enqueue(p);
}
int vvhip_rdf_read(vvhip_plan* p, int64_t* words_out, int64_t capacity_words, vvhip_rdf_counts* out, int32_t reset) {
    long long head[vv::RDF_HEAD];
    TRY(recorder_fetch(p, &vvhip_plan::rdf, "rdf", words_out, capacity_words, head));
    if (out) {
        double s;
        std::memcpy(&s, &head[vv::RDF_INV_VOLUME], sizeof s);
        *out = {head[vv::RDF_SAMPLES], head[vv::RDF_DROPPED], head[vv::RDF_INVALID], s};
    }
    return reset ? recorder_reset(p, p->rdf) : VVHIP_OK;
}
int vvhip_rdf_stop(vvhip_plan* p) { return recorder_stop(p, &vvhip_plan::rdf, "rdf"); }
int vvhip_rdf_info(const vvhip_plan* p, vvhip_rdf_layout* out) { return recorder_info(p, &vvhip_plan::rdf, out); }

int vvhip_sdf_start(vvhip_plan* p, const vvhip_sdf_desc* d) {
    if (!p) return VVHIP_ERR_INVALID;
    if (!d) return fail(p, VVHIP_ERR_INVALID, "sdf: null description");
    if (d->interval < 1) return fail(p, VVHIP_ERR_INVALID, "sdf: interval must be >= 1 step");
    if (!(d->extent > 0) || !std::isfinite(d->extent)) return fail(p, VVHIP_ERR_INVALID, "sdf: extent must be finite and > 0");
    if (d->nbins < 1 || d->nbins > vv::SDF_MAX_BINS) return fail(p, VVHIP_ERR_INVALID, "sdf: nbins must be in [1, 128]");
    if (d->num_frames < 0) return fail(p, VVHIP_ERR_INVALID, "sdf: num_frames must be >= 0");
    if (d->num_frame_groups < 1 || d->num_frame_groups > vv::SDF_MAX_GROUPS) return fail(p, VVHIP_ERR_INVALID, "sdf: num_frame_groups must be in [1, 16]");
    if (d->num_site_groups < 1 || d->num_site_groups > vv::SDF_MAX_GROUPS) return fail(p, VVHIP_ERR_INVALID, "sdf: num_site_groups must be in [1, 16]");
    if (d->num_classes < 1 || d->num_classes > vv::SDF_MAX_CLASSES) return fail(p, VVHIP_ERR_INVALID, "sdf: num_classes must be in [1, 16]");
    if (!d->classes) return fail(p, VVHIP_ERR_INVALID, "sdf: classes must not be NULL");
    if (!d->frames && d->num_frames > 0) return fail(p, VVHIP_ERR_INVALID, "sdf: frames must not be NULL with num_frames > 0");
    TRY(check_max_samples(p, "sdf", d->max_samples));
    for (int32_t f = 0; d->frame_group && f < d->num_frames; f++)
        if (d->frame_group[f] < -1 || d->frame_group[f] >= d->num_frame_groups)
            return fail(p, VVHIP_ERR_INVALID, "sdf: frame_group[" + std::to_string(f) + "] = " + std::to_string((int) d->frame_group[f]) + " is outside [-1, num_frame_groups = " + std::to_string(d->num_frame_groups) + ")");
    for (int32_t i = 0; d->site_group && i < p->hp.num_atoms; i++)
        if (d->site_group[i] < -1 || d->site_group[i] >= d->num_site_groups)
            return fail(p, VVHIP_ERR_INVALID, "sdf: site_group[" + std::to_string(i) + "] = " + std::to_string((int) d->site_group[i]) + " is outside [-1, num_site_groups = " + std::to_string(d->num_site_groups) + ")");
    for (int32_t c = 0; c < d->num_classes; c++)
        for (int q = 0; q < 2; q++) {
            const int32_t count = q ? d->num_site_groups : d->num_frame_groups;
            if (d->classes[2 * c + q] < 0 || d->classes[2 * c + q] >= count)
                return fail(p, VVHIP_ERR_INVALID, "sdf: classes[" + std::to_string(c) + "][" + std::to_string(q) + "] = " + std::to_string(d->classes[2 * c + q]) + " is outside [0, " +
                                                  (q ? "num_site_groups = " : "num_frame_groups = ") + std::to_string(count) + ")");
        }
    for (int32_t f = 0; f < d->num_frames; f++) {
        const int32_t* t = d->frames + 3 * (size_t) f;
        const std::string who = "sdf: frames[" + std::to_string(f) + "] = {" + std::to_string(t[0]) + ", " + std::to_string(t[1]) + ", " + std::to_string(t[2]) + "}";
        for (int q = 0; q < 3; q++)
            if (t[q] < 0 || t[q] >= p->hp.num_atoms) return fail(p, VVHIP_ERR_INVALID, who + " has an index outside the System's " + std::to_string(p->hp.num_atoms) + " particles");
        if (t[0] == t[1] || t[0] == t[2] || t[1] == t[2]) return fail(p, VVHIP_ERR_INVALID, who + " names a particle twice");
        const int32_t m = p->hp.mol_id[(size_t) t[0]];
        if (p->hp.mol_id[(size_t) t[1]] != m || p->hp.mol_id[(size_t) t[2]] != m) return fail(p, VVHIP_ERR_INVALID, who + " spans molecules (mol_id): a frame lies in one molecule");
    }
    // ---- the sites, the frames, the layout and the pair kernel's work list, host only
    vvhip_plan::Sdf N;
    vvhip_sdf_layout& L = N.lay;
    L.interval = d->interval; L.nbins = d->nbins; L.num_frame_groups = d->num_frame_groups; L.num_site_groups = d->num_site_groups;
    L.num_classes = d->num_classes; L.exclude_same_molecule = d->exclude_same_molecule != 0; L.tile = vv::RDF_TILE;
    L.max_samples = d->max_samples; L.words = (int64_t) d->num_classes * d->nbins * d->nbins * d->nbins;
    L.extent = d->extent; L.voxel = 2.0 * d->extent / (double) d->nbins;
    if (L.words > VVHIP_SDF_MAX_WORDS)
        return fail(p, VVHIP_ERR_INVALID, "sdf: the table would have " + std::to_string((long long) L.words) + " words (num_classes * nbins^3), above the cap of " +
                                          std::to_string((long long) VVHIP_SDF_MAX_WORDS) + " (64 MiB, which a recovery snapshot copies too): fewer voxels or classes");
    Sites S = sites_by_group(p->hp, d->site_group, d->num_site_groups, L.exclude_same_molecule != 0, nullptr, false);
    std::copy(S.count, S.count + d->num_site_groups, L.num_sites);
    int32_t ffirst[vv::SDF_MAX_GROUPS + 1] = {0};
    auto fgroup_of = [&](int32_t f) { return d->frame_group ? (int) d->frame_group[f] : 0; };
    for (int32_t f = 0; f < d->num_frames; f++)
        if (fgroup_of(f) >= 0) L.num_frames[fgroup_of(f)]++;
    for (int g = 0; g < d->num_frame_groups; g++) ffirst[g + 1] = ffirst[g] + L.num_frames[g];
    int64_t largest = 0;
    for (int32_t c = 0; c < d->num_classes; c++) {
        L.classes[c][0] = d->classes[2 * c]; L.classes[c][1] = d->classes[2 * c + 1];
        L.pairs_per_sample[c] = (int64_t) L.num_frames[L.classes[c][0]] * L.num_sites[L.classes[c][1]];
        largest = std::max(largest, L.pairs_per_sample[c]);
    }
    TRY(check_pair_count(p, "sdf", largest, d->max_samples, "voxel"));
    if (!box_holds_cube(p->box, d->extent))
        return fail(p, VVHIP_ERR_INVALID, "sdf: extent = " + std::to_string(d->extent) + " nm is too large for the box: 3 extent^2 must be below (min(L) / 2)^2 with min(L) = " +
                                          std::to_string(std::min(p->box[0], std::min(p->box[1], p->box[2]))) + " nm, or a site would have more than one image in the cube");
    TRY(no_pairs_across_shards(p, "sdf", "table"));
    N.index = std::move(S.index); N.mol = std::move(S.mol);
    // the frames ordered by group, inside a group as given
    const size_t nf = (size_t) ffirst[d->num_frame_groups];
    N.frames.resize(3 * nf); N.fgroup.resize(nf);
    if (L.exclude_same_molecule) N.fmol.resize(nf);
    int32_t next[vv::SDF_MAX_GROUPS];
    std::copy(ffirst, ffirst + vv::SDF_MAX_GROUPS, next);
    for (int32_t f = 0; f < d->num_frames; f++) {
        const int g = fgroup_of(f);
        if (g < 0) continue;
        const size_t at = (size_t) next[g]++;
        std::copy(d->frames + 3 * (size_t) f, d->frames + 3 * (size_t) f + 3, N.frames.begin() + 3 * at);
        N.fgroup[at] = (unsigned char) g;
        if (L.exclude_same_molecule) N.fmol[at] = p->hp.mol_id[(size_t) d->frames[3 * (size_t) f]];
    }
    // the work list, as the RDF's: per class and i-tile of frames the j-sites in runs of `max_jsites`, a multiple of 64.  A small
    // workload gets runs of 64, so that its blocks fill the device; beyond sdf_items_target blocks a run grows
    constexpr int T = vv::RDF_TILE;
    long long runs = 0;                                     // of 64 j-sites, over all i-tiles
    for (int32_t c = 0; c < d->num_classes; c++)
        runs += ((long long) L.num_frames[L.classes[c][0]] + T - 1) / T * (((long long) L.num_sites[L.classes[c][1]] + 63) / 64);
    const int target = std::max(1, p->sdf_items_target);
    N.max_jsites = 64 * (int) std::max<long long>(1, std::min<long long>(4096, (runs + target - 1) / target));
    for (int32_t c = 0; c < d->num_classes; c++) {
        const int fg = L.classes[c][0], sg = L.classes[c][1];
        const int32_t na = L.num_frames[fg], nb = L.num_sites[sg];
        for (int32_t i0 = 0; i0 < na; i0 += T)
            for (int32_t j0 = 0; j0 < nb; j0 += N.max_jsites)
                N.items.push_back({c, 0, ffirst[fg] + i0, std::min(T, na - i0), S.first[sg], j0, std::min(nb, j0 + N.max_jsites), 0});
    }
    L.num_items = (int32_t) N.items.size();
    L.scratch_bytes = ((int64_t) 3 * N.stride() + (int64_t) vv::SDF_FRAME_PLANES * N.fstride()) * (int64_t) sizeof(double);
    return recorder_install(p, &vvhip_plan::sdf, "sdf", N, d->interval);
}
int vvhip_sdf_sample(vvhip_plan* p) {
    NEED_BOUND(p);
    if (!p->sdf.on) return fail(p, VVHIP_ERR_INVALID, "sdf: none started (vvhip_sdf_start)");
    TRY(quiesce(p, "sdf", false, false));
    return sdf_enqueue(p);
}
int vvhip_sdf_read(vvhip_plan* p, int64_t* words_out, int64_t capacity_words, vvhip_sdf_counts* out, int32_t reset) {
    long long head[vv::SDF_HEAD];
    TRY(recorder_fetch(p, &vvhip_plan::sdf, "sdf", words_out, capacity_words, head));
    if (out) {
        *out = {head[vv::SDF_SAMPLES], head[vv::SDF_DROPPED], head[vv::SDF_INVALID], head[vv::SDF_BAD_FRAMES], 0.0, {0}};
        std::memcpy(&out->inv_volume_sum, &head[vv::SDF_INV_VOLUME], sizeof(double));
        std::copy(head + vv::SDF_VISITS, head + vv::SDF_VISITS + vv::SDF_MAX_GROUPS, out->frame_visits);
    }
    return reset ? recorder_reset(p, p->sdf) : VVHIP_OK;
}
int vvhip_sdf_stop(vvhip_plan* p) { return recorder_stop(p, &vvhip_plan::sdf, "sdf"); }
int vvhip_sdf_info(const vvhip_plan* p, vvhip_sdf_layout* out) { return recorder_info(p, &vvhip_plan::sdf, out); }

int vvhip_current_start(vvhip_plan* p, const vvhip_current_desc* d) {
    if (!p) return VVHIP_ERR_INVALID;
    if (!d) return fail(p, VVHIP_ERR_INVALID, "current: null description");
    TRY(check_lags(p, "current", d->interval, d->num_lags, d->origin_every));
    if (d->num_groups < 1 || d->num_groups > vv::CUR_MAX_GROUPS) return fail(p, VVHIP_ERR_INVALID, "current: num_groups must be in [1, 8]");
    TRY(check_max_samples(p, "current", d->max_samples));
    if (!(d->limit_position >= 0) || !std::isfinite(d->limit_position)) return fail(p, VVHIP_ERR_INVALID, "current: limit_position must be finite and >= 0 (0: the default of 64 nm)");
    if (!(d->limit_velocity >= 0) || !std::isfinite(d->limit_velocity)) return fail(p, VVHIP_ERR_INVALID, "current: limit_velocity must be finite and >= 0 (0: the default of 64 nm/ps)");
    if (!d->weight) return fail(p, VVHIP_ERR_INVALID, "current: weight must not be NULL");
    TRY(check_groups(p, "current", d->group, d->num_groups));
    TRY(check_weights(p, "current", d->weight));
    // ---- the recorded particles, the layout and the fixed point, host only
    vvhip_plan::Current N;
    vvhip_current_layout& L = N.lay;
    Sites S = sites_by_group(p->hp, d->group, d->num_groups, false, d->weight, true);
    const int G = d->num_groups;
    L.interval = d->interval; L.num_lags = d->num_lags; L.origin_every = d->origin_every; L.num_groups = G;
    L.max_samples = d->max_samples;
    L.num_particles = (int32_t) S.index.size();
    L.num_origins = num_origins_of(d->num_lags, d->origin_every);
    L.num_disp_classes = G * (G + 1) / 2; L.num_cur_classes = G * G;
    L.row_words = 1 + 3 * (L.num_disp_classes + L.num_cur_classes);
    L.words = (int64_t) (L.num_lags + 1) * L.row_words;
    L.ring_bytes = (int64_t) L.num_origins * (G * 6 + 1) * (int64_t) sizeof(long long);
    L.limit_position = d->limit_position > 0 ? pow2_at_least(d->limit_position) : 64.0;
    L.limit_velocity = d->limit_velocity > 0 ? pow2_at_least(d->limit_velocity) : 64.0;
    L.weight_bound = S.wmax > 0 ? pow2_above(S.wmax) : 1.0;
    const int head_room = 62 - ceil_log2((long long) S.index.size() + 1) - std::ilogb(L.weight_bound);
    L.frac_bits_position = std::min(40, head_room - std::ilogb(L.limit_position));
    L.frac_bits_velocity = std::min(40, head_room - std::ilogb(L.limit_velocity));
    for (int q = 0; q < 2; q++) {
        const int f = q ? L.frac_bits_velocity : L.frac_bits_position;
        if (f < 8)
            return fail(p, VVHIP_ERR_INVALID, std::string("current: the ") + (q ? "velocity" : "position") + " sums would keep " + std::to_string(f) + " fraction bits (< 8) with " +
                                              std::to_string(S.index.size()) + " particles, weights below " + std::to_string(L.weight_bound) + " and limit " +
                                              std::to_string(q ? L.limit_velocity : L.limit_position) + ": lower the limit or scale the weights");
    }
    TRY(no_sums_across_shards(p, "current"));
    N.index = std::move(S.index); N.weight = std::move(S.weight); N.group = std::move(S.group);
    N.two_level = p->current_two_level != 0;
    return recorder_install(p, &vvhip_plan::current, "current", N, d->interval);
}
int vvhip_current_read(vvhip_plan* p, int64_t* words_out, int64_t capacity_words, vvhip_current_counts* out, int32_t reset) {
    long long head[vv::CUR_HEAD];
    TRY(recorder_fetch(p, &vvhip_plan::current, "current", words_out, capacity_words, head));
    if (out) {
        double s;
        std::memcpy(&s, &head[vv::CUR_INV_VOLUME], sizeof s);
        *out = {head[vv::CUR_SAMPLES], head[vv::CUR_DROPPED], head[vv::CUR_OUT_OF_RANGE], head[vv::CUR_INVALID], head[vv::CUR_FLOOR], s};
    }
    return reset ? recorder_reset(p, p->current) : VVHIP_OK;
}
int vvhip_current_stop(vvhip_plan* p) { return recorder_stop(p, &vvhip_plan::current, "current"); }
int vvhip_current_info(const vvhip_plan* p, vvhip_current_layout* out) { return recorder_info(p, &vvhip_plan::current, out); }

int vvhip_modes_start(vvhip_plan* p, const vvhip_modes_desc* d) {
    if (!p) return VVHIP_ERR_INVALID;
    if (!d) return fail(p, VVHIP_ERR_INVALID, "modes: null description");
    TRY(check_lags(p, "modes", d->interval, d->num_lags, d->origin_every, 0));
    if (d->num_groups < 1 || d->num_groups > vv::MODES_MAX_GROUPS) return fail(p, VVHIP_ERR_INVALID, "modes: num_groups must be in [1, 8]");
    if (d->num_modes < 1 || d->num_modes > 4096) return fail(p, VVHIP_ERR_INVALID, "modes: num_modes must be in [1, 4096]");
    TRY(check_max_samples(p, "modes", d->max_samples));
    if (!(d->limit_position >= 0) || !std::isfinite(d->limit_position)) return fail(p, VVHIP_ERR_INVALID, "modes: limit_position must be finite and >= 0 (0: the default of 64 nm)");
    if (!d->weight) return fail(p, VVHIP_ERR_INVALID, "modes: weight must not be NULL");
    if (!d->modes) return fail(p, VVHIP_ERR_INVALID, "modes: modes must not be NULL");
    for (int32_t k = 0; k < d->num_modes; k++)
        for (int c = 0; c < 3; c++)
            if (d->modes[3 * k + c] < -4095 || d->modes[3 * k + c] > 4095)
                return fail(p, VVHIP_ERR_INVALID, "modes: modes[" + std::to_string(k) + "][" + std::to_string(c) + "] = " + std::to_string(d->modes[3 * k + c]) + " is outside [-4095, 4095]");
    TRY(check_groups(p, "modes", d->group, d->num_groups));
    TRY(check_weights(p, "modes", d->weight));
    // ---- the recorded sites, the layout, the fixed point and the mode kernel's work list, host only
    vvhip_plan::Modes N;
    vvhip_modes_layout& L = N.lay;
    const int G = d->num_groups, K = d->num_modes;
    Sites S = sites_by_group(p->hp, d->group, G, false, d->weight, false);
    std::copy(S.count, S.count + G, L.group_sites);
    const int32_t* first = S.first;
    L.interval = d->interval; L.num_lags = d->num_lags; L.origin_every = d->origin_every; L.num_groups = G; L.num_modes = K;
    L.max_samples = d->max_samples;
    L.num_particles = first[G];
    L.num_origins = num_origins_of(d->num_lags, d->origin_every);
    L.row_words = 1 + G * G * K;
    L.words = (int64_t) (L.num_lags + 1) * L.row_words;
    L.ring_bytes = (int64_t) L.num_origins * ((int64_t) G * K * 2 + 1) * (int64_t) sizeof(long long);
    L.limit_position = d->limit_position > 0 ? pow2_at_least(d->limit_position) : 64.0;
    L.weight_bound = S.wmax > 0 ? pow2_above(S.wmax) : 1.0;
    L.frac_bits = 30 - std::ilogb(L.weight_bound);
    if (L.frac_bits < 8)
        return fail(p, VVHIP_ERR_INVALID, "modes: the terms would keep " + std::to_string(L.frac_bits) + " fraction bits (< 8) with weights below " +
                                          std::to_string(L.weight_bound) + ": scale the weights");
    if (31 + ceil_log2((long long) L.num_particles + 1) > 62)
        return fail(p, VVHIP_ERR_INVALID, "modes: " + std::to_string(L.num_particles) + " terms of 31 bits could overflow a 64-bit sum");
    if (L.words > (1ll << 26))
        return fail(p, VVHIP_ERR_INVALID, "modes: the table would have " + std::to_string((long long) L.words) + " words (num_lags + 1 rows of 1 + G^2 K), above 2^26: "
                                          "record fewer lags, modes or groups");
    TRY(no_sums_across_shards(p, "modes"));
    N.index = std::move(S.index); N.weight = std::move(S.weight);
    N.modes.assign(d->modes, d->modes + 3 * (size_t) K);
    // the work list: per group its sites in runs of block_threads * sites_per_thread, the modes in runs of k_tile.  First choices (nothing
    // here has been scanned on a device yet: TUNING_LOG.md): blocks of 256 threads; 4 sites per thread and 32 modes per item where that
    // still makes 1024 items, else fewer of either (sites first: a short mode run pays the wave sum and the flush more often)
    L.block_threads = p->modes_block_threads ? p->modes_block_threads : 256;
    auto count_items = [&](int P, int kt) {
        long long n = 0;
        for (int g = 0; g < G; g++) n += (long long) ((L.group_sites[g] + L.block_threads * P - 1) / (L.block_threads * P)) * ((K + kt - 1) / kt);
        return n;
    };
    int P = p->modes_sites_per_thread ? p->modes_sites_per_thread : 4, kt = p->modes_k_tile ? p->modes_k_tile : 32;
    while (!p->modes_sites_per_thread && P > 1 && count_items(P, kt) < 1024) P /= 2;
    while (!p->modes_k_tile && kt > 8 && count_items(P, kt) < 1024) kt /= 2;
    L.sites_per_thread = P; L.k_tile = kt;
    const int run = L.block_threads * P;
    for (int g = 0; g < G; g++)
        for (int32_t s0 = first[g]; s0 < first[g + 1]; s0 += run)
            for (int32_t k0 = 0; k0 < K; k0 += kt)
                N.items.push_back({g, s0, std::min(first[g + 1], s0 + run), k0, std::min(K, k0 + kt), {0, 0, 0}});
    L.num_items = (int32_t) N.items.size();
    L.scratch_bytes = (int64_t) 3 * N.stride() * (int64_t) sizeof(unsigned int);
    return recorder_install(p, &vvhip_plan::modes, "modes", N, d->interval);
}
int vvhip_modes_read(vvhip_plan* p, int64_t* words_out, int64_t capacity_words, vvhip_modes_counts* out, int32_t reset) {
    long long head[vv::MODES_HEAD];
    TRY(recorder_fetch(p, &vvhip_plan::modes, "modes", words_out, capacity_words, head));
    if (out) {
        *out = {head[vv::MODES_SAMPLES], head[vv::MODES_DROPPED], head[vv::MODES_OUT_OF_RANGE], head[vv::MODES_INVALID], head[vv::MODES_FLOOR], {0, 0, 0}};
        std::memcpy(out->box_sum, &head[vv::MODES_BOX_SUM], sizeof out->box_sum);
    }
    return reset ? recorder_reset(p, p->modes) : VVHIP_OK;
}
int vvhip_modes_stop(vvhip_plan* p) { return recorder_stop(p, &vvhip_plan::modes, "modes"); }
int vvhip_modes_info(const vvhip_plan* p, vvhip_modes_layout* out) { return recorder_info(p, &vvhip_plan::modes, out); }

int vvhip_contacts_start(vvhip_plan* p, const vvhip_contacts_desc* d) {
    if (!p) return VVHIP_ERR_INVALID;
    if (!d) return fail(p, VVHIP_ERR_INVALID, "contacts: null description");
    TRY(check_lags(p, "contacts", d->interval, d->num_lags, d->origin_every));
    if (d->num_groups < 1 || d->num_groups > vv::CONTACTS_MAX_GROUPS) return fail(p, VVHIP_ERR_INVALID, "contacts: num_groups must be in [1, 16]");
    if (d->num_classes < 1 || d->num_classes > vv::CONTACTS_MAX_CLASSES) return fail(p, VVHIP_ERR_INVALID, "contacts: num_classes must be in [1, 8]");
    if (!d->classes) return fail(p, VVHIP_ERR_INVALID, "contacts: classes must not be NULL");
    if (!d->r_cut) return fail(p, VVHIP_ERR_INVALID, "contacts: r_cut must not be NULL");
    TRY(check_max_samples(p, "contacts", d->max_samples));
    TRY(check_groups(p, "contacts", d->group, d->num_groups));
    TRY(check_classes(p, "contacts", d->classes, d->num_classes, d->num_groups));
    for (int32_t c = 0; c < d->num_classes; c++)
        if (!(d->r_cut[c] > 0) || !std::isfinite(d->r_cut[c]))
            return fail(p, VVHIP_ERR_INVALID, "contacts: r_cut[" + std::to_string(c) + "] must be finite and > 0");
    // ---- the sites, the layout and the two kernels' work lists, host only
    vvhip_plan::Contacts N;
    vvhip_contacts_layout& L = N.lay;
    L.interval = d->interval; L.num_lags = d->num_lags; L.origin_every = d->origin_every; L.num_groups = d->num_groups;
    L.num_classes = d->num_classes; L.exclude_same_molecule = d->exclude_same_molecule != 0; L.continuous = d->continuous != 0;
    L.max_samples = d->max_samples; L.words = (int64_t) d->num_classes * d->num_lags * 4;
    L.rows_per_tile = p->contacts_rows_per_tile; L.words_per_item = p->contacts_words_per_item; L.skip_zero_words = p->contacts_skip_zero;
    Sites S = sites_by_group(p->hp, d->group, d->num_groups, L.exclude_same_molecule != 0, nullptr, false);
    std::copy(S.count, S.count + d->num_groups, L.num_sites);
    std::copy(S.first, S.first + vv::CONTACTS_MAX_GROUPS + 1, N.first);
    int64_t largest = 0;
    double longest = 0;
    for (int32_t c = 0; c < d->num_classes; c++) {
        const int ga = d->classes[2 * c], gb = d->classes[2 * c + 1];
        L.classes[c][0] = ga; L.classes[c][1] = gb;
        L.rows[c] = L.num_sites[ga]; L.cols[c] = L.num_sites[gb];
        L.r_cut[c] = d->r_cut[c];
        largest = std::max(largest, (int64_t) L.rows[c] * L.cols[c]);
        longest = std::max(longest, d->r_cut[c]);
    }
    N.geo = vv::contacts_layout(L.num_classes, L.rows, L.cols, L.num_lags, L.origin_every, L.continuous != 0, N.first[d->num_groups], vv::CONTACTS_HEAD);
    const vv::ContactsLayout& G = N.geo;
    L.num_origins = G.num_origins; L.sample_words = G.sample_words;
    for (int32_t c = 0; c < d->num_classes; c++) L.class_words[c] = G.class_words[c];
    L.words_bytes = G.words_bytes; L.scratch_bytes = G.scratch_bytes; L.total_bytes = G.total_bytes;
    TRY(check_origins(p, "contacts", L.num_origins));
    TRY(check_pair_count(p, "contacts", largest, d->max_samples, "word"));
    if (L.total_bytes > VVHIP_CONTACTS_MAX_BYTES)
        return fail(p, VVHIP_ERR_INVALID, "contacts: the recorder would hold " + std::to_string((long long) L.total_bytes) + " bytes (" + std::to_string(L.num_origins) + " slots of " +
                                          std::to_string((long long) L.sample_words * 8) + " bytes" + (L.continuous ? ", twice" : "") + "), above VVHIP_CONTACTS_MAX_BYTES = 2^32: raise origin_every, record fewer lags or fewer sites");
    TRY(check_half_box(p, "contacts", "the cutoff ", longest));
    TRY(no_pairs_across_shards(p, "contacts", "matrix"));
    N.index = std::move(S.index); N.mol = std::move(S.mol);
    // the work lists (vv_layout.h): per class, tile of rows and run of column words a block of the mask kernel; per class and run of
    // CONTACTS_CORR_PAIRS pairs of words a block of the correlate kernel for every slot
    N.mask_items.resize((size_t) vv::contacts_mask_items(G, L.num_classes, L.rows_per_tile, L.words_per_item, nullptr));
    vv::contacts_mask_items(G, L.num_classes, L.rows_per_tile, L.words_per_item, N.mask_items.data());
    N.corr_items.resize((size_t) vv::contacts_corr_items(G, L.num_classes, nullptr));
    vv::contacts_corr_items(G, L.num_classes, N.corr_items.data());
    L.num_mask_items = (int32_t) N.mask_items.size(); L.num_corr_items = (int32_t) N.corr_items.size();
    return recorder_install(p, &vvhip_plan::contacts, "contacts", N, d->interval);
}
int vvhip_contacts_sample(vvhip_plan* p) {
    NEED_BOUND(p);
    if (!p->contacts.on) return fail(p, VVHIP_ERR_INVALID, "contacts: none started (vvhip_contacts_start)");
    TRY(quiesce(p, "contacts", false, false));
    return contacts_enqueue(p);
}
int vvhip_contacts_read(vvhip_plan* p, int64_t* words_out, int64_t capacity_words, vvhip_contacts_counts* out, int32_t reset) {
    long long head[vv::CONTACTS_HEAD];
    TRY(recorder_fetch(p, &vvhip_plan::contacts, "contacts", words_out, capacity_words, head));
    if (out) *out = {head[vv::CONTACTS_SAMPLES], head[vv::CONTACTS_DROPPED], head[vv::CONTACTS_INVALID]};
    return reset ? recorder_reset(p, p->contacts) : VVHIP_OK;
}
int vvhip_contacts_stop(vvhip_plan* p) { return recorder_stop(p, &vvhip_plan::contacts, "contacts"); }
int vvhip_contacts_info(const vvhip_plan* p, vvhip_contacts_layout* out) { return recorder_info(p, &vvhip_plan::contacts, out); }

int vvhip_acf_start(vvhip_plan* p, const vvhip_acf_desc* d) {
    if (!p) return VVHIP_ERR_INVALID;
    if (!d) return fail(p, VVHIP_ERR_INVALID, "acf: null description");
    TRY(check_lags(p, "acf", d->interval, d->num_lags, d->origin_every));
    if (d->mode != VVHIP_ACF_VELOCITY_PARTICLES && d->mode != VVHIP_ACF_VELOCITY_MOLECULES && d->mode != VVHIP_ACF_ORIENTATION)
        return fail(p, VVHIP_ERR_INVALID, "acf: mode must be VVHIP_ACF_VELOCITY_PARTICLES, VVHIP_ACF_VELOCITY_MOLECULES or VVHIP_ACF_ORIENTATION");
    if (d->num_groups < 1 || d->num_groups > 16) return fail(p, VVHIP_ERR_INVALID, "acf: num_groups must be in [1, 16]");
    TRY(check_max_samples(p, "acf", d->max_samples));
    if (!(d->limit >= 0) || !std::isfinite(d->limit)) return fail(p, VVHIP_ERR_INVALID, "acf: limit must be finite and >= 0 (0: the default of 64 nm/ps)");
    const bool orientation = d->mode == VVHIP_ACF_ORIENTATION;
    if (orientation && d->limit != 0) return fail(p, VVHIP_ERR_INVALID, "acf: limit must be 0 in orientation mode (a unit vector has no range to choose)");
    if (orientation && (d->num_pairs < 0 || (d->num_pairs > 0 && !d->pairs))) return fail(p, VVHIP_ERR_INVALID, "acf: orientation mode needs pairs[2 * num_pairs] and num_pairs >= 0");
    if (!orientation && (d->pairs || d->num_pairs != 0)) return fail(p, VVHIP_ERR_INVALID, "acf: pairs and num_pairs belong to orientation mode only");
    const vv::HostPlan& hp = p->hp;
    TRY(check_groups(p, "acf", d->group, d->num_groups, orientation ? d->num_pairs : -1));      // (of the particles, or of the pairs)
    // ---- the units this plan records, the layout and the fixed point, host only
    vvhip_plan::Acf N;
    vvhip_acf_layout& L = N.lay;
    N.grouped = d->group != nullptr; N.molecules = d->mode == VVHIP_ACF_VELOCITY_MOLECULES;
    PlanUnits U;
    if (!orientation) TRY(plan_units(p, "acf", d->group, N.molecules, U));
    // orientation: the pairs in place of the particles.  Every pair is validated before its group is looked at
    for (int32_t u = 0; orientation && u < d->num_pairs; u++) {
        const int32_t h = d->pairs[2 * u], t = d->pairs[2 * u + 1];
        const std::string name = "acf: pair " + std::to_string(u) + " (head " + std::to_string(h) + ", tail " + std::to_string(t) + ")";
        if (h < 0 || h >= hp.num_atoms || t < 0 || t >= hp.num_atoms) return fail(p, VVHIP_ERR_INVALID, name + " names a particle outside the System's " + std::to_string(hp.num_atoms));
        if (h == t) return fail(p, VVHIP_ERR_INVALID, name + " has head = tail: no direction");
        if (hp.mol_id[(size_t) h] != hp.mol_id[(size_t) t])
            return fail(p, VVHIP_ERR_INVALID, name + " joins molecules " + std::to_string(hp.mol_id[(size_t) h]) + " and " + std::to_string(hp.mol_id[(size_t) t]) + ": no minimum image is taken, head and tail must lie in one molecule");
        const int g = d->group ? (int) d->group[u] : 0;
        if (g < 0) continue;
        U.described++;
        const int here = (h >= hp.shard_begin && h < hp.shard_end) + (t >= hp.shard_begin && t < hp.shard_end);
        U.cut = U.cut || here == 1;
        if (here == 2) U.units.push_back({g, u});
    }
    L.interval = d->interval; L.num_lags = d->num_lags; L.origin_every = d->origin_every; L.mode = d->mode; L.num_groups = d->num_groups;
    L.max_samples = d->max_samples;
    L.num_units = (int32_t) U.units.size();
    L.num_origins = num_origins_of(d->num_lags, d->origin_every);
    L.row_words = orientation ? 5 : 4;
    L.words = (int64_t) L.num_groups * L.num_lags * L.row_words;
    L.limit = orientation ? 1.0 : d->limit > 0 ? pow2_at_least(d->limit) : 64.0;
    L.ring_bytes = (int64_t) L.num_origins * 3 * N.stride() * (int64_t) sizeof(double);
    TRY(units_frac_bits(p, "acf", U.described, L.max_samples, L.origin_every, L.limit, &L.frac_bits));
    TRY(check_origins(p, "acf", L.num_origins));
    if (N.molecules && U.cut)
        return fail(p, VVHIP_ERR_UNSUPPORTED, "acf: the particle shard cuts a molecule: its centre-of-mass velocity needs particles of another shard");
    if (orientation && U.cut)
        return fail(p, VVHIP_ERR_UNSUPPORTED, "acf: the particle shard cuts a recorded pair: its vector needs a particle of another shard (shard on molecule boundaries)");
    fill_units(hp, N, U, orientation ? d->pairs : nullptr);
    return recorder_install(p, &vvhip_plan::acf, "acf", N, d->interval);
}
int vvhip_acf_read(vvhip_plan* p, int64_t* words_out, int64_t capacity_words, vvhip_acf_counts* out, int32_t reset) {
    long long head[vv::ACF_HEAD];
    TRY(recorder_fetch(p, &vvhip_plan::acf, "acf", words_out, capacity_words, head));
    if (out) *out = {head[vv::ACF_SAMPLES], head[vv::ACF_DROPPED], head[vv::ACF_OUT_OF_RANGE], head[vv::ACF_FLOOR]};
    return reset ? recorder_reset(p, p->acf) : VVHIP_OK;
}
int vvhip_acf_stop(vvhip_plan* p) { return recorder_stop(p, &vvhip_plan::acf, "acf"); }
int vvhip_acf_info(const vvhip_plan* p, vvhip_acf_layout* out) { return recorder_info(p, &vvhip_plan::acf, out); }

}  // extern "C"
