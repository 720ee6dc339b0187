// vv_run.cpp -- the plan-driven loops (vvhip_run_graph / vvhip_run_eager): the random slices of their steps, the captured graphs and their
// keys, and the recovery from a missed rendezvous of the one-launch step.
#include "vv_plan.hpp"

// the slot of parity q that holds (or will hold) the graph with this key
static vvhip_plan::GraphSlot& graph_slot(vvhip_plan* p, int q, const GraphKey& key) {
    auto& row = p->graph[q & 1];
    for (auto& g : row)
        if (g.exec && g.key == key) return g;
    for (auto& g : row)
        if (!g.exec) return g;
    return row[p->graph_next[q & 1]++ % vvhip_plan::kGraphWays];
}

// integration.prepareRandomNumbers(n) for the plan-driven loops: hand out the next slice; when the buffer is exhausted
// enqueue a refill by the device generator and start over.  `force_refill` starts a graph with fresh numbers.
static int next_random_slice(vvhip_plan* p, uint32_t* index, bool force_refill) {
    *index = 0;
    if (!p->hp.has_ld) return VVHIP_OK;
    const vvhip_plan_info& in = p->hp.info;
    const uint32_t need = (uint32_t) std::max(in.num_normal_ld, 1) + 2u * (uint32_t) std::max(in.num_pairs_ld, 1);   // HOST:806-807,863
    if (need > p->buf.random_size) return fail(p, VVHIP_ERR_INVALID, "random buffer smaller than one step's demand");
    if (force_refill || p->cur.random_pos + need > p->buf.random_size) {
        HIP_TRY(p, vv::launch_fill_normals((float4*) p->buf.random, p->buf.random_size, p->rng_seed, p->d_epoch.get(), p->stream));
        p->cur.random_pos = 0;
    }
    *index = p->cur.random_pos;
    p->cur.random_pos += need;
    return VVHIP_OK;
}

// ---- recovery from a missed rendezvous (vvhip_plan::Recovery)
// What a snapshot -- and a checkpoint (vv_checkpoint.cpp) -- holds: see RecItem in vv_plan.hpp.
std::vector<RecItem> recovery_items(vvhip_plan* p, const bool with[kRiders]) {
    vvhip_plan::Recovery& r = p->rec;
    const vv::HostPlan& hp = p->hp;
    const size_t nloc = (size_t) (hp.shard_end - hp.shard_begin), rs = sizeof_real(hp.precision), ms = sizeof_mixed(hp.precision);
    std::vector<RecItem> v = {
        {p->buf.posq, &r.posq, nloc * 4 * rs, false, (uint32_t) rs},
        {p->buf.posq_correction, &r.corr, p->buf.posq_correction ? nloc * 4 * rs : 0, false, (uint32_t) rs},
        {p->buf.velm, &r.velm, nloc * 4 * ms, false, (uint32_t) ms},
        {p->buf.force, &r.force, (size_t) hp.padded_num_atoms * 3 * 8, false},                                              // (planar int64)
        {p->d_fextra.get(), &r.fextra, nloc * 3 * rs, false, (uint32_t) (3 * rs / 4)},
        {const_cast<void*>(p->buf.random), &r.random, hp.has_ld ? (size_t) p->buf.random_size * sizeof(float4) : 0, false},      // the Langevin normals in use
        {p->d_nh.get(), &r.nh, 2 * sizeof(vv::NHDevState), false},
        {p->d_epoch.get(), &r.epoch, sizeof(unsigned long long), false}};
    const Riders rd = riders(p);
    for (int k = 0; with && k < kRiders; k++)      // (words the plan no longer has, or not yet, are left out)
        if (with[k] && rd[k].late) v.push_back({rd[k].late, &r.late[k], rd[k].late_bytes, true});
    return v;
}
static int recovery_snapshot(vvhip_plan* p) {
    vvhip_plan::Recovery& r = p->rec;
    const Riders rd = riders(p);                    // (none of them can start or stop while the snapshot is unverified: both settle it first)
    for (int k = 0; k < kRiders; k++) r.saved[k] = rd[k].late != nullptr;
    for (const RecItem& it : recovery_items(p, r.saved)) {
        if (!it.bytes) continue;
        HIP_TRY(p, it.saved->ensure(it.bytes));      // (a re-bind may have brought a larger random buffer)
        HIP_TRY(p, hipMemcpyAsync(it.saved->get(), it.live, it.bytes, hipMemcpyDeviceToDevice, p->stream));
    }
    r.cur = p->cur;
    r.runs.clear();
    r.valid = true;
    return VVHIP_OK;
}
// At the entry of a plan-driven run call: take the snapshot if there is none and the call is worth one; remember the call.
static int recovery_note_run(vvhip_plan* p, int kind, int nsteps, int spg, const ForceProvider& fp) {
    vvhip_plan::Recovery& r = p->rec;
    if (r.replaying || p->capturing || nsteps <= 0) return VVHIP_OK;
    if (!r.valid) {
        if (!r.enabled || nsteps < r.min_steps || !fused_state_ok(p) || p->comm || p->mb_on) return VVHIP_OK;
        TRY(recovery_snapshot(p));
    }
    r.runs.push_back({kind, nsteps, spg, fp});
    return VVHIP_OK;
}
int recover_rendezvous(vvhip_plan* p, bool on_request) {
    vvhip_plan::Recovery& r = p->rec;
    long long steps = 0;
    for (const auto& run : r.runs) steps += run.nsteps;
    if (!on_request)
        std::fprintf(stderr,"libvvhip: the one-launch step's blocks did not meet within 0.2 s (another process's kernels on the device?): the last %lld step(s) "
                         "are repeated from the plan's snapshot with two launches per step, and the plan keeps two launches from here on\n", steps);
    const std::vector<RecItem> items = recovery_items(p, r.saved);      // (of the riders: what the snapshot took and the plan still has)
    for (const RecItem& it : items)
        if (!it.late && it.bytes && it.saved->get()) HIP_TRY(p, hipMemcpyAsync(it.live, it.saved->get(), it.bytes, hipMemcpyDeviceToDevice, p->stream));
    // both accumulator copies are zero between steps; whatever the failed steps left in them goes
    HIP_TRY(p, hipMemsetAsync(p->d_acc.get(), 0, 2 * kAccN * sizeof(unsigned long long), p->stream));
    if (p->d_bigacc) HIP_TRY(p, hipMemsetAsync(p->d_bigacc.get(), 0, (size_t) p->hp.num_big * 4 * sizeof(unsigned long long), p->stream));
    HIP_TRY(p, hipMemsetAsync(rv_dead_tail(p->d_rv.get()), 0, kRvDeadTail * sizeof(unsigned long long), p->stream));
    // (with the step counter: the riders' schedules follow it, so the repeat writes the failed steps' rows and frames again at the same places
    // and redoes their removals at the same steps; the riders' scratch words are zero between steps whatever the failed steps computed)
    p->cur = r.cur;
    for (const RecItem& it : items)
        if (it.late) HIP_TRY(p, hipMemcpyAsync(it.live, it.saved->get(), it.bytes, hipMemcpyDeviceToDevice, p->stream));
    for (int w = 1; w < 4; w++) __atomic_store_n(&p->h_status[w], 0u, __ATOMIC_RELAXED);
    p->fused = false;
    forget_fused_checks(p);
    drop_graphs(p);
    r.recoveries++;
    r.valid = false;
    r.replaying = true;
    int rc = VVHIP_OK;
    const std::vector<vvhip_plan::Recovery::Run> runs = r.runs;
    r.runs.clear();
    for (const auto& run : runs) {
        rc = run.kind == 0 ? vvhip_run_graph(p, run.nsteps, run.spg, run.fp.site, run.fp.kt, run.fp.kd) : vvhip_run_eager(p, run.nsteps, run.fp.site, run.fp.kt, run.fp.kd);
        if (rc != VVHIP_OK) break;
    }
    r.replaying = false;
    if (rc != VVHIP_OK) return rc;
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    return check_exchange_health(p);
}

// One step of the plan-driven loops (vvhip_run_graph / vvhip_run_eager): force provider + fused step, in the scheme's order.
int plan_step(vvhip_plan* p, const ForceProvider& fp, bool refill) {
    uint32_t ri = 0;
    TRY(next_random_slice(p, &ri, refill));
    if (p->hp.params.use_middle_scheme) {
        if (fp.site) TRY(vvhip_synth_tether_force(p, fp.site, fp.kt, fp.kd));
        return vvhip_step_middle(p, ri);
    }
    TRY(vvhip_step_vv_first(p));
    if (fp.site) TRY(vvhip_synth_tether_force(p, fp.site, fp.kt, fp.kd));
    return vvhip_step_vv_second(p, ri);
}

// Capture + instantiate + upload the graph of `steps_per_graph` steps for thermostat parity `q`, unless that slot already holds it.
// Nothing is launched: the physical state is untouched.
// The graph is captured at step counter c0 (where its replays start): every rider that is on sits at the steps its window at c0 names.
static int prepare_slot(vvhip_plan* p, int q, int steps_per_graph, const ForceProvider& fp, long long c0, vvhip_plan::GraphSlot** out = nullptr) {
    hipStream_t s = p->stream;
    TRY(ensure_mass_table(p));                       // a one-off fill must not be recorded into the replayed graph
    GraphKey key{steps_per_graph, fp};
    const Riders rd = riders(p);
    for (int k = 0; k < kRiders; k++)
        if (rd[k].on) key.due[k] = rd[k].window(c0, steps_per_graph);
    vvhip_plan::GraphSlot& g = graph_slot(p, q, key);
    if (out) *out = &g;
    if (g.exec && g.key == key) return VVHIP_OK;
    if (g.exec) { (void) hipStreamSynchronize(s); (void) hipGraphExecDestroy(g.exec); g.exec = nullptr; }      // (a replay of the one that goes may still be in flight)
    // The capture walks the host's cursor (parity, Langevin random slice, step counter) through the graph's steps; it is put back
    // afterwards, because nothing has run yet.  A replay moves it to the graph's end (vvhip_run_graph).
    const vvhip_plan::Cursor cur0 = p->cur;
    p->cur.parity = q & 1;
    p->cur.step_count = c0;
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { p->cur = cur0; return hip_fail(p, e, "hipStreamBeginCapture"); }
    p->capturing = true;
    int rc = VVHIP_OK;
    // Langevin: a captured graph begins with a refill of the random buffer (the device generator's epoch advances per refill), so every replay draws new numbers
    for (int i = 0; i < steps_per_graph && rc == VVHIP_OK; i++) rc = plan_step(p, fp, i == 0 && p->hp.has_ld);
    p->capturing = false;
    e = hipStreamEndCapture(s, &graph);
    g.random_end = p->cur.random_pos;
    p->cur = cur0;
    if (rc != VVHIP_OK) { if (graph) (void) hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return hip_fail(p, e, "hipStreamEndCapture");
    e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void) hipGraphDestroy(graph);
    if (e != hipSuccess) { g.exec = nullptr; return hip_fail(p, e, "hipGraphInstantiate"); }
    (void) hipGraphUpload(g.exec, s);                // pay the first launch's set-up here, not in the caller's timed region
    g.key = std::move(key);
    p->graph_captures++;
    return VVHIP_OK;
}

extern "C" {

int vvhip_set_random_seed(vvhip_plan* p, uint64_t seed) {
    if (!p) return VVHIP_ERR_INVALID;
    p->rng_seed = seed;
    return VVHIP_OK;
}
int vvhip_fill_random(vvhip_plan* p) {
    NEED_BOUND(p);
    TRY(settle_recovery(p));
    if (!p->buf.random || !p->buf.random_size) return fail(p, VVHIP_ERR_INVALID, "no random buffer bound");
    HIP_TRY(p, vv::launch_fill_normals((float4*) p->buf.random, p->buf.random_size, p->rng_seed, p->d_epoch.get(), p->stream));
    p->cur.random_pos = 0;
    return VVHIP_OK;
}

int vvhip_synth_tether_force(vvhip_plan* p, const void* site, double k_tether, double k_drude) {
    NEED_BOUND(p);
    if (!site) return VVHIP_ERR_INVALID;
    TRY(settle_recovery(p));
    ScopedTimer t(p, T_OTHER, true);
    // (instrumented build: the provider stamps its waves only while vvhip_debug_step_spans numbers the launches -- its grid is not capped like the
    // kernels', and rows beyond the span buffer's 4096 per launch would be written past its end)
    vv::TetherArgs ta{p->buf.posq, site, p->buf.velm, (long long*) p->buf.force, p->d_slots.get(),
                      p->hp.padded_num_atoms, p->hp.info.num_waves, k_tether, k_drude, p->dbg_seq >= 0 ? p->d_dbg_span.get() : nullptr, p->dbg_parity, 0};
    if (p->dbg_seq >= 0) ta.dbg_parity = p->dbg_seq++ % 6;       // vvhip_debug_step_spans: every launch of the sequence stamps rows of its own
    HIP_TRY(p, vv::launch_tether(p->hp.precision, ta, p->block_threads, p->stream, t.e0, t.e1));
    return VVHIP_OK;
}

// Both parities' executables, ready to launch.  Hosts call this outside any timed region (bench.py does, after its warm-up);
// vvhip_run_graph prepares the slot of the current parity itself when it is missing.
int vvhip_graph_prepare(vvhip_plan* p, int steps_per_graph, const void* site, double k_tether, double k_drude) {
    NEED_BOUND(p);
    if (steps_per_graph < 1) return VVHIP_ERR_INVALID;
    if (steps_per_graph % 2) steps_per_graph += 1;   // the thermostat double-buffers by step parity: a graph must hold an even number of steps
    if (!p->stream) return fail(p, VVHIP_ERR_INVALID, "graph capture needs a non-null stream in vvhip_buffers.stream");
    const ForceProvider fp{site, k_tether, k_drude};
    TRY(prepare_slot(p, p->cur.parity, steps_per_graph, fp, p->cur.step_count));
    return prepare_slot(p, p->cur.parity ^ 1, steps_per_graph, fp, p->cur.step_count);
}

int vvhip_run_graph(vvhip_plan* p, int nsteps, int steps_per_graph, const void* site, double k_tether, double k_drude) {
    NEED_BOUND(p);
    if (nsteps < 0 || steps_per_graph < 1) return VVHIP_ERR_INVALID;
    if (steps_per_graph % 2) steps_per_graph += 1;
    TRY(check_exchange_health(p));
    hipStream_t s = p->stream;
    if (!s) return fail(p, VVHIP_ERR_INVALID, "graph capture needs a non-null stream in vvhip_buffers.stream");
    const ForceProvider fp{site, k_tether, k_drude};
    TRY(recovery_note_run(p, 0, nsteps, steps_per_graph, fp));
    struct InLoop { vvhip_plan* p; bool was; InLoop(vvhip_plan* q) : p(q), was(q->rec.in_loop) { p->rec.in_loop = true; } ~InLoop() { p->rec.in_loop = was; } } in_loop(p);
    const bool middle = p->hp.params.use_middle_scheme;
    // classic scheme (API:272-338): every step is first half -> forces -> second half, and the first half needs the forces of the
    // current positions; they are (re)computed once per call here, outside the replayed part
    if (!middle && site && nsteps > 0) TRY(vvhip_synth_tether_force(p, site, k_tether, k_drude));
    int done = 0;
    if (nsteps >= steps_per_graph) {
        vvhip_plan::GraphSlot* g = nullptr;
        TRY(prepare_slot(p, p->cur.parity, steps_per_graph, fp, p->cur.step_count, &g));     // no-op when the slot of this parity is ready
        const Riders rd = riders(p);
        for (; done + steps_per_graph <= nsteps; done += steps_per_graph) {
            // with a rider on, the replays' rows / removals / frames fall on other steps of the graph as the counter moves on: the graph whose
            // windows fit (at most two per rider when its interval and the graph's length divide one another; otherwise the cache may capture
            // again; on a logarithmic schedule most windows carry nothing and keep hitting the executable without)
            bool fits = true;
            for (int k = 0; k < kRiders && fits && done > 0; k++)
                fits = !rd[k].on || rd[k].window(p->cur.step_count, steps_per_graph) == g->key.due[k];
            if (!fits) TRY(prepare_slot(p, p->cur.parity, steps_per_graph, fp, p->cur.step_count, &g));
            HIP_TRY(p, hipGraphLaunch(g->exec, s));
            p->cur.step_count += steps_per_graph;
        }
        p->cur.random_pos = g->random_end;               // an even number of steps: the parity is where it was
        if (!middle && extra_flags(p)) p->cur.fextra_dirty = true;
        if (middle && middle_application(p).fe_virtual) p->cur.fextra_virtual = true;    // what the replayed steps' phase 0 would have set
    }
    for (; done < nsteps; done++) TRY(plan_step(p, fp, false));
    return VVHIP_OK;
}

int vvhip_run_eager(vvhip_plan* p, int nsteps, const void* site, double k_tether, double k_drude) {
    NEED_BOUND(p);
    if (nsteps < 0) return VVHIP_ERR_INVALID;
    TRY(check_exchange_health(p));
    const ForceProvider fp{site, k_tether, k_drude};
    TRY(recovery_note_run(p, 1, nsteps, 0, fp));
    struct InLoop { vvhip_plan* p; bool was; InLoop(vvhip_plan* q) : p(q), was(q->rec.in_loop) { p->rec.in_loop = true; } ~InLoop() { p->rec.in_loop = was; } } in_loop(p);
    if (!p->hp.params.use_middle_scheme && site && nsteps > 0) TRY(vvhip_synth_tether_force(p, site, k_tether, k_drude));   // see vvhip_run_graph
    for (int i = 0; i < nsteps; i++) TRY(plan_step(p, fp, false));
    return VVHIP_OK;
}

// The same steps through the per-KernelImpl entry points in VVIntegrator::stepMiddle's order (API:237-268) -- what the OpenMM adapter
// issues when constraints it cannot fuse force OpenMM's solver between the stages (the solver's own launches are not included).
int vvhip_run_eager_unfused(vvhip_plan* p, int nsteps, const void* site, double k_tether, double k_drude) {
    NEED_BOUND(p);
    if (nsteps < 0) return VVHIP_ERR_INVALID;
    if (!p->hp.params.use_middle_scheme) return fail(p, VVHIP_ERR_INVALID, "plan was created for the classic scheme");
    for (int i = 0; i < nsteps; i++) {
        uint32_t ri = 0;
        TRY(next_random_slice(p, &ri, false));
        if (site) TRY(vvhip_synth_tether_force(p, site, k_tether, k_drude));
        TRY(vvhip_reset_extra_force(p));
        if (p->hp.has_ld) TRY(vvhip_apply_langevin_force(p, ri));
        if (p->hp.has_ef) TRY(vvhip_apply_electric_force(p));
        if (cos_on(p)) TRY(vvhip_apply_cosine_force(p));
        TRY(vvhip_middle_kick(p));                  // (applyVelocityConstraints would run here)
        TRY(vvhip_middle_half_drift1(p));
        if (p->hp.has_nh) {
            if (cos_on(p)) { TRY(vvhip_calc_velocity_bias(p)); TRY(vvhip_remove_velocity_bias(p)); }
            TRY(vvhip_scale_velocity(p));
            if (cos_on(p)) TRY(vvhip_restore_velocity_bias(p));
        }
        TRY(vvhip_middle_half_drift2(p));           // (applyConstraints would run here)
        TRY(vvhip_middle_finish(p));
        if (p->hp.has_images) TRY(vvhip_update_image_positions(p));
    }
    return VVHIP_OK;
}

}  // extern "C"
