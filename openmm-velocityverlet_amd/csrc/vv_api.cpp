// vv_api.cpp -- the C ABI of include/vvhip.h on top of vv_host (analysis) and vv_kernels (HIP).
// "HOST" = platforms/cuda/src/CudaVVKernels.cpp, "API" = openmmapi/src/VVIntegrator.cpp of the reference.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include <dlfcn.h>
#include <unistd.h>
#include <rccl/rccl.h>      // types and prototypes only: the library is resolved at run time (see rccl_api)

#include "vv_devmem.hpp"
#include "vv_host.hpp"
#include "vv_kernels.hpp"
#include "vv_rtc.hpp"

namespace {
// RCCL is looked up lazily so that single-GPU users never need it.  If the process already has a librccl (PyTorch
// brings its own) that copy is used -- two RCCL builds in one process is asking for trouble.
struct RcclApi {
    void* handle = nullptr;
    decltype(&ncclGetUniqueId) getUniqueId = nullptr;
    decltype(&ncclCommInitRank) commInitRank = nullptr;
    decltype(&ncclAllReduce) allReduce = nullptr;
    decltype(&ncclCommDestroy) commDestroy = nullptr;
    decltype(&ncclCommCount) commCount = nullptr;
    decltype(&ncclGetErrorString) getErrorString = nullptr;
    bool ok = false;
};
RcclApi& rccl_api() {
    static RcclApi r;
    if (r.handle) return r;
    r.handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!r.handle) r.handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!r.handle) r.handle = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!r.handle) return r;
    r.getUniqueId = (decltype(r.getUniqueId)) dlsym(r.handle, "ncclGetUniqueId");
    r.commInitRank = (decltype(r.commInitRank)) dlsym(r.handle, "ncclCommInitRank");
    r.allReduce = (decltype(r.allReduce)) dlsym(r.handle, "ncclAllReduce");
    r.commDestroy = (decltype(r.commDestroy)) dlsym(r.handle, "ncclCommDestroy");
    r.commCount = (decltype(r.commCount)) dlsym(r.handle, "ncclCommCount");
    r.getErrorString = (decltype(r.getErrorString)) dlsym(r.handle, "ncclGetErrorString");
    r.ok = r.getUniqueId && r.commInitRank && r.allReduce && r.commDestroy;
    return r;
}

constexpr double kAvogadro = 6.02214076e23;
constexpr double kBoltz = (1.380649e-23 * kAvogadro) / 1000.0;
enum TimerClass { T_A = 0, T_B = 1, T_OTHER = 2 };
}  // namespace

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

struct vvhip_plan {
    vv::HostPlan hp;
    std::string err;
    bool bound = false;
    vvhip_buffers buf{};
    hipStream_t stream = nullptr;
    double box[3] = {1, 1, 1};
    double acc_scale[vv::NUM_ACC], acc_inv_scale[vv::NUM_ACC];
    int block_threads = 256;       // 64 x tile waves per block, the same for the force provider, kernel A and kernel B
    int grid_cap_a = 2048, grid_cap_b = 1024;   // most blocks per launch (multiples of the CU count): see pick_launch_shape
    int split_chain_waves = 44000;   // systems with at least this many waves (~2.6 M particles) run the chain as its own launch.  Round 4, with two blocks of seven tile
                                     // waves per CU below it (profiles/r04zd_mid_sizes.txt; chain in kernel B | own launch, steps/s): 888 k particles 20.8 | 18.9 k,
                                     // 1.33 M 14.5 | 14.0 k, 1.78 M 11.4 | 11.1 k, 2.66 M 7.38 | 7.37 k, 4.4 M 4.14 | 4.20 k, 8.9 M 2.16 | 2.21 k (round 2 had it at 12 288)
    // The reference's kick kernels add forceExtra ALWAYS (K/middle.cu:11-21, K/velocityVerlet.cu:20-22) and the array is only reset in
    // steps that have a source of extra forces (API:238-240, 316-318): once the cos acceleration is set to 0 in a run without Langevin
    // particles or a field, the last cos force stays in forceExtra and every later kick keeps adding it.  The fused middle step computes
    // extra forces on the fly and leaves the array alone; `cur.fextra_virtual` says the array SHOULD hold the cos force of the last fused
    // step.  vvhip_set_params materialises it (kernel A from the cached cos(kz)) when the acceleration goes to 0, and a fused kick
    // without sources loads the array whenever it is dirty -- the reference's behaviour to the bit, quirk included.
    // The host's cursor through the steps: what a graph capture walks through its steps and puts back (prepare_slot) and what a recovery
    // returns to its snapshot (Recovery::cur)
    struct Cursor {
        int parity = 0;                // which copy of the thermostat state / accumulators the next reduction/consumer pair uses
        uint32_t random_pos = 0;       // prepareRandomNumbers cursor for the plan-driven loops (vvhip_run_*)
        bool fextra_dirty = false;     // forceExtra holds something since the last reset (split entry points)
        bool fextra_virtual = false;   // forceExtra SHOULD hold the cos force of the last fused step (see above)
        // full steps counted since vvhip_bind (the step entry points advance it, a replay advances it by the graph's length): the schedule of
        // the series' rows (vvhip_series_*) and of the removals of the centre-of-mass motion
        long long step_count = 0;
    } cur;
    bool trace = false;            // roctx range + one stderr line per launch group (the reference's setDebugEnabled, VVIntegrator.h:417-419)
    bool fextra_external = false;  // the host asked for the pointer (vvhip_force_extra) and may write to it: never assume zeros
    bool no_moments = false;       // test hook "no_moments": keep the three-launch cos sequence (comparison runs)
    // with an arithmetic work-item layout (HostPlan::per) the kernels compute particle indices instead of loading slot words (test hook "periodic_kernels" = 0:
    // comparison runs).  Kernel A: no slot traffic (1.13 -> 1.0 x the algorithmic bytes) and the next tile's loads in flight during this tile's
    // arithmetic: 133 vs 138 us in sequence at 8.9 M particles (round 2 without the second tile in flight: 113.6 vs 115.7 back to back);
    // test hook "periodic_a" = 0 switches it off
    bool periodic_kernels = true, periodic_a = true, periodic_b = true;
    int shake_mode = 1;            // hydrogen-type constraint clusters: 1 = all constraints of a cluster at once (direct velocity solve, coupled Newton
                                   // for positions), 0 = Gauss-Seidel sweeps by the central lane (OpenMM's iteration; generic kernels) -- VVHIP_SHAKE_MODE
    // Race detection by timing (VVHIP_STALL=us[:period]): every period-th launch of this plan is preceded by a host sleep of `us` microseconds --
    // the GPU drains, anything that was only ordered by the depth of the queue (a fill or copy on another stream, a host read without a
    // synchronisation) lands differently, and the trajectory changes.  tests/test_gpu_stalls.py compares stalled and unstalled runs bit for bit.
    long stall_us = 0, stall_period = 1, stall_count = 0;
    bool acc_store = true;         // kernel A launches of <= 256 blocks store old + new into their accumulator slots instead of atomics (test hook "acc_store" = 0: atomics)
    long long generic_launches[2] = {0, 0};   // kernel A / B launches of this plan (captured ones count once) that ran the generic kernel
    uint32_t generic_flags[2] = {0, 0};       // ... and the last stage set that did (vvhip_generic_launches)
    std::vector<uint32_t> generic_seen[2];    // every stage set that did (VVHIP_WARN_GENERIC prints each once)
    bool rekick = true;            // fused middle step: kick repeated in kernel B instead of a velm store in kernel A (use_rekick)
    // One launch per step (vv_device.inc: "fused step"): kernels A and B of the middle scheme as one launch of co-resident blocks around an
    // in-kernel rendezvous.  `fused` = allowed (vvhip_debug_tune "fused": A/B comparisons and the bit-for-bit tests switch it off);
    // d_rv = the rendezvous words, [2 thermostat parities][NUM_ACC][ACC_SLOTS], uncached; fused_checks = the pairs of stage sets / launch
    // shapes whose kernel and occupancy were looked up and what came of it, fused_last = the entry the last attempt used (-1: none since the
    // cache was emptied).
    bool fused = true;
    // the wait grows when more than blocks / 2^shift blocks needed a second round (test hook "fused_late_shift").  1/16 of the blocks (shift 4,
    // the first choice) let the wait climb where the blocks finish their front unevenly (constraint clusters: 11 units against the best pinned 7);
    // half of them: C3 + HBonds 80.2 -> 81.9 k steps/s, C4 83.1 -> 84.2 k, C5 + HBonds 96.0 -> 97.4 k, C2 150.4 -> 152.4 k, C3 / C5 + 0.4 %
    // (profiles/r05s_late_shift_scan.txt)
    int fused_late_shift = 1;
    int fused_poll_delay = -1;     // >= 0: pins the wait between a block's publish and its first poll round, units of 256 clocks (test hook "fused_poll_delay"); -1: self-tuning
    vv::DevBuf<unsigned long long> d_rv;
    struct FusedCheck { uint32_t a = 0, b = 0; int threads = 0, waves = 0; bool ok = false; };
    FusedCheck fused_checks[4];    // (the classic scheme alternates between the pairs of its two halves)
    int fused_check_next = 0, fused_last = -1;
    long long fused_launches = 0;
    // Recovery from a missed rendezvous (round 6).  The one-launch step needs its blocks resident together; another process's kernel on the
    // device can break that, the blocks' bounded wait then runs out (sticky word [2]) and the step -- and every step enqueued behind it -- has
    // worked on incomplete sums.  The plan-driven loops (vvhip_run_graph / vvhip_run_eager) therefore keep a device-side copy of the physical
    // state from the entry of the first run call that is not yet known to have ended well (positions, correction, velocities, forces, extra
    // forces, both thermostat copies, the random generator's epoch: 116 B per particle in mixed precision, taken only for calls of at least
    // `min_steps` steps) together with the run calls since; the next vvhip_synchronize that finds word [2] raised puts the copy back, pins
    // the plan to two launches per step (bit for bit the same step), repeats the calls and says so once on stderr.  No multi-GPU exchange in
    // between (the other ranks would have to repeat theirs).  `vvhip_debug_tune(plan, "recover", 0)` / VVHIP_RECOVER=0 switch it off.
    struct Recovery {
        bool enabled = true, valid = false, replaying = false, in_loop = false;
        int min_steps = 64;
        vv::DevBuf<void> posq, corr, velm, force, fextra, random;
        vv::DevBuf<vv::NHDevState> nh;
        vv::DevBuf<unsigned long long> epoch;
        Cursor cur;                               // the host's cursor at the snapshot
        struct Run { int kind, nsteps, spg; const void* site; double kt, kd; };
        std::vector<Run> runs;
        long long recoveries = 0;
        vv::DevBuf<unsigned long long> series_cursor;  // the series' device-side row cursor (its schedule, the step counter, is in `cur`)
        bool series_saved = false;
        vv::DevBuf<vv::CmmDevRecord> cmm_rec;     // the counters of the scheduled removals of the centre-of-mass motion
        bool cmm_saved = false;
    } rec;
    // plan-owned device state: every buffer frees itself with the plan (vv_devmem.hpp)
    vv::DevBuf<int2> d_slots;
    vv::DevBuf<int32_t> d_slot_image;
    vv::DevBuf<int32_t> d_slot_rand;
    vv::DevBuf<int32_t> d_slot_big;
    vv::DevBuf<int32_t> d_slot_shake;
    vv::DevBuf<float4> d_slot_shake_param;
    vv::DevBuf<int2> d_slot_vsite;
    vv::DevBuf<double> d_vsite_params;
    vv::DevBuf<int32_t> d_vsite_atom;
    vv::DevBuf<unsigned long long> d_bigacc;
    vv::DevBuf<int2> d_image_pairs;
    vv::DevBuf<void> d_fextra;
    vv::DevBuf<void> d_old_delta;
    vv::DevBuf<void> d_pos_delta;  // used when the caller does not supply one
    vv::DevBuf<void> d_comv;       // per-segment COM velocities handed from kernel A to kernel B
    vv::DevBuf<double> d_slot_m;   // static per-lane RECIP(velm.w) (vv_args.hpp: A_MTAB), filled on the device from velm.w
    vv::DevBuf<double> d_slot_f;   // static per-lane Drude-pair mass fraction (A_MTAB / B_MTAB)
    bool mass_tab_a = false, mass_tab_b = true;   // kernel A / B launches read the tables (defaults follow the build; test hooks "mass_tab_a" / "mass_tab_b" override: comparison runs)
    bool mass_tab_valid = false;   // tables match the bound velm.w (vvhip_bind / vvhip_masses_changed reset it)
    vv::DevBuf<double> d_seg_mass; // static (mass, 1/mass) per COM segment
    vv::DevBuf<int> d_seg_base;    // per wave: COM segments in the waves before it
    vv::DevBuf<double> d_comw;     // per-segment mass-weighted mean of cos(kz) (moment form of the cos perturbation)
    vv::DevBuf<double> d_cosz;     // per-lane cos(2 pi z / Lz) of the current step
    vv::DevBuf<unsigned long long> d_acc;  // [2 parities][NUM_ACC][ACC_SLOTS]
    vv::DevBuf<vv::NHDevState> d_nh;        // [2 parities]
    vv::DevBuf<unsigned long long> d_epoch; // refill counter of the device Gaussian generator
    uint64_t rng_seed = 0;
    // HIP-event timing (eager launches only)
    bool timing = false;
    bool timing_kernels_only = false;   // vvhip_timing_enable(plan, 2): dispatch timestamps of kernels A and B only, nothing added to the stream
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events[3];
    std::vector<hipEvent_t> event_pool;  // events of earlier timing sessions, reused (hipEventCreate per launch would make the host the bottleneck)
    // captured graph for vvhip_run_graph
    // One executable per thermostat parity (the state is double-buffered by step parity, so a graph captured at parity q only
    // replays correctly when the plan is at parity q again).  Captured by vvhip_graph_prepare / the first vvhip_run_graph that
    // needs it, never re-captured while the key (steps, force provider) is unchanged: a run that alternates eager tails and
    // replays keeps both.
    struct GraphSlot {
        hipGraphExec_t exec = nullptr;
        int steps = 0;
        const void* site = nullptr;
        double kt = 0, kd = 0;
        uint32_t random_end = 0;               // prepareRandomNumbers cursor after the graph's last step
        std::vector<int> rows;                 // steps of the graph (1 .. steps) that append a series row: part of the key
        std::vector<int> cmm;                  // steps of the graph (0 .. steps - 1) with a removal of the centre-of-mass motion in front: part of the key
    };
    // (round 6: up to four graph lengths per parity -- a host that replays a short graph in front of a long one keeps both)
    static constexpr int kGraphWays = 4;
    GraphSlot graph[2][kGraphWays];
    int graph_next[2] = {0, 0};
    bool capturing = false;
    // particle sharding over GPUs: RCCL communicator for the accumulator exchange (null = single GPU)
    ncclComm_t comm = nullptr;
    int comm_ranks = 1;
    // ... or the xGMI mailbox (vv_args.hpp: Mailbox): no collective launch, works inside a captured graph
    vv::DevBuf<unsigned long long> mb_local;      // uncached, exported through hipIpc
    vv::DevBuf<unsigned long long*> d_mb_peers;   // device array of the peers' mappings
    vv::DevBuf<unsigned int> d_mb_ctl;
    std::vector<vv::IpcMapping> mb_opened;        // the peers' boxes as mapped here
    int mb_ranks = 0, mb_rank = 0;
    bool mb_on = false;
    // A peer's box lives on THIS device (several ranks sharing one GPU: test set-ups): found out by vvhip_mailbox_connect.  Such ranks'
    // kernels compete for the same CUs, and device-filling grids of polling thermostat waves keep the other process's kernels off
    // the device until the bounded waits run out: every rank then launches on its share of the CUs (shared_device_cap).
    bool mb_shared_device = false;
    int dbg_seq = -1;              // instrumented build: >= 0 while vvhip_debug_step_spans numbers the launches of its steps
    int mb_device_ranks = 1;       // ranks whose boxes live on this device (this one included)
    // Sticky health word in pinned host memory, written by the kernels with system-scope stores when something goes wrong and
    // read by the host without synchronising: [0] a mailbox wait on the peers ran out (the ranks have diverged), [1] a fixed-point
    // accumulator left its range (|sum| x scale >= 2^62: the thermostat would see garbage).  Checked at the entry of the run loops
    // and in vvhip_synchronize / vvhip_status.
    vv::PinnedBuf<unsigned int> h_status;
    unsigned int* d_status = nullptr;             // the same words as the device sees them
    bool launch_shape_forced = false;             // a test hook fixed the launch shape ("block_threads", "grid_cap_a / b"): keep it at bind
    int num_cus = 256;                            // hipDeviceProp_t::multiProcessorCount of the bound device
    vv::DevBuf<vv::ChainLaneBlock> d_lane_const;  // [3] chain constants per temperature group (kernel B's thermostat wave)
    vv::ChainLaneBlock lane_const_host[VVHIP_NUM_TG] = {};
    bool lane_const_valid = false;
    vv::DevBuf<long long> d_dbg_span;
    int dbg_parity = 0;
    vv::DevBuf<long long> d_dbg;                  // instrumented build only (vvhip_debug_timestamps)
    int dbg_block = 0;
    // Drude temperature report (vvhip_drude_temperatures): its tables (HostPlan::report_*) and its own scratch, nothing shared with the step
    vv::DevBuf<int32_t> d_rep_lane_mol;
    vv::DevBuf<double> d_rep_lane_mass;
    vv::DevBuf<double> d_rep_lane_mu;
    vv::DevBuf<double> d_rep_mol_mass;
    vv::DevBuf<int4> d_rep_cross;
    vv::DevBuf<double> d_rep_cross_mu;
    vv::DevBuf<long long> d_rep;                  // [8] result words (vv_args.hpp: REP_*), then [6 per molecule] momentum words
    vv::PinnedBuf<long long> h_rep;               // pinned: the result words as copied back
    long long graph_captures = 0;
    // Series (vvhip_series_*): the rows the steps append on the device, scheduled by cur.step_count
    struct Series {
        bool on = false;
        int interval = 0, capacity = 0, mask = 0;
        long long k0 = 0;                         // row 0 is step interval * k0
        vv::DevBuf<vvhip_series_row> d_rows;      // [capacity + 1]: behind the last row a guard row (vvhip_debug_series_guard)
        vv::DevBuf<unsigned long long> d_cursor;  // [2] rows appended (past capacity too), rows dropped
        vv::DevBuf<long long> d_scratch;          // the report's scratch for the rows (as d_rep), zero between rows
    } series;
    // Removal of the centre-of-mass motion (vvhip_cm_motion_*; vv_dev_cmm.inc), scheduled by step_count: scratch and records of its own,
    // allocated by the first call that needs them
    struct CmMotion {
        bool on = false;
        int frequency = 0;
        vv::DevBuf<long long> d_words;            // [CMM_WORDS] zero between removals
        vv::DevBuf<vv::CmmDevRecord> d_rec;       // [2] the schedule's record; the record of vvhip_remove_cm_motion's one-off calls
        vv::PinnedBuf<double> h_v;                // pinned: the V of a one-off call as copied back
    } cmm;
    // Maxwell-Boltzmann start velocities (vvhip_set_velocities_to_temperature): HostPlan::therm_laneless, uploaded by the first call
    vv::DevBuf<int32_t> d_therm_laneless;
};

static void drop_graphs(vvhip_plan* p) {
    for (auto& row : p->graph)
        for (auto& g : row)
            if (g.exec) { (void) hipGraphExecDestroy(g.exec); g.exec = nullptr; }
}
static int step_done(vvhip_plan* p);
static int step_begin(vvhip_plan* p);
// The steps i = 1 .. steps after step counter c0 that append a series row (empty without a series)
static std::vector<int> series_rows_in(const vvhip_plan* p, long long c0, int steps) {
    std::vector<int> r;
    if (!p->series.on) return r;
    const long long k = p->series.interval;
    for (long long i = k - c0 % k; i <= steps; i += k) r.push_back((int) i);
    return r;
}
// The steps i = 0 .. steps - 1 after step counter c0 with a removal of the centre-of-mass motion in front (empty without a schedule)
static std::vector<int> cmm_steps_in(const vvhip_plan* p, long long c0, int steps) {
    std::vector<int> r;
    if (!p->cmm.on) return r;
    const long long f = p->cmm.frequency;
    for (long long i = (f - c0 % f) % f; i < steps; i += f) r.push_back((int) i);
    return r;
}
// the slot of parity q that holds (or will hold) the graph with this key
static vvhip_plan::GraphSlot& graph_slot(vvhip_plan* p, int q, int steps, const void* site, double kt, double kd, const std::vector<int>& rows,
                                         const std::vector<int>& cmm) {
    auto& row = p->graph[q & 1];
    for (auto& g : row)
        if (g.exec && g.steps == steps && g.site == site && g.kt == kt && g.kd == kd && g.rows == rows && g.cmm == cmm) return g;
    for (auto& g : row)
        if (!g.exec) return g;
    return row[p->graph_next[q & 1]++ % vvhip_plan::kGraphWays];
}

namespace vv { unsigned vv_last_grid_value = 0; }
static unsigned vv_last_grid() { return vv::vv_last_grid_value; }
extern "C" int vvhip_debug_read_accumulators(vvhip_plan* p, double out[4], int zero_after);

namespace {

int fail(vvhip_plan* p, int code, const std::string& msg) {
    if (p) p->err = msg;
    return code;
}
int recover_rendezvous(vvhip_plan* p);
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
int hip_fail(vvhip_plan* p, hipError_t e, const char* what) {
    return fail(p, e == hipErrorNoDevice || e == hipErrorInvalidDevice ? VVHIP_ERR_NO_DEVICE : VVHIP_ERR_HIP,
                std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(p, call)                                         \
    do {                                                         \
        hipError_t e_ = (call);                                  \
        if (e_ != hipSuccess) return hip_fail(p, e_, #call);     \
    } while (0)
#define TRY(x)                       \
    do {                             \
        int rc_ = (x);               \
        if (rc_ != VVHIP_OK) return rc_; \
    } while (0)
#define NEED_BOUND(p)                                                                  \
    do {                                                                               \
        if (!(p)) return VVHIP_ERR_INVALID;                                            \
        if (!(p)->bound) return fail(p, VVHIP_ERR_INVALID, "vvhip_bind has not been called"); \
    } while (0)

size_t sizeof_real(int prec) { return prec == VVHIP_DOUBLE ? 8 : 4; }
size_t sizeof_mixed(int prec) { return prec == VVHIP_SINGLE ? 4 : 8; }

// 2^k fixed-point scale leaving `headroom` x `bound` below 2^62
double pick_scale(double bound, double headroom) {
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

vv::NHConst make_chain(vvhip_plan* p, uint32_t flags);
constexpr int kAccN = vv::NUM_ACC * vv::ACC_SLOTS;
constexpr int kRvCopy = 6 * kAccN;      // rendezvous words of one thermostat parity: up to 6 replicas (vv_device.inc: RV_REPLICAS) of [NUM_ACC][ACC_SLOTS]
// distance between the two parity copies: only the rows in use (4 without the cos moments)
int acc_stride(const vvhip_plan* p) { return (p->hp.params.cos_acceleration != 0 ? vv::NUM_ACC : 4) * vv::ACC_SLOTS; }

vv::KArgs make_args(vvhip_plan* p, uint32_t flags, uint32_t random_index) {
    const vvhip_params& q = p->hp.params;
    vv::KArgs a{};
    a.velm = p->buf.velm;
    a.posq = p->buf.posq;
    a.corr = p->hp.precision == VVHIP_MIXED ? p->buf.posq_correction : nullptr;
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

vv::NHConst make_chain(vvhip_plan* p, uint32_t flags) {
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

struct ScopedTimer {
    vvhip_plan* p;
    int cls;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool on, ranged = false;
    // dispatch = true: the launcher delivers the dispatch's own begin / end timestamps into e0 / e1 (kernels A and B: vv_launch);
    // otherwise the events are recorded around the enqueued work (adds two barrier packets to the stream)
    bool dispatch;
    static hipEvent_t take(vvhip_plan* p) {
        hipEvent_t e = nullptr;
        if (!p->event_pool.empty()) { e = p->event_pool.back(); p->event_pool.pop_back(); }
        else (void) hipEventCreate(&e);
        return e;
    }
    ScopedTimer(vvhip_plan* p_, int cls_, bool dispatch_ = false)
        : p(p_), cls(cls_), on(p_->timing && !p_->capturing && (cls_ != T_OTHER || !p_->timing_kernels_only)), dispatch(dispatch_) {
        if (p->trace && !p->capturing) {
            static const char* names[3] = {"vvhip kernel A (kick / extra forces / sums)", "vvhip kernel B (thermostat / drift / hard wall)", "vvhip other"};
            if (roctx_api().push) { roctx_api().push(names[cls]); ranged = true; }
        }
        if (on) {
            e0 = take(p);
            e1 = take(p);
            if (!dispatch) (void) hipEventRecord(e0, p->stream);
        }
    }
    ~ScopedTimer() {
        if (ranged) roctx_api().pop();
        if (on) {
            if (!dispatch) (void) hipEventRecord(e1, p->stream);
            p->events[cls].emplace_back(e0, e1);
        }
    }
};

// The static mass tables are filled lazily, right in front of the first stage launch that reads them (by then velm.w is what the
// host integrates with); inside a graph capture that would record the fill into every replay, so the capture entry points call this first.
static inline void debug_stall(vvhip_plan* p) {
    if (p->stall_us > 0 && !p->capturing && ++p->stall_count % p->stall_period == 0) usleep((useconds_t) p->stall_us);
}
// Ranks that SHARE a device (test set-ups; found out by vvhip_mailbox_connect) exchange through kernel B's polling thermostat waves: the
// ranks' kernels must be resident together, or the one that got the device first polls until its bounded waits run out while the
// others' launches cannot start (measured round 4, two ranks on one MI355X, 0.44 M / 0.89 M particles: device-filling grids time out
// with either work-item layout, grids of <= half the CUs per rank never do -- tools/probes/mailbox_periodic.sh).  Every rank then
// takes its share of the CUs, one block per CU.  Ranks on devices of their own keep the plan's launch shape.
// A launch that found neither a compiled nor a run-time kernel for its stage set and ran the generic one (15-20 % slower): counted per
// plan (vvhip_generic_launches); VVHIP_WARN_GENERIC=1 also prints one line per plan, kernel and stage set.
void note_generic_launch(vvhip_plan* p, int kernel, uint32_t flags) {
    p->generic_launches[kernel]++;
    // (two stage sets that alternate -- a classic step's halves -- would print on every launch if only the last one were remembered)
    bool seen = false;
    for (uint32_t f : p->generic_seen[kernel]) seen = seen || f == flags;
    if (!seen && p->generic_seen[kernel].size() < 64) p->generic_seen[kernel].push_back(flags);
    p->generic_flags[kernel] = flags;
    static const bool warn = std::getenv("VVHIP_WARN_GENERIC") != nullptr;
    if (warn && !seen) std::fprintf(stderr, "vvhip: kernel %c runs stage set 0x%x on the generic kernel (no compiled specialisation)\n", kernel == 0 ? 'A' : 'B', flags);
}
int shared_device_cap(const vvhip_plan* p, int cap) {
    if (!(p->mb_on && p->mb_shared_device) || p->launch_shape_forced) return cap;
    return std::max(1, std::min(cap, p->num_cus / std::max(1, p->mb_device_ranks)));
}
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
bool periodic_b(const vvhip_plan* p) { return p->hp.per.enabled && p->periodic_kernels && p->periodic_b; }
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

bool cos_on(const vvhip_plan* p) { return p->hp.params.cos_acceleration != 0; }
// How a thermostat application (sums in kernel A -> exchange between the ranks -> chain -> scaling in kernel B) runs for the plan as it
// stands; thermo_mode is the one place that derives it.
// COS_MOMENTS = the cos perturbation in two launches instead of three: kernel A accumulates the group sums as moments of the biased
// velocities next to the bias moment itself, kernel B's inline chain finishes the algebra (vv_args.hpp: the moment bits).  Not with
// molecules larger than a wave or the stand-alone chain launch (long chains, very large systems), which keep the bias -> KE -> scale
// sequence of COS_THREE_LAUNCH (API:252-259).
enum class ThermoMode { NO_NH, PLAIN, COS_MOMENTS, COS_THREE_LAUNCH };
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
    q.rv_late_cur = (unsigned int*) (p->d_rv.get() + 2 * kRvCopy) + vv::ACC_SLOTS * p->cur.parity;
    q.rv_late_prev = (const unsigned int*) (p->d_rv.get() + 2 * kRvCopy) + vv::ACC_SLOTS * (p->cur.parity ^ 1);
    q.fused_late_shift = p->fused_late_shift;
    HIP_TRY(p, vv::launch_fused(p->hp.precision, q, p->block_threads, p->d_rv.get() + p->cur.parity * kRvCopy, p->stream, t.e0, t.e1, &route, nullptr));
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
// No source of extra forces in a step: its kick adds whatever forceExtra still holds (see Cursor::fextra_virtual)
uint32_t stale_fextra(const vvhip_plan* p) { return (p->cur.fextra_dirty || p->fextra_external) ? vv::A_FE_LOAD : 0u; }
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
bool shake_on(const vvhip_plan* p) { return !p->hp.slot_shake.empty(); }
// stage bits of the in-kernel constraints the plan holds: hydrogen-type clusters and / or rigid three-site molecules
uint32_t cons_a(const vvhip_plan* p) { return (p->hp.info.num_shake_clusters > 0 ? vv::A_SHAKE_V : 0u) | (p->hp.info.num_settle_clusters > 0 ? vv::A_SETTLE : 0u) | (p->hp.info.num_general_constraints > 0 ? vv::A_GCONS : 0u); }
uint32_t cons_b(const vvhip_plan* p) { return (p->hp.info.num_shake_clusters > 0 ? vv::B_SHAKE : 0u) | (p->hp.info.num_settle_clusters > 0 ? vv::B_SETTLE : 0u) | (p->hp.info.num_general_constraints > 0 ? vv::B_GCONS : 0u); }
#define NEED_FUSABLE(p)                                                                                                   \
    do {                                                                                                                \
        if (!(p)->hp.info.constraints_fused)                                                                            \
            return fail(p, VVHIP_ERR_UNSUPPORTED, std::string("the System has constraints this backend cannot solve in-kernel") + ((p)->hp.unfused_reason.empty() ? "" : " (" + (p)->hp.unfused_reason + ")") + \
                                                  ": use the split entry points around the host's constraint solver"); \
    } while (0)

}  // namespace

extern "C" {

static void mailbox_release(vvhip_plan* p);

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
    if (p->bound) {
        // The captured graphs bake EVERY caller-owned pointer (make_args): a re-bind that swaps any of them must drop both
        // executables, or vvhip_run_graph would replay kernels on the old arrays without a word.  The stream is not part of a
        // captured node.  Only another velm array invalidates the mass tables (its inverse masses are re-read).
        const vvhip_buffers& o = p->buf;
        const bool same = b->velm == o.velm && b->posq == o.posq && b->posq_correction == o.posq_correction && b->force == o.force &&
                          b->pos_delta == o.pos_delta && b->random == o.random && b->random_size == o.random_size;
        if (b->velm != o.velm) p->mass_tab_valid = false;
        if (!same || p->series.on || p->cmm.on) drop_graphs(p);      // (a series row and a scheduled removal read velm through their captured arguments too)
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
    // (+ ACC_SLOTS words: the two rows of "polled twice" flags; + 8: the "a rendezvous has failed" word behind them, vv_device.inc: rv_dead_word)
    HIP_TRY(p, vv::zeros(p->d_rv, (size_t) (2 * kRvCopy + vv::ACC_SLOTS + 8) * sizeof(unsigned long long), p->stream, true));
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
    if (p->box[0] == box[0] && p->box[1] == box[1] && p->box[2] == box[2]) return VVHIP_OK;      // hosts re-send it every step
    for (int i = 0; i < 3; i++) p->box[i] = box[i];
    drop_graphs(p);                                  // the box is baked into the captured kernel arguments
    return VVHIP_OK;
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

// ------------------------------------------------------------------------------------------ fused path
int vvhip_step_middle_phases(const vvhip_plan* p) {
    if (!p) return VVHIP_ERR_INVALID;
    const ThermoMode mode = thermo_mode(p);
    return mode == ThermoMode::NO_NH ? 1 : mode == ThermoMode::COS_THREE_LAUNCH ? 3 : 2;
}

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
// Does vvhip_step_middle take the one-launch step for this plan as it stands?  (The kernel itself is looked up at the first step; a pair
// of stage sets already found wanting says so here.)
static bool fused_active(const vvhip_plan* p) {
    if (!p->bound || !p->hp.params.use_middle_scheme || !p->hp.info.constraints_fused || !fused_state_ok(p) || thermo_mode(p) == ThermoMode::COS_THREE_LAUNCH) return false;
    return p->fused_last < 0 || p->fused_checks[p->fused_last].ok;
}

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

// Element-wise int64 sum of the accumulators of `phase` over all ranks, on the plan's stream (ncclSum is exact on
// integers, so every rank continues with identical bits).  No-op without a communicator.
static int exchange_accumulators(vvhip_plan* p, int phase) {
    if (use_mailbox(p)) return VVHIP_OK;   // kernel B exchanges the totals itself
    if (!p->comm) return VVHIP_OK;      // a 1-rank communicator still issues the collective (exercises the path on one GPU)
    void* ptr = nullptr;
    int32_t count = 0;
    int rc = vvhip_accumulators(p, phase, &ptr, &count);
    if (rc != VVHIP_OK) return rc;
    ScopedTimer t(p, T_OTHER);
    ncclResult_t e = rccl_api().allReduce(ptr, ptr, (size_t) count, ncclInt64, ncclSum, p->comm, p->stream);
    if (e != ncclSuccess) return fail(p, VVHIP_ERR_HIP, std::string("ncclAllReduce: ") + (rccl_api().getErrorString ? rccl_api().getErrorString(e) : "error"));
    return VVHIP_OK;
}

// ---- A thermostat application with the stages that ride on it, as data: what every step entry point launches, and what
// vvhip_debug_fused_flags reports.  Phase k < phases - 1 is a launch of kernel A (through run_ke where it ends in the sums: molecules
// larger than a wave split it), the last phase the chain and kernel B (run_chain_and_b), with the ranks' exchange between the phases;
// without Nose-Hoover particles the one phase is kernel A, then kernel B, whichever has stages.
struct ThermoApp {
    ThermoMode mode = ThermoMode::NO_NH;
    int phases = 1;
    struct Launch { uint32_t flags = 0; bool sums = false; } a[2];
    uint32_t b = 0;
    bool with_bias = false;                     // the stand-alone chain launch also finishes the bias moment
    bool one_launch = false;                    // (fused_a, fused_b) can be one launch (run_fused): the same sets without the hand-over bits
    uint32_t fused_a = 0, fused_b = 0;
    bool fe_virtual = false;                    // kernel A forms the cos force on the fly, and nothing else: see Cursor::fextra_virtual
};
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
static int run_application_fused(vvhip_plan* p, const ThermoApp& t, uint32_t random_index, bool* taken) {
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
static ThermoApp middle_application(const vvhip_plan* p) {
    const ThermoMode mode = thermo_mode(p);
    // with sources of extra forces they are formed on the fly and the forceExtra array is out of date from here on
    const uint32_t ex = extra_flags(p);
    uint32_t kick = vv::A_KICK_FULL | (ex ? ex : stale_fextra(p)) | cons_a(p);
    // (without NH particles the kick caches cos(kz) all the same: vvhip_set_params rebuilds the stale forceExtra from it)
    if (mode == ThermoMode::NO_NH && cos_on(p)) kick |= vv::A_CZ_STORE;
    return compose_application(mode, kick, vv::B_DRIFT_MIDDLE | tail_flags(p) | cons_b(p), use_rekick(p));
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

// NH half-step used by the classic scheme (API:295-304, 327-336); `b_extra` is fused into the scaling kernel.
static int nh_half(vvhip_plan* p, uint32_t a_first, uint32_t random_index, uint32_t b_extra) {
    return run_application(p, compose_application(thermo_mode(p), a_first, b_extra, false), random_index);
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
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "Drude temperature report: not inside a graph capture");
    TRY(settle_recovery(p));
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
    a.rows = S.d_rows.get(); a.cursor = S.d_cursor.get(); a.capacity = S.capacity;
    for (int k = 0; k < 3; k++) a.box[k] = p->box[k];
    a.cos_acceleration = p->hp.params.cos_acceleration;
    HIP_TRY(p, vv::launch_series_append(a, p->grid_cap_a, p->stream));
    return VVHIP_OK;
}
// A full step has been enqueued (or captured): count it, and append a row when it is due.
static int step_done(vvhip_plan* p) {
    p->cur.step_count++;
    if (p->series.on && p->cur.step_count % p->series.interval == 0) return series_row(p);
    return VVHIP_OK;
}

// ------------------------------------------------------------------------------------------ centre-of-mass motion (vvhip_cm_motion_*)
static bool cmm_sharded(const vvhip_plan* p) { return p->hp.shard_begin != 0 || p->hp.shard_end != p->hp.num_atoms; }
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
// A full step is about to be enqueued (or captured): the removal in front of it when its index is due.  The one hook of every entry point
// that starts a step (next to step_done, which ends it).
static int step_begin(vvhip_plan* p) {
    if (p->cmm.on && p->cur.step_count % p->cmm.frequency == 0) return cmm_enqueue(p, 0);
    return VVHIP_OK;
}
int vvhip_cm_motion_start(vvhip_plan* p, int32_t frequency) {
    if (!p) return VVHIP_ERR_INVALID;
    if (frequency < 1) return fail(p, VVHIP_ERR_INVALID, "centre-of-mass motion: frequency must be >= 1 step");
    if (!p->hp.has_cm_motion_remover)
        return fail(p, VVHIP_ERR_INVALID, "centre-of-mass motion: the plan was described without a CMMotionRemover (has_cm_motion_remover = 0), so the thermostat's "
                                          "degrees of freedom (DOF) still count the 3 of the centre of mass; describe the System with the remover to schedule removals");
    if (cmm_sharded(p))
        return fail(p, VVHIP_ERR_UNSUPPORTED, "centre-of-mass motion: a sharded plan holds a part of the momentum only (summing over the ranks is not implemented)");
    NEED_BOUND(p);
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "centre-of-mass motion: not inside a graph capture");
    TRY(settle_recovery(p));
    HIP_TRY(p, hipStreamSynchronize(p->stream));      // (removals of a schedule before may still be in flight)
    TRY(cmm_ensure(p));
    HIP_TRY(p, hipMemsetAsync(p->cmm.d_rec.get(), 0, sizeof(vv::CmmDevRecord), p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    drop_graphs(p);
    p->cmm.on = true; p->cmm.frequency = frequency;
    return VVHIP_OK;
}
int vvhip_cm_motion_stop(vvhip_plan* p) {
    if (!p) return VVHIP_ERR_INVALID;
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "centre-of-mass motion: not inside a graph capture");
    if (!p->cmm.on) return VVHIP_OK;
    TRY(settle_recovery(p));
    if (p->bound) HIP_TRY(p, hipStreamSynchronize(p->stream));
    p->cmm.on = false; p->cmm.frequency = 0;
    drop_graphs(p);
    return VVHIP_OK;
}
int vvhip_remove_cm_motion(vvhip_plan* p, double v_removed[3]) {
    if (!p) return VVHIP_ERR_INVALID;
    if (cmm_sharded(p))
        return fail(p, VVHIP_ERR_UNSUPPORTED, "centre-of-mass motion: a sharded plan holds a part of the momentum only (summing over the ranks is not implemented)");
    NEED_BOUND(p);
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "centre-of-mass motion: not inside a graph capture");
    TRY(settle_recovery(p));
    TRY(cmm_ensure(p));
    TRY(cmm_enqueue(p, 1));
    HIP_TRY(p, hipMemcpyAsync(p->cmm.h_v.get(), p->cmm.d_rec.get()[1].last_v, 3 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    if (std::isnan(p->cmm.h_v[0]))      // (what the subtract kernel records for a removal it skipped)
        return fail(p, VVHIP_ERR_OVERFLOW, "centre-of-mass motion: a momentum term is NaN or beyond the fixed-point range; nothing was subtracted");
    if (v_removed) std::memcpy(v_removed, p->cmm.h_v.get(), 3 * sizeof(double));
    return VVHIP_OK;
}
int vvhip_cm_motion_read(vvhip_plan* p, vvhip_cm_motion_record* out) {
    if (!p || !out) return VVHIP_ERR_INVALID;
    vvhip_cm_motion_record r{};
    r.frequency = p->cmm.on ? p->cmm.frequency : 0;
    r.total_mass = p->hp.cm_total_mass;
    if (p->bound && p->cmm.d_rec) {
        if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "centre-of-mass motion: not inside a graph capture");
        TRY(settle_recovery(p));                        // (a repaired run redoes its removals first)
        HIP_TRY(p, hipStreamSynchronize(p->stream));
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
    if (remove_cm && cmm_sharded(p))
        return fail(p, VVHIP_ERR_UNSUPPORTED, "centre-of-mass motion: a sharded plan holds a part of the momentum only (summing over the ranks is not implemented)");
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
    if (remove_cm) {
        TRY(cmm_enqueue(p, 1));
        HIP_TRY(p, hipMemcpyAsync(p->cmm.h_v.get(), p->cmm.d_rec.get()[1].last_v, 3 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    }
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    if (remove_cm) {
        if (std::isnan(p->cmm.h_v[0]))
            return fail(p, VVHIP_ERR_OVERFLOW, "centre-of-mass motion: a momentum term is NaN or beyond the fixed-point range; nothing was subtracted");
        r.cm_removed = 1;
        std::memcpy(r.v_removed, p->cmm.h_v.get(), 3 * sizeof(double));
    }
    if (out) *out = r;
    return VVHIP_OK;
}
static void series_release(vvhip_plan* p) {
    vvhip_plan::Series& S = p->series;
    S.d_rows.reset(); S.d_cursor.reset(); S.d_scratch.reset();
    S.on = false; S.interval = S.capacity = S.mask = 0; S.k0 = 0;
}
static constexpr int kGuardByte = 0xA5;
int vvhip_series_start(vvhip_plan* p, int32_t interval, int32_t capacity, int32_t mask) {
    if (!p) return VVHIP_ERR_INVALID;
    if (interval < 1) return fail(p, VVHIP_ERR_INVALID, "series: interval must be >= 1 step");
    if (capacity < 1) return fail(p, VVHIP_ERR_INVALID, "series: capacity must be >= 1 row");
    if (mask == 0 || (mask & ~(VVHIP_SERIES_DRUDE | VVHIP_SERIES_THERMOSTAT)))
        return fail(p, VVHIP_ERR_INVALID, "series: mask must be a non-empty set of VVHIP_SERIES_DRUDE / VVHIP_SERIES_THERMOSTAT");
    if ((mask & VVHIP_SERIES_DRUDE) && !p->hp.report_unsupported.empty())
        return fail(p, VVHIP_ERR_UNSUPPORTED, "Drude temperature report: " + p->hp.report_unsupported);
    NEED_BOUND(p);
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "series: not inside a graph capture");
    TRY(settle_recovery(p));
    HIP_TRY(p, hipStreamSynchronize(p->stream));      // (rows of a series before may still be in flight)
    series_release(p);
    drop_graphs(p);
    vvhip_plan::Series& S = p->series;
    const size_t row_bytes = sizeof(vvhip_series_row), scratch = (8 + 6 * p->hp.report_mol_mass.size()) * sizeof(long long);
    HIP_TRY(p, vv::zeros(S.d_rows, ((size_t) capacity + 1) * row_bytes, p->stream));
    HIP_TRY(p, hipMemsetAsync((char*) S.d_rows.get() + (size_t) capacity * row_bytes, kGuardByte, row_bytes, p->stream));
    HIP_TRY(p, vv::zeros(S.d_cursor, 2 * sizeof(unsigned long long), p->stream));
    HIP_TRY(p, vv::zeros(S.d_scratch, scratch, p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    S.on = true; S.interval = interval; S.capacity = capacity; S.mask = mask;
    S.k0 = p->cur.step_count / interval + 1;               // the first multiple of interval after the current step
    return VVHIP_OK;
}
int vvhip_series_read(vvhip_plan* p, vvhip_series_row* rows_out, int32_t max_rows, int32_t* n_rows, int64_t* first_step, int64_t* dropped,
                      int32_t reset) {
    NEED_BOUND(p);
    if (max_rows < 0 || (max_rows > 0 && !rows_out)) return VVHIP_ERR_INVALID;
    vvhip_plan::Series& S = p->series;
    if (!S.on) return fail(p, VVHIP_ERR_INVALID, "series: none started (vvhip_series_start)");
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "series: not inside a graph capture");
    TRY(settle_recovery(p));                            // (a repaired run rewrites its rows first)
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    unsigned long long cur[2];
    HIP_TRY(p, hipMemcpy(cur, S.d_cursor.get(), sizeof(cur), hipMemcpyDeviceToHost));
    const long long n = (long long) std::min<unsigned long long>(cur[0], (unsigned long long) S.capacity);
    const long long copy = std::min<long long>(n, max_rows);
    if (copy > 0) HIP_TRY(p, hipMemcpy(rows_out, S.d_rows.get(), (size_t) copy * sizeof(vvhip_series_row), hipMemcpyDeviceToHost));
    if (n_rows) *n_rows = (int32_t) n;
    if (first_step) *first_step = (int64_t) S.interval * S.k0;
    if (dropped) *dropped = (int64_t) cur[1];
    if (reset) {
        HIP_TRY(p, hipMemsetAsync(S.d_cursor.get(), 0, 2 * sizeof(unsigned long long), p->stream));
        HIP_TRY(p, hipStreamSynchronize(p->stream));
        S.k0 += (long long) cur[0];                     // (dropped rows included: their steps are gone)
    }
    return VVHIP_OK;
}
int vvhip_series_stop(vvhip_plan* p) {
    if (!p) return VVHIP_ERR_INVALID;
    if (p->capturing) return fail(p, VVHIP_ERR_INVALID, "series: not inside a graph capture");
    if (!p->series.on) return VVHIP_OK;
    TRY(settle_recovery(p));
    if (p->bound) HIP_TRY(p, hipStreamSynchronize(p->stream));
    series_release(p);
    drop_graphs(p);
    return VVHIP_OK;
}
int vvhip_series_info(const vvhip_plan* p, vvhip_series_layout* out) {
    if (!p || !out) return VVHIP_ERR_INVALID;
    vvhip_series_layout r{};
    r.row_bytes = (int32_t) sizeof(vvhip_series_row);
    r.off_drude_raw = (int32_t) offsetof(vvhip_series_row, drude_raw);
    r.off_nh = (int32_t) offsetof(vvhip_series_row, nh);
    r.off_box = (int32_t) offsetof(vvhip_series_row, box);
    r.active = p->series.on; r.interval = p->series.interval; r.capacity = p->series.capacity; r.mask = p->series.mask;
    r.steps = p->cur.step_count;
    r.graph_captures = p->graph_captures;
    *out = r;
    return VVHIP_OK;
}
int vvhip_debug_series_guard(vvhip_plan* p, int32_t* intact) {
    NEED_BOUND(p);
    if (!intact) return VVHIP_ERR_INVALID;
    if (!p->series.on) return fail(p, VVHIP_ERR_INVALID, "series: none started (vvhip_series_start)");
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    unsigned char g[sizeof(vvhip_series_row)];
    HIP_TRY(p, hipMemcpy(g, p->series.d_rows.get() + p->series.capacity, sizeof(g), hipMemcpyDeviceToHost));
    *intact = 1;
    for (unsigned char c : g) if (c != kGuardByte) *intact = 0;
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
    if (p->d_rv) HIP_TRY(p, hipMemsetAsync(p->d_rv.get() + 2 * kRvCopy + vv::ACC_SLOTS, 0, 8 * sizeof(unsigned long long), p->stream));      // "a rendezvous has failed" (vv_device.inc: rv_dead_word)
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

// ---- recovery from a missed rendezvous (vvhip_plan::Recovery)
static size_t rec_bytes(const vvhip_plan* p, int which) {
    const vv::HostPlan& hp = p->hp;
    const size_t nloc = (size_t) (hp.shard_end - hp.shard_begin), rs = sizeof_real(hp.precision), ms = sizeof_mixed(hp.precision);
    switch (which) {
        case 0: return nloc * 4 * rs;                                  // posq
        case 1: return p->buf.posq_correction ? nloc * 4 * rs : 0;     // posqCorrection
        case 2: return nloc * 4 * ms;                                  // velm
        case 3: return (size_t) hp.padded_num_atoms * 3 * 8;           // force (planar int64)
        case 4: return nloc * 3 * rs;                                  // forceExtra
        default: return p->hp.has_ld ? (size_t) p->buf.random_size * sizeof(float4) : 0;      // the Langevin normals in use
    }
}
static int recovery_snapshot(vvhip_plan* p) {
    vvhip_plan::Recovery& r = p->rec;
    vv::DevBuf<void>* dst[6] = {&r.posq, &r.corr, &r.velm, &r.force, &r.fextra, &r.random};
    const void* src[6] = {p->buf.posq, p->buf.posq_correction, p->buf.velm, p->buf.force, p->d_fextra.get(), p->buf.random};
    for (int i = 0; i < 6; i++) {
        const size_t n = rec_bytes(p, i);
        if (!n) continue;
        HIP_TRY(p, dst[i]->ensure(n));      // (a re-bind may have brought a larger random buffer)
        HIP_TRY(p, hipMemcpyAsync(dst[i]->get(), src[i], n, hipMemcpyDeviceToDevice, p->stream));
    }
    HIP_TRY(p, r.nh.ensure(2 * sizeof(vv::NHDevState)));
    HIP_TRY(p, r.epoch.ensure(sizeof(unsigned long long)));
    HIP_TRY(p, hipMemcpyAsync(r.nh.get(), p->d_nh.get(), 2 * sizeof(vv::NHDevState), hipMemcpyDeviceToDevice, p->stream));
    HIP_TRY(p, hipMemcpyAsync(r.epoch.get(), p->d_epoch.get(), sizeof(unsigned long long), hipMemcpyDeviceToDevice, p->stream));
    r.cur = p->cur;
    r.series_saved = p->series.on;                  // (a series cannot start or stop while the snapshot is unverified: both settle it first)
    if (r.series_saved) {
        HIP_TRY(p, r.series_cursor.ensure(2 * sizeof(unsigned long long)));
        HIP_TRY(p, hipMemcpyAsync(r.series_cursor.get(), p->series.d_cursor.get(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, p->stream));
    }
    r.cmm_saved = (bool) p->cmm.d_rec;          // (a schedule cannot start or stop while the snapshot is unverified either)
    if (r.cmm_saved) {
        HIP_TRY(p, r.cmm_rec.ensure(sizeof(vv::CmmDevRecord)));
        HIP_TRY(p, hipMemcpyAsync(r.cmm_rec.get(), p->cmm.d_rec.get(), sizeof(vv::CmmDevRecord), hipMemcpyDeviceToDevice, p->stream));
    }
    r.runs.clear();
    r.valid = true;
    return VVHIP_OK;
}
// At the entry of a plan-driven run call: take the snapshot if there is none and the call is worth one; remember the call.
static int recovery_note_run(vvhip_plan* p, int kind, int nsteps, int spg, const void* site, double kt, double kd) {
    vvhip_plan::Recovery& r = p->rec;
    if (r.replaying || p->capturing || nsteps <= 0) return VVHIP_OK;
    if (!r.valid) {
        if (!r.enabled || nsteps < r.min_steps || !fused_state_ok(p) || p->comm || p->mb_on) return VVHIP_OK;
        TRY(recovery_snapshot(p));
    }
    r.runs.push_back({kind, nsteps, spg, site, kt, kd});
    return VVHIP_OK;
}
namespace {
int recover_rendezvous(vvhip_plan* p) {
    vvhip_plan::Recovery& r = p->rec;
    long long steps = 0;
    for (const auto& run : r.runs) steps += run.nsteps;
    std::fprintf(stderr, "libvvhip: the one-launch step's blocks did not meet within 0.2 s (another process's kernels on the device?): the last %lld step(s) "
                         "are repeated from the plan's snapshot with two launches per step, and the plan keeps two launches from here on\n", steps);
    void* src[6] = {r.posq.get(), r.corr.get(), r.velm.get(), r.force.get(), r.fextra.get(), r.random.get()};
    void* dst[6] = {p->buf.posq, p->buf.posq_correction, p->buf.velm, p->buf.force, p->d_fextra.get(), const_cast<void*>(p->buf.random)};
    for (int i = 0; i < 6; i++) {
        const size_t n = rec_bytes(p, i);
        if (n && src[i]) HIP_TRY(p, hipMemcpyAsync(dst[i], src[i], n, hipMemcpyDeviceToDevice, p->stream));
    }
    HIP_TRY(p, hipMemcpyAsync(p->d_nh.get(), r.nh.get(), 2 * sizeof(vv::NHDevState), hipMemcpyDeviceToDevice, p->stream));
    HIP_TRY(p, hipMemcpyAsync(p->d_epoch.get(), r.epoch.get(), sizeof(unsigned long long), hipMemcpyDeviceToDevice, p->stream));
    // both accumulator copies are zero between steps; whatever the failed steps left in them goes
    HIP_TRY(p, hipMemsetAsync(p->d_acc.get(), 0, 2 * kAccN * sizeof(unsigned long long), p->stream));
    if (p->d_bigacc) HIP_TRY(p, hipMemsetAsync(p->d_bigacc.get(), 0, (size_t) p->hp.num_big * 4 * sizeof(unsigned long long), p->stream));
    HIP_TRY(p, hipMemsetAsync(p->d_rv.get() + 2 * kRvCopy + vv::ACC_SLOTS, 0, 8 * sizeof(unsigned long long), p->stream));
    // (with the step counter: the series' rows of the failed steps are written again, at the same places, by the repeat)
    p->cur = r.cur;
    if (r.series_saved && p->series.on)
        HIP_TRY(p, hipMemcpyAsync(p->series.d_cursor.get(), r.series_cursor.get(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, p->stream));
    // ... and so are the removals of the centre-of-mass motion, at the same steps (the schedule follows the step counter): their counters go
    // back with it (the scratch words are zero between removals whatever the failed steps computed)
    if (r.cmm_saved && p->cmm.d_rec)
        HIP_TRY(p, hipMemcpyAsync(p->cmm.d_rec.get(), r.cmm_rec.get(), sizeof(vv::CmmDevRecord), hipMemcpyDeviceToDevice, p->stream));
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
        rc = run.kind == 0 ? vvhip_run_graph(p, run.nsteps, run.spg, run.site, run.kt, run.kd) : vvhip_run_eager(p, run.nsteps, run.site, run.kt, run.kd);
        if (rc != VVHIP_OK) break;
    }
    r.replaying = false;
    if (rc != VVHIP_OK) return rc;
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    return check_exchange_health(p);
}
}

// One step of the plan-driven loops (vvhip_run_graph / vvhip_run_eager): force provider + fused step, in the scheme's order.
static int plan_step(vvhip_plan* p, const void* site, double k_tether, double k_drude, bool refill) {
    uint32_t ri = 0;
    TRY(next_random_slice(p, &ri, refill));
    if (p->hp.params.use_middle_scheme) {
        if (site) TRY(vvhip_synth_tether_force(p, site, k_tether, k_drude));
        return vvhip_step_middle(p, ri);
    }
    TRY(vvhip_step_vv_first(p));
    if (site) TRY(vvhip_synth_tether_force(p, site, k_tether, k_drude));
    return vvhip_step_vv_second(p, ri);
}

// Capture + instantiate + upload the graph of `steps_per_graph` steps for thermostat parity `q`, unless that slot already holds it.
// Nothing is launched: the physical state is untouched.
// The graph is captured at step counter c0 (where its replays start): its series rows sit at the steps series_rows_in(c0) names.
static int prepare_slot(vvhip_plan* p, int q, int steps_per_graph, const void* site, double k_tether, double k_drude, long long c0,
                        vvhip_plan::GraphSlot** out = nullptr) {
    hipStream_t s = p->stream;
    TRY(ensure_mass_table(p));                       // a one-off fill must not be recorded into the replayed graph
    const std::vector<int> rows = series_rows_in(p, c0, steps_per_graph), cmm = cmm_steps_in(p, c0, steps_per_graph);
    vvhip_plan::GraphSlot& g = graph_slot(p, q, steps_per_graph, site, k_tether, k_drude, rows, cmm);
    if (out) *out = &g;
    if (g.exec && g.steps == steps_per_graph && g.site == site && g.kt == k_tether && g.kd == k_drude && g.rows == rows && g.cmm == cmm) return VVHIP_OK;
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
    for (int i = 0; i < steps_per_graph && rc == VVHIP_OK; i++) rc = plan_step(p, site, k_tether, k_drude, i == 0 && p->hp.has_ld);
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
    g.steps = steps_per_graph; g.site = site; g.kt = k_tether; g.kd = k_drude; g.rows = rows; g.cmm = cmm;
    p->graph_captures++;
    return VVHIP_OK;
}

// Both parities' executables, ready to launch.  Hosts call this outside any timed region (bench.py does, after its warm-up);
// vvhip_run_graph prepares the slot of the current parity itself when it is missing.
int vvhip_graph_prepare(vvhip_plan* p, int steps_per_graph, const void* site, double k_tether, double k_drude) {
    NEED_BOUND(p);
    if (steps_per_graph < 1) return VVHIP_ERR_INVALID;
    if (steps_per_graph % 2) steps_per_graph += 1;   // the thermostat double-buffers by step parity: a graph must hold an even number of steps
    if (!p->stream) return fail(p, VVHIP_ERR_INVALID, "graph capture needs a non-null stream in vvhip_buffers.stream");
    TRY(prepare_slot(p, p->cur.parity, steps_per_graph, site, k_tether, k_drude, p->cur.step_count));
    return prepare_slot(p, p->cur.parity ^ 1, steps_per_graph, site, k_tether, k_drude, p->cur.step_count);
}

int vvhip_run_graph(vvhip_plan* p, int nsteps, int steps_per_graph, const void* site, double k_tether, double k_drude) {
    NEED_BOUND(p);
    if (nsteps < 0 || steps_per_graph < 1) return VVHIP_ERR_INVALID;
    if (steps_per_graph % 2) steps_per_graph += 1;
    TRY(check_exchange_health(p));
    hipStream_t s = p->stream;
    if (!s) return fail(p, VVHIP_ERR_INVALID, "graph capture needs a non-null stream in vvhip_buffers.stream");
    TRY(recovery_note_run(p, 0, nsteps, steps_per_graph, site, k_tether, k_drude));
    struct InLoop { vvhip_plan* p; bool was; InLoop(vvhip_plan* q) : p(q), was(q->rec.in_loop) { p->rec.in_loop = true; } ~InLoop() { p->rec.in_loop = was; } } in_loop(p);
    const bool middle = p->hp.params.use_middle_scheme;
    // classic scheme (API:272-338): every step is first half -> forces -> second half, and the first half needs the forces of the
    // current positions; they are (re)computed once per call here, outside the replayed part
    if (!middle && site && nsteps > 0) TRY(vvhip_synth_tether_force(p, site, k_tether, k_drude));
    int done = 0;
    if (nsteps >= steps_per_graph) {
        vvhip_plan::GraphSlot* g = nullptr;
        TRY(prepare_slot(p, p->cur.parity, steps_per_graph, site, k_tether, k_drude, p->cur.step_count, &g));     // no-op when the slot of this parity is ready
        for (; done + steps_per_graph <= nsteps; done += steps_per_graph) {
            // with a series the replays' rows fall on other steps of the graph as the counter moves on: the graph whose rows fit
            // (at most two when the interval and the graph's length divide one another; otherwise the cache may capture again)
            // (the same for the steps that carry a removal of the centre-of-mass motion)
            if (done > 0 && ((p->series.on && series_rows_in(p, p->cur.step_count, steps_per_graph) != g->rows) ||
                             (p->cmm.on && cmm_steps_in(p, p->cur.step_count, steps_per_graph) != g->cmm)))
                TRY(prepare_slot(p, p->cur.parity, steps_per_graph, site, k_tether, k_drude, p->cur.step_count, &g));
            HIP_TRY(p, hipGraphLaunch(g->exec, s));
            p->cur.step_count += steps_per_graph;
        }
        p->cur.random_pos = g->random_end;               // an even number of steps: the parity is where it was
        if (!middle && extra_flags(p)) p->cur.fextra_dirty = true;
        if (middle && middle_application(p).fe_virtual) p->cur.fextra_virtual = true;    // what the replayed steps' phase 0 would have set
    }
    for (; done < nsteps; done++) TRY(plan_step(p, site, k_tether, k_drude, false));
    return VVHIP_OK;
}

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
    HIP_TRY(p, p->d_dbg.ensure(128 * sizeof(long long)));
    HIP_TRY(p, hipMemsetAsync(p->d_dbg.get(), 0, 128 * sizeof(long long), p->stream));
    p->dbg_block = block;
    const int parity = p->cur.parity;
    int rc = (flags & 0x80000000u) ? run_a(p, flags & 0x7FFFFFFFu, 0) : run_b(p, flags);
    p->cur.parity = parity;
    if (rc != VVHIP_OK) return rc;
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    HIP_TRY(p, hipMemcpy(out, p->d_dbg.get(), 128 * sizeof(long long), hipMemcpyDeviceToHost));
    return VVHIP_OK;
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
    HIP_TRY(p, p->d_dbg.ensure(128 * sizeof(long long)));
    HIP_TRY(p, hipMemsetAsync(p->d_dbg.get(), 0, 128 * sizeof(long long), p->stream));
    p->dbg_block = block;
    bool taken = false;
    if (p->hp.params.use_middle_scheme && p->hp.info.constraints_fused) TRY(run_application_fused(p, middle_application(p), 0, &taken));
    if (!taken) return fail(p, VVHIP_ERR_UNSUPPORTED, "the plan does not take the one-launch step");
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    HIP_TRY(p, hipMemcpy(out, p->d_dbg.get(), 128 * sizeof(long long), hipMemcpyDeviceToHost));
    return VVHIP_OK;
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
    const size_t per = (size_t) 4096 * 8 * 2;
    HIP_TRY(p, p->d_dbg_span.ensure(6 * per * sizeof(long long)));
    HIP_TRY(p, hipMemsetAsync(p->d_dbg_span.get(), 0, 6 * per * sizeof(long long), p->stream));
    const int parity = p->cur.parity;
    int rc = VVHIP_OK;
    for (int i = 0; i < reps && rc == VVHIP_OK; i++) { p->cur.parity = parity; p->dbg_parity = i & 1; rc = kernel == 0 ? run_a(p, flags, 0) : run_b(p, flags); }
    p->cur.parity = parity;
    const int last = (reps - 1) & 1;
    p->dbg_parity = 0;
    if (rc != VVHIP_OK) return rc;
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    std::vector<long long> h(2 * per);
    HIP_TRY(p, hipMemcpy(h.data(), p->d_dbg_span.get(), h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    // the grid size is not known here: the launch of parity q used rows [q * grid, (q+1) * grid); find them by scanning non-zero pairs
    std::vector<long long> in[2], ex[2];
    std::vector<int> blk;
    const int grid = (int) vv_last_grid();
    for (int q = 0; q < 2; q++)
        for (size_t r = 0; r < (size_t) grid * 8; r++) {
            const long long a0 = h[(((size_t) q * 4096) * 8 + r) * 2], a1 = h[(((size_t) q * 4096) * 8 + r) * 2 + 1];
            if (a0 && a1) { in[q].push_back(a0); ex[q].push_back(a1); if (q == ((reps - 1) & 1)) blk.push_back((int) (r / 8)); }
        }
    if (in[0].empty() || in[1].empty()) return fail(p, VVHIP_ERR_INVALID, "no stamps recorded");
    const int L = last, P = 1 - last;
    const long long first_in = *std::min_element(in[L].begin(), in[L].end()), last_out = *std::max_element(ex[L].begin(), ex[L].end());
    const long long prev_out = *std::max_element(ex[P].begin(), ex[P].end());
    std::vector<long long> rel, life;
    for (size_t k = 0; k < in[L].size(); k++) { rel.push_back(in[L][k] - first_in); life.push_back(ex[L][k] - in[L][k]); }
    size_t worst = 0;
    for (size_t k = 0; k < in[L].size(); k++) if (ex[L][k] > ex[L][worst]) worst = k;
    out[6] = (double) blk[worst]; out[7] = (double) (in[L][worst] - first_in) * 10.0;
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
    const size_t per = (size_t) 4096 * 8 * 2;
    HIP_TRY(p, p->d_dbg_span.ensure(6 * per * sizeof(long long)));
    TRY(ensure_mass_table(p));
    for (int i = 0; i < nsteps - 2; i++) TRY(plan_step(p, site, k_tether, k_drude, false));      // warm: same launches, rows overwritten below
    HIP_TRY(p, hipMemsetAsync(p->d_dbg_span.get(), 0, 6 * per * sizeof(long long), p->stream));
    p->dbg_seq = 0;
    int rc = VVHIP_OK;
    const long long fused_before = p->fused_launches;
    for (int i = 0; i < 2 && rc == VVHIP_OK; i++) rc = plan_step(p, site, k_tether, k_drude, false);
    p->dbg_seq = -1;
    if (rc != VVHIP_OK) return rc;
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    std::vector<long long> h(6 * per);
    HIP_TRY(p, hipMemcpy(h.data(), p->d_dbg_span.get(), h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    long long t0 = 0;
    // (the one-launch step: provider + one kernel per step, four launches; rows 4 and 5 stay zero)
    const int nlaunch = p->fused_launches > fused_before ? 4 : 6;
    for (int l = 0; l < 36; l++) out[l] = 0;
    for (int l = 0; l < nlaunch; l++) {
        std::vector<long long> in, ex;
        for (size_t r = 0; r < (size_t) 4096 * 8; r++) {
            const long long a0 = h[((size_t) l * 4096 * 8 + r) * 2], a1 = h[((size_t) l * 4096 * 8 + r) * 2 + 1];
            if (a0 && a1) { in.push_back(a0); ex.push_back(a1); }
        }
        if (in.empty()) return fail(p, VVHIP_ERR_INVALID, "no stamps recorded for one of the launches");
        std::sort(in.begin(), in.end()); std::sort(ex.begin(), ex.end());
        if (l == 0) t0 = in.front();
        const long long v[6] = {in.front(), in[in.size() / 2], in.back(), ex.front(), ex[ex.size() / 2], ex.back()};
        for (int k = 0; k < 6; k++) out[l * 6 + k] = (double) (v[k] - t0) * 10.0;
    }
    return VVHIP_OK;
#endif
}

int vvhip_comm_unique_id(void* id128) {
    if (!id128) return VVHIP_ERR_INVALID;
    RcclApi& r = rccl_api();
    if (!r.ok) return VVHIP_ERR_UNSUPPORTED;
    ncclUniqueId id;
    if (r.getUniqueId(&id) != ncclSuccess) return VVHIP_ERR_HIP;
    std::memcpy(id128, &id, sizeof(id));
    return VVHIP_OK;
}
int vvhip_comm_init(vvhip_plan* p, const void* id128, int nranks, int rank) {
    NEED_BOUND(p);
    if (!id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(p, VVHIP_ERR_INVALID, "bad communicator arguments");
    RcclApi& r = rccl_api();
    if (!r.ok) return fail(p, VVHIP_ERR_UNSUPPORTED, "librccl.so.1 could not be loaded");
    if (p->comm) { (void) r.commDestroy(p->comm); p->comm = nullptr; }
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    ncclResult_t e = r.commInitRank(&p->comm, nranks, id, rank);
    if (e != ncclSuccess) { p->comm = nullptr; return fail(p, VVHIP_ERR_HIP, std::string("ncclCommInitRank: ") + (r.getErrorString ? r.getErrorString(e) : "error")); }
    p->comm_ranks = nranks;
    drop_graphs(p);
    return VVHIP_OK;
}
int vvhip_comm_count(vvhip_plan* p, int32_t* ranks) {
    if (!p || !ranks) return VVHIP_ERR_INVALID;
    *ranks = 0;
    if (!p->comm) return VVHIP_OK;                   // no communicator: 0
    RcclApi& r = rccl_api();
    int n = p->comm_ranks;
    if (r.commCount && r.commCount(p->comm, &n) != ncclSuccess) return fail(p, VVHIP_ERR_HIP, "ncclCommCount failed");
    *ranks = n;
    return VVHIP_OK;
}
int vvhip_peer_access(int device, int peer_device, int32_t* can_access) {
    if (!can_access) return VVHIP_ERR_INVALID;
    int can = 0;
    if (device == peer_device) { *can_access = 1; return VVHIP_OK; }
    if (hipDeviceCanAccessPeer(&can, device, peer_device) != hipSuccess) return VVHIP_ERR_HIP;
    *can_access = can;
    return VVHIP_OK;
}
// ---- xGMI mailbox (include/vvhip.h): create -> exchange the 64-byte handles by any means -> connect
// back to "created, not connected": the peers' mappings and the table of them go
static void mailbox_disconnect(vvhip_plan* p) {
    p->mb_on = false;
    p->mb_shared_device = false;       // (a second connect must not count the first one's ranks again)
    p->mb_device_ranks = 1;
    p->mb_opened.clear();
    p->d_mb_peers.reset();
}
static void mailbox_release(vvhip_plan* p) {
    mailbox_disconnect(p);
    p->d_mb_ctl.reset();
    p->mb_local.reset();
    p->mb_ranks = 0;
}
int vvhip_mailbox_create(vvhip_plan* p, int nranks, int rank, void* handle64) {
    NEED_BOUND(p);
    if (!handle64 || nranks < 1 || nranks > vv::MB_MAX_RANKS || rank < 0 || rank >= nranks)
        return fail(p, VVHIP_ERR_INVALID, "mailbox: 1 <= ranks <= 16, 0 <= rank < ranks");
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "the C ABI hands the IPC handle over as 64 bytes");
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    mailbox_release(p);
    drop_graphs(p);
    const size_t bytes = (size_t) 2 * nranks * vv::MB_WORDS * sizeof(unsigned long long);
    // uncached: peers' stores land in this GPU's memory over xGMI and must be seen by loads that would otherwise hit in L2
    HIP_TRY(p, vv::zeros(p->mb_local, std::max(bytes, (size_t) 4096), p->stream, true));
    HIP_TRY(p, vv::zeros(p->d_mb_ctl, 4 * sizeof(unsigned int), p->stream));
    HIP_TRY(p, hipDeviceSynchronize());
    hipIpcMemHandle_t h;
    HIP_TRY(p, hipIpcGetMemHandle(&h, p->mb_local.get()));
    std::memcpy(handle64, &h, 64);
    p->mb_ranks = nranks;
    p->mb_rank = rank;
    return VVHIP_OK;
}
int vvhip_mailbox_connect(vvhip_plan* p, const void* handles) {
    NEED_BOUND(p);
    if (!p->mb_local || !handles) return fail(p, VVHIP_ERR_INVALID, "vvhip_mailbox_create has not been called");
    std::vector<unsigned long long*> peers((size_t) p->mb_ranks, nullptr);
    // A second connect: what vvhip_mailbox_destroy does first -- captured step graphs carry the OLD peer table's address and the peers' box
    // addresses in their kernel arguments (a replay after the free below would read unmapped memory), launches still in flight use them too,
    // and whether the step may be one launch depends on who shares the device (re-evaluated: forget_fused_checks).
    TRY(settle_recovery(p));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    drop_graphs(p);
    forget_fused_checks(p);
    mailbox_disconnect(p);
    // (an error below leaves the mailbox as it is now: created, not connected)
    auto give_up = [p](hipError_t e, const char* what) { mailbox_disconnect(p); return hip_fail(p, e, what); };
    for (int r = 0; r < p->mb_ranks; r++) {
        if (r == p->mb_rank) { peers[r] = p->mb_local.get(); continue; }
        hipIpcMemHandle_t h;
        std::memcpy(&h, (const char*) handles + (size_t) r * 64, 64);
        vv::IpcMapping box;
        if (hipError_t e = box.open(h); e != hipSuccess) return give_up(e, "hipIpcOpenMemHandle");
        void* m = box.get();
        p->mb_opened.push_back(std::move(box));
        peers[r] = (unsigned long long*) m;
        // whose memory is it?  A box on this very device means that rank shares the GPU with this one
        hipPointerAttribute_t attr;
        int dev = -1;
        if (hipGetDevice(&dev) == hipSuccess && hipPointerGetAttributes(&attr, m) == hipSuccess && attr.device == dev) { p->mb_shared_device = true; p->mb_device_ranks++; }
        else (void) hipGetLastError();
    }
    if (hipError_t e = vv::upload(p->d_mb_peers, peers); e != hipSuccess) return give_up(e, "upload of the peer table");
    p->mb_on = true;
    return VVHIP_OK;
}
int vvhip_mailbox_status(vvhip_plan* p, int32_t* active, int32_t* timed_out) {
    NEED_BOUND(p);
    if (active) *active = use_mailbox(p) ? 1 : 0;
    if (timed_out) {
        *timed_out = 0;
        if (p->d_mb_ctl) {
            unsigned int ctl[4];
            HIP_TRY(p, hipStreamSynchronize(p->stream));
            HIP_TRY(p, hipMemcpy(ctl, p->d_mb_ctl.get(), sizeof ctl, hipMemcpyDeviceToHost));
            *timed_out = (int32_t) ctl[0];
        }
    }
    return VVHIP_OK;
}
int vvhip_mailbox_layout(vvhip_plan* p, int32_t* shared_device, int32_t* arithmetic_layout) {
    NEED_BOUND(p);
    if (shared_device) *shared_device = p->mb_shared_device ? 1 : 0;
    if (arithmetic_layout) *arithmetic_layout = (use_mailbox(p) && periodic_b(p)) ? 1 : 0;
    return VVHIP_OK;
}
int vvhip_mailbox_destroy(vvhip_plan* p) {
    NEED_BOUND(p);
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    drop_graphs(p);
    mailbox_release(p);
    return VVHIP_OK;
}

int vvhip_comm_destroy(vvhip_plan* p) {
    if (!p) return VVHIP_ERR_INVALID;
    if (p->comm) { (void) hipStreamSynchronize(p->stream); (void) rccl_api().commDestroy(p->comm); p->comm = nullptr; p->comm_ranks = 1; }
    return VVHIP_OK;
}
int vvhip_run_eager(vvhip_plan* p, int nsteps, const void* site, double k_tether, double k_drude) {
    NEED_BOUND(p);
    if (nsteps < 0) return VVHIP_ERR_INVALID;
    TRY(check_exchange_health(p));
    TRY(recovery_note_run(p, 1, nsteps, 0, site, k_tether, k_drude));
    struct InLoop { vvhip_plan* p; bool was; InLoop(vvhip_plan* q) : p(q), was(q->rec.in_loop) { p->rec.in_loop = true; } ~InLoop() { p->rec.in_loop = was; } } in_loop(p);
    if (!p->hp.params.use_middle_scheme && site && nsteps > 0) TRY(vvhip_synth_tether_force(p, site, k_tether, k_drude));   // see vvhip_run_graph
    for (int i = 0; i < nsteps; i++) TRY(plan_step(p, site, k_tether, k_drude, false));
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

}  // extern "C"
