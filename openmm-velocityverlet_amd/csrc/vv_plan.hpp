// vv_plan.hpp -- the one internal header of the C ABI (include/vvhip.h): the plan, and what more than one of its translation units calls.
// "HOST" = platforms/cuda/src/CudaVVKernels.cpp, "API" = openmmapi/src/VVIntegrator.cpp of the reference.
//
//   vv_api.cpp       life cycle (create / tune / bind / parameters / destroy), the status words and vvhip_synchronize, the caller-owned
//                    one-liners (vvhip_malloc ... vvhip_stream_*); fail, hip_fail, settle_recovery, check_exchange_health, drop_graphs
//   vv_launch.cpp    fixed-point scales, launch shape, kernel arguments, ScopedTimer + roctx, run_a / run_b / run_chain / run_ke /
//                    run_chain_and_b / run_fused and the checks in front of it, thermo_mode, the stage-bit helpers; vvhip_timing_*,
//                    vvhip_generic_launches, vvhip_set_trace, vvhip_rtc_*
//   vv_steps.cpp     the thermostat application (compose_application, run_application*), every step entry point, the split
//                    (kernel-interface) entry points, vvhip_algorithmic_bytes, vvhip_accumulators
//   vv_observe.cpp   what rides beside the step: the Drude report, start velocities, and the thirteen scheduled riders in ride order (riders) --
//                    series row, removal of the centre-of-mass motion, trajectory frame, profile / MSD / RDF / current / density-mode / contact / autocorrelation / self van Hove / distinct van Hove / spatial distribution sample, with their
//                    late words: the rings' cursors, the removals' record, the ten recorders' d_words; the recorders' one life cycle
//                    (recorder_*), step_begin / step_done, quiesce; the riders' one schedule is vv_schedule.hpp (integers only, no HIP)
//   vv_barostat.cpp  the device half of a Monte Carlo barostat attempt: vvhip_barostat_scale / _restore / _read
//   vv_run.cpp       the plan-driven loops: random slices, recovery from a missed rendezvous, plan_step, graph capture and replay,
//                    vvhip_run_graph / vvhip_run_eager(_unfused), vvhip_synth_tether_force
//   vv_checkpoint.cpp  the state as a durable blob: vvhip_state_digest, vvhip_checkpoint_size / _save / _load, over the SAME list of items as
//                    the recovery snapshot (recovery_items); the blob's format and parser are vv_ckpt_format.cpp (no HIP in it)
//   vv_exchange.cpp  between the ranks: the RCCL loader and vvhip_comm_*, the xGMI mailbox, exchange_accumulators
//   vv_debug.cpp     test hooks (vvhip_debug_* except vvhip_debug_tune), vvhip_time_kernel, the probes of the instrumented build
//
// Whatever one file alone uses is static (or in an anonymous namespace) there; what is declared here is hidden from the dynamic symbol
// table, which holds the vvhip_* functions of include/vvhip.h and nothing else of these files.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include <rccl/rccl.h>      // types and prototypes only: the library is resolved at run time (see rccl_api)

#include "vv_devmem.hpp"
#include "vv_host.hpp"
#include "vv_kernels.hpp"
#include "vv_rtc.hpp"
#include "vv_schedule.hpp"

#pragma GCC visibility push(hidden)

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
RcclApi& rccl_api();

using vv::kAvogadro;      // vv_host.hpp
using vv::kBoltz;
enum TimerClass { T_A = 0, T_B = 1, T_OTHER = 2 };
constexpr int kAccN = vv::NUM_ACC * vv::ACC_SLOTS;
// The one-launch step's rendezvous buffer (d_rv), in 8-byte words -- the one statement of its layout on the host:
//   [2 thermostat parities][kRvRoom replicas][NUM_ACC][ACC_SLOTS]   the blocks' words; vv::RV_REPLICAS of the kRvRoom copies are in use, the rest is slack
//   [2 parities][ACC_SLOTS] 4-byte words                            "this block polled twice", read by the wait's controller of the step after next
//   [kRvDeadTail] words                                             the first one = "a rendezvous of this plan has failed" (vv_device.inc: rv_dead_word)
constexpr int kRvRoom = 6;
static_assert(vv::RV_REPLICAS <= kRvRoom, "the replicas in use must fit the room of a parity");
constexpr int kRvCopy = kRvRoom * kAccN;
constexpr int kRvLateWord = 2 * kRvCopy;
constexpr int kRvDeadWord = kRvLateWord + 2 * vv::ACC_SLOTS * (int) sizeof(unsigned int) / (int) sizeof(unsigned long long);
constexpr int kRvDeadTail = 8;
constexpr int kRvWords = kRvDeadWord + kRvDeadTail;
static_assert(kRvCopy == 15360 && kRvLateWord == 30720 && kRvDeadWord == 30976 && kRvWords == 30984, "the addresses the compiled kernels see");
inline unsigned long long* rv_words(unsigned long long* rv, int parity) { return rv + parity * kRvCopy; }
inline unsigned int* rv_late_row(unsigned long long* rv, int parity) { return (unsigned int*) (rv + kRvLateWord) + vv::ACC_SLOTS * parity; }
inline unsigned long long* rv_dead_tail(unsigned long long* rv) { return rv + kRvDeadWord; }
constexpr int kGuardByte = 0xA5;    // fills the guard item behind a ring's last item (Ring)
static_assert(vv::ACF_VELOCITY_PARTICLES == VVHIP_ACF_VELOCITY_PARTICLES && vv::ACF_VELOCITY_MOLECULES == VVHIP_ACF_VELOCITY_MOLECULES && vv::ACF_ORIENTATION == VVHIP_ACF_ORIENTATION, "vv_args.hpp states the ABI's three modes");
static_assert(SCHEDULE_LINEAR == VVHIP_FRAMES_LINEAR && SCHEDULE_LOG10 == VVHIP_FRAMES_LOG10, "vv_schedule.hpp states the ABI's two kinds");
// The step's scheduled riders (riders()) in ride order, each with its late words, what a recovery puts back with the step counter:
//   0 series row (the ring's cursor)   1 removal of the centre-of-mass motion, in front of its step (the schedule's record)
//   2 trajectory frame (the ring's cursor)   3 profile sample   4 MSD sample   5 RDF sample   6 current sample   7 density-mode sample   8 contact sample   9 autocorrelation sample   10 self van Hove sample   11 distinct van Hove sample   12 spatial distribution sample (3 .. 12: all of d_words)
constexpr int kRiders = 13;

// How a thermostat application (sums in kernel A -> exchange between the ranks -> chain -> scaling in kernel B) runs for the plan as it
// stands; thermo_mode is the one place that derives it.
// COS_MOMENTS = the cos perturbation in two launches instead of three: kernel A accumulates the group sums as moments of the biased
// velocities next to the bias moment itself, kernel B's inline chain finishes the algebra (vv_args.hpp: the moment bits).  Not with
// molecules larger than a wave or the stand-alone chain launch (long chains, very large systems), which keep the bias -> KE -> scale
// sequence of COS_THREE_LAUNCH (API:252-259).
enum class ThermoMode { NO_NH, PLAIN, COS_MOMENTS, COS_THREE_LAUNCH };

// The synthetic force provider of the plan-driven loops (vvhip_run_*: tether sites and the two spring constants; site = null: the host's forces)
struct ForceProvider { const void* site; double kt, kd; };
// What a captured graph depends on besides the thermostat parity of its slot
struct GraphKey {
    int steps = 0;
    ForceProvider fp{};
    std::vector<int> due[kRiders];         // per rider the steps of the graph it rides on (Rider::window; empty while it is off)
    bool operator==(const GraphKey& o) const {
        return steps == o.steps && fp.site == o.fp.site && fp.kt == o.fp.kt && fp.kd == o.fp.kd && std::equal(due, due + kRiders, o.due);
    }
};

// What the series' rows and the recorder's frames both are: `capacity` items of item_bytes on the device with a guard item behind the last
// (kGuardByte: vvhip_debug_*_guard) and a two-word cursor {items counted (past capacity too), items dropped} that the append kernels advance.
// fetch, copy_out and guard_intact read what the device has written: the stream has drained.
struct Ring {
    size_t item_bytes = 0; int capacity = 0;
    vv::DevBuf<unsigned char> d_items;
    vv::DevBuf<unsigned long long> d_cursor;
    struct Count { long long stored, counted, dropped; };
    // zeroed items, guard and cursor, enqueued on `s`; a failed allocation leaves `*failed` = the bytes it asked for
    hipError_t alloc(size_t item_bytes_, int capacity_, hipStream_t s, size_t* failed) {
        hipError_t e = vv::zeros(d_items, *failed = ((size_t) capacity_ + 1) * item_bytes_, s);
        if (e == hipSuccess) e = hipMemsetAsync(d_items.get() + (size_t) capacity_ * item_bytes_, kGuardByte, item_bytes_, s);
        if (e == hipSuccess) e = vv::zeros(d_cursor, *failed = 2 * sizeof(unsigned long long), s);
        if (e == hipSuccess) { item_bytes = item_bytes_; capacity = capacity_; }
        return e;
    }
    hipError_t fetch(Count* c) const {
        unsigned long long cur[2] = {0, 0};
        const hipError_t e = hipMemcpy(cur, d_cursor.get(), sizeof(cur), hipMemcpyDeviceToHost);
        *c = {(long long) (cur[0] < (unsigned long long) capacity ? cur[0] : capacity), (long long) cur[0], (long long) cur[1]};
        return e;
    }
    hipError_t copy_out(void* out, long long n) const { return n > 0 ? hipMemcpy(out, d_items.get(), (size_t) n * item_bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    hipError_t guard_intact(int32_t* intact) const {
        std::vector<unsigned char> g(item_bytes);
        const hipError_t e = hipMemcpy(g.data(), d_items.get() + (size_t) capacity * item_bytes, item_bytes, hipMemcpyDeviceToHost);
        *intact = std::all_of(g.begin(), g.end(), [](unsigned char c) { return c == kGuardByte; });
        return e;
    }
    hipError_t reset_cursor(hipStream_t s) {      // complete on return
        const hipError_t e = hipMemsetAsync(d_cursor.get(), 0, 2 * sizeof(unsigned long long), s);
        return e == hipSuccess ? hipStreamSynchronize(s) : e;
    }
};

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
    int profile_grid_cap = 256;    // most blocks of a profile sample's accumulating kernel, besides grid_cap_a: every block flushes a table of its own (test hook "profile_grid_cap"; TUNING_LOG.md)
    int msd_block_threads = 0;     // threads per block of an MSD sample's accumulating kernel, 0: by the number of units (msd_enqueue; test hook "msd_block_threads")
    int msd_wave_reduce = 1;       // an MSD sample's waves whose units share a group add their four sums once (test hook "msd_wave_reduce": 0 = every lane adds; same bits)
    int current_two_level = 0;     // a current sample's reduce stores per-block slabs that the correlate kernel sums, instead of agent-scope adds (test hook "current_two_level", read at the start; same bits; TUNING_LOG.md)
    int current_block_threads = 0; // threads per block of a current sample's reduce, 0: by the number of particles (current_enqueue; test hook "current_block_threads"; same bits)
    int modes_sites_per_thread = 0; // sites a thread of a density-mode sample's mode kernel keeps in registers: 1, 2, 4, 8; 0: by the number of work items (vvhip_modes_start; test hook "modes_sites_per_thread", read at the start; same bits)
    int modes_k_tile = 0;          // modes per work item of that kernel, 1 .. 1024; 0: by the number of work items (test hook "modes_k_tile", read at the start; same bits)
    int modes_block_threads = 0;   // threads per block of that kernel, 0: 256 (test hook "modes_block_threads", read at the start; same bits)
    int rdf_hist_copies = 1;       // private histograms per block of an RDF sample's pair kernel: 1, or 4 = one per wave where they fit the LDS budget (test hook "rdf_hist_copies"; same bits; TUNING_LOG.md)
    int contacts_rows_per_tile = 128;   // rows a block of a contact sample's mask kernel stages in LDS: a multiple of 64 up to 1024 (test hook "contacts_rows_per_tile", read at the start; same bits; TUNING_LOG.md)
    int contacts_words_per_item = 4;    // column words per work item of that kernel, one per wave and trip: 1 .. 64 (test hook "contacts_words_per_item", read at the start; same bits)
    int contacts_skip_zero = 1;         // the correlate kernel loads neither the sample's nor the surviving words behind a zero origin word (test hook "contacts_skip_zero"; same bits)
    int acf_block_threads = 0;          // threads per block of an autocorrelation sample's accumulating kernel, 0: by the number of units (acf_enqueue; test hook "acf_block_threads")
    int acf_wave_reduce = 1;            // an autocorrelation sample's waves whose units share a group add their sums once (test hook "acf_wave_reduce": 0 = every lane adds; same bits)
    int vanhove_block_threads = 0;      // threads per block of a self van Hove sample's accumulating kernel, 0: by the number of units (vanhove_enqueue; test hook "vanhove_block_threads")
    int vanhove_lds = 1;                // that kernel counts a slot in a block-private LDS histogram and flushes the non-zero bins (test hook "vanhove_lds": 0 = every increment is a global add; same bits)
    int vanhove_wave_reduce = 1;        // its waves whose units share a group add their six head words once (test hook "vanhove_wave_reduce": 0 = every lane adds; same bits)
    int acf_slots_in_flight = 4;        // ring slots whose loads that kernel issues before it uses the first, 1 .. 8 (test hook "acf_slots_in_flight"; same bits; TUNING_LOG.md)
    int vhd_hist_copies = 1;       // private histograms per block of a distinct van Hove sample's pair kernel: 1, or 4 = one per wave where they fit (test hook "vhd_hist_copies"; same bits)
    int vhd_items_target = 4096;   // its work list aims at about this many items before it gives one more than 64 j-sites (test hook "vhd_items_target"; read at the start)
    int vhd_lds = 1;               // that kernel counts into a block-private LDS histogram (test hook "vhd_lds": 0 = every pair is a global add; same bits)
    int sdf_items_target = 4096;   // a spatial distribution sample's work list aims at about this many blocks before it gives a block more than 64 j-sites (test hook "sdf_items_target"; read at the start)
    int rdf_items_target = 4096;   // the pair kernel's work list aims at about this many blocks before it gives a block more than 64 j-sites (test hook "rdf_items_target")
    int split_chain_waves = 44000;  // systems with at least this many waves (~2.6 M particles) run the chain as its own launch.  Round 4, with two blocks of seven tile
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
        // all thirteen riders -- series row, removal of the centre-of-mass motion, trajectory frame, profile, MSD, RDF, current, density-mode, contact, autocorrelation, self van Hove, distinct van Hove and spatial distribution sample.  A
        // recovery puts it back together with their late words: the two rings' cursors, the removals' record, the ten recorders' d_words
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
    // d_rv = the rendezvous buffer, uncached (its layout: kRvWords above); fused_checks = the pairs of stage sets / launch
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
        // the saved copies (vv_run.cpp: recovery_items pairs each with the live array it belongs to)
        vv::DevBuf<void> posq, corr, velm, force, fextra, random, nh, epoch;
        Cursor cur;                               // the host's cursor at the snapshot
        struct Run { int kind, nsteps, spg; ForceProvider fp; };
        std::vector<Run> runs;
        long long recoveries = 0;
        vv::DevBuf<void> late[kRiders];           // per rider its Rider::late words (its schedule, the step counter, is in `cur`) ...
        bool saved[kRiders] = {};                 // ... where the snapshot took them
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
        GraphKey key;
        uint32_t random_end = 0;               // prepareRandomNumbers cursor after the graph's last step
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
        Schedule when;                            // (linear)
        int mask = 0;
        long long k0 = 0;                         // row 0 is step when.interval * k0
        Ring ring;                                // of vvhip_series_row
        vv::DevBuf<long long> d_scratch;          // the report's scratch for the rows (as d_rep), zero between rows
    } series;
    // Trajectory frames (vvhip_frames_*; vv_dev_frames.inc), scheduled by cur.step_count.  `described`: the layout below is that of the last
    // description that passed vvhip_frames_start's argument checks (kept for an unbound plan too: vvhip_frames_info answers from it);
    // `on`: the recorder runs and the device buffers exist
    struct Frames {
        bool on = false, described = false, has_subset = false;
        Schedule when;
        int capacity = 0, mask = 0;               // (the capacity as described: the ring has it once the recorder runs)
        int num_particles = 0, component_bytes = 0, plane_stride = 0;
        long long frame_bytes = 0, off_positions = -1, off_velocities = -1;
        long long start_step = 0;                 // the step count at the start
        long long origin = 0;                     // frame j belongs to the j-th due step after this one (start_step, or the last frame counted before a reset)
        std::vector<int32_t> particles;           // with a subset: the global indices this plan records (subset within the shard), ascending
        Ring ring;                                // of frame_bytes each
        vv::DevBuf<int32_t> d_subset;             // [num_particles] shard-relative indices (with a subset)
    } frames;
    // What the ten accumulating recorders below share, and the shape vv_observe.cpp's recorder_* skeleton works on.  `described`: `lay` is
    // the layout of the last description that passed the recorder's *_start checks (kept for an unbound plan too: *_info answers from it);
    // `on`: the recorder runs and the device buffers exist.  Each recorder adds
    //   lay, dev               its vvhip_*_layout; its device tables besides d_words (`dev = {}` drops them all)
    //   kHead, table_offset()  the count words in front of d_words; where the table starts in it, in words
    //   bytes()                of d_words
    //   alloc(s, &asked)       d_words, zeroed on stream s, and dev from the host tables; a request that fails leaves its bytes in `asked`
    //   reset(s)               what *_read's reset enqueues
    // Stated once below them: Units, the unit tables and all of the above for the three recorders of per-unit vectors (msd, acf, vanhove); Slotted,
    // "no slot holds a sample" and the reset for the three whose ring slots carry a word of their own (current, modes, contacts).  Rdf, Vhd, Sdf and
    // Contacts keep their own index / mol / stride(): a shared base would cost more lines than the four it saves.  The host tables come
    // from vv_observe.cpp's "shared pieces of a start".
    struct Recorder {
        bool on = false, described = false;
        Schedule when;                            // (linear)
        vv::DevBuf<long long> d_words;            // counts, then what the recorder accumulates -- ALL of it the rider's late words
        // one table as the host built it, of 16 bytes at the least
        template <class T, class U>
        static hipError_t put(vv::DevBuf<T>& buf, const std::vector<U>& v, size_t* asked, size_t floor = 16) {
            *asked = std::max(floor, v.size() * sizeof(U));
            return vv::upload(buf, v, floor);
        }
    };
    // A recorder D whose ring slots have a word each that is -1 while the slot holds no sample: D::slots() = {first word, words} of them in
    // d_words, D::front_words() what lies in front of the ring.  alloc() ends with empty_slots(); a reset zeroes the front and empties the
    // slots, so the ring may keep its bits.  (No slots -- density modes without lags --: nothing is enqueued for them.)
    template <class D>
    struct Slotted : Recorder {
        hipError_t empty_slots(hipStream_t s) {
            const std::pair<size_t, size_t> w = static_cast<const D*>(this)->slots();
            return w.second == 0 ? hipSuccess : hipMemsetAsync(d_words.get() + w.first, 0xFF, w.second * sizeof(long long), s);
        }
        hipError_t reset(hipStream_t s) {
            const hipError_t e = hipMemsetAsync(d_words.get(), 0, static_cast<const D*>(this)->front_words() * sizeof(long long), s);
            return e == hipSuccess ? empty_slots(s) : e;
        }
    };
    // Profiles (vvhip_profile_*; vv_dev_profile.inc), scheduled by cur.step_count
    struct Profile : Recorder {
        bool grouped = false;
        vvhip_profile_layout lay{};
        std::vector<int32_t> index;               // shard-relative indices of the recorded particles, ascending; empty: every particle of the shard
        std::vector<unsigned char> group;         // [num_particles] their groups (grouped)
        std::vector<double> mass;                 // [num_particles] their masses
        struct Dev { vv::DevBuf<int32_t> index; vv::DevBuf<unsigned char> group; vv::DevBuf<double> mass; } dev;
        static constexpr int kHead = vv::PROFILE_HEAD;      // d_words: [kHead + lay.words] counts, then the table
        size_t table_offset() const { return kHead; }
        size_t bytes() const { return (size_t) (kHead + lay.words) * sizeof(long long); }
        hipError_t alloc(hipStream_t s, size_t* asked) {
            hipError_t e = vv::zeros(d_words, *asked = bytes(), s);
            if (e == hipSuccess) e = put(dev.mass, mass, asked);
            if (e == hipSuccess && !index.empty()) e = put(dev.index, index, asked);
            if (e == hipSuccess && grouped) e = put(dev.group, group, asked);
            return e;
        }
        hipError_t reset(hipStream_t s) { return hipMemsetAsync(d_words.get(), 0, bytes(), s); }
    } profile;
    // A recorder of one vector per unit, of layout L with Head count words: mean-squared displacements (vvhip_msd_*; vv_dev_msd.inc) and
    // autocorrelations (vvhip_acf_*; vv_dev_acf.inc), scheduled by cur.step_count.  The unit tables are built from the plan's molecules
    // when the recorder starts (vv_observe.cpp: plan_units, fill_units): units ordered by group, then by particle / molecule / pair index
    template <class L, int Head>
    struct Units : Recorder {
        bool grouped = false, molecules = false;  // molecules: the start's mode is the recorder's molecule mode (first, weight, total exist)
        L lay{};
        std::vector<int32_t> index;               // particles: shard-relative index per unit, empty: unit u is particle u; molecules: the member lists, each ascending; orientation: head, tail per unit
        std::vector<int32_t> first;               // molecules: [num_units + 1] offsets into index / weight
        std::vector<double> weight, total;        // molecules: the members' masses; [num_units] their sums M in the members' order
        std::vector<unsigned char> group;         // [num_units] (grouped)
        struct Dev { vv::DevBuf<int32_t> index, first; vv::DevBuf<double> weight, total; vv::DevBuf<unsigned char> group; } dev;
        static constexpr int kHead = Head;                  // d_words: [kHead + lay.words] counts, floor and table, then the ring of origins
        size_t table_offset() const { return kHead; }
        int32_t stride() const { return (lay.num_units + 15) / 16 * 16; }
        size_t bytes() const { return (size_t) (kHead + lay.words) * sizeof(long long) + (size_t) lay.ring_bytes; }
        hipError_t alloc(hipStream_t s, size_t* asked) {
            hipError_t e = vv::zeros(d_words, *asked = bytes(), s);
            if (e == hipSuccess && !index.empty()) e = put(dev.index, index, asked);
            if (molecules) {
                if (e == hipSuccess) e = put(dev.first, first, asked);
                if (e == hipSuccess) e = put(dev.weight, weight, asked);
                if (e == hipSuccess) e = put(dev.total, total, asked);
            }
            if (e == hipSuccess && grouped) e = put(dev.group, group, asked);
            return e;
        }
        // (counts, floor and table; with the ordinal back at 0 no slot of the ring is live, so the ring may keep its bits)
        hipError_t reset(hipStream_t s) { return hipMemsetAsync(d_words.get(), 0, (size_t) (kHead + lay.words) * sizeof(long long), s); }
    };
    using Msd = Units<vvhip_msd_layout, vv::MSD_HEAD>;
    using Acf = Units<vvhip_acf_layout, vv::ACF_HEAD>;
    Msd msd;
    // Radial distribution functions (vvhip_rdf_*; vv_dev_rdf.inc), scheduled by cur.step_count.  The site list (ordered by group, inside a
    // group ascending by particle), the sites' molecules and the pair kernel's work items are built when the recorder starts
    struct Rdf : Recorder {
        vvhip_rdf_layout lay{};
        std::vector<int32_t> index, mol;          // [sites] particle and molecule of every site (mol: with the exclusion on)
        std::vector<vv::RdfItem> items;
        int max_jsites = 64;                      // no item has more j-sites
        struct Dev {
            vv::DevBuf<int32_t> index, mol;
            vv::DevBuf<vv::RdfItem> items;
            vv::DevBuf<double> scratch;           // [3][stride()] rewritten by every sample, not saved
        } dev;
        static constexpr int kHead = vv::RDF_HEAD;          // d_words: [kHead + lay.words] counts, then the table
        size_t table_offset() const { return kHead; }
        int32_t stride() const { return ((int32_t) index.size() + 15) / 16 * 16; }
        size_t bytes() const { return (size_t) (kHead + lay.words) * sizeof(long long); }
        hipError_t alloc(hipStream_t s, size_t* asked) {
            hipError_t e = vv::zeros(d_words, *asked = bytes(), s);
            if (e == hipSuccess) e = vv::zeros(dev.scratch, *asked = std::max<size_t>(16, (size_t) lay.scratch_bytes), s);
            if (e == hipSuccess) e = put(dev.index, index, asked);
            if (e == hipSuccess && lay.exclude_same_molecule) e = put(dev.mol, mol, asked);
            if (e == hipSuccess) e = put(dev.items, items, asked, 32);
            return e;
        }
        hipError_t reset(hipStream_t s) { return hipMemsetAsync(d_words.get(), 0, bytes(), s); }
    } rdf;
    // Collective current correlations (vvhip_current_*; vv_dev_current.inc), scheduled by cur.step_count.  The compact list of the recorded
    // particles, ordered by group, then by index, is built when the recorder starts
    struct Current : Slotted<Current> {
        bool two_level = false;                   // vvhip_plan::current_two_level as the start found it
        vvhip_current_layout lay{};
        std::vector<int32_t> index;               // [num_particles] the recorded particles
        std::vector<double> weight;               // beside index
        std::vector<unsigned char> group;         // beside index
        struct Dev {
            vv::DevBuf<int32_t> index;
            vv::DevBuf<double> weight;
            vv::DevBuf<unsigned char> group;
            vv::DevBuf<long long> slabs;          // two-level form only: the reduce blocks' slabs, rewritten by every sample, not saved
        } dev;
        static constexpr int kHead = vv::CUR_HEAD;          // d_words: head, sums, table, ring, the slots' words
        size_t table_offset() const { return kHead + sums_words(); }
        size_t slab_words() const { return ((size_t) (lay.num_particles + 63) / 64 + 1) * (sums_words() + 1); }
        size_t sums_words() const { return (size_t) lay.num_groups * 6; }
        size_t front_words() const { return (size_t) kHead + sums_words() + (size_t) lay.words; }      // what a reset zeroes
        size_t bytes() const { return front_words() * sizeof(long long) + (size_t) lay.ring_bytes; }
        std::pair<size_t, size_t> slots() const { return {bytes() / sizeof(long long) - lay.num_origins, (size_t) lay.num_origins}; }      // the allocation's last words
        hipError_t alloc(hipStream_t s, size_t* asked) {
            hipError_t e = vv::zeros(d_words, *asked = bytes(), s);
            if (e == hipSuccess) e = put(dev.index, index, asked);
            if (e == hipSuccess) e = put(dev.weight, weight, asked);
            if (e == hipSuccess) e = put(dev.group, group, asked);
            if (e == hipSuccess && two_level) e = vv::zeros(dev.slabs, *asked = slab_words() * sizeof(long long), s);
            return e == hipSuccess ? empty_slots(s) : e;
        }
    } current;
    // Density modes for the structure factors (vvhip_modes_*; vv_dev_modes.inc), scheduled by cur.step_count.  The compact list of the
    // recorded sites (ordered by group, then by index), the modes and the mode kernel's work items are built when the recorder starts;
    // lay holds the shape the items were built for (sites_per_thread, k_tile, block_threads)
    struct Modes : Slotted<Modes> {
        vvhip_modes_layout lay{};
        std::vector<int32_t> index;               // [num_particles] the recorded sites
        std::vector<double> weight;               // beside index
        std::vector<int32_t> modes;               // [num_modes][3]
        std::vector<vv::ModesItem> items;
        struct Dev {
            vv::DevBuf<int32_t> index, modes;
            vv::DevBuf<double> weight;
            vv::DevBuf<vv::ModesItem> items;
            vv::DevBuf<unsigned int> turns;       // [3][stride()] rewritten by every sample, not saved
        } dev;
        static constexpr int kHead = vv::MODES_HEAD;        // d_words: head, sums, table, ring, the slots' words
        size_t table_offset() const { return kHead + sums_words(); }
        int32_t stride() const { return (lay.num_particles + 15) / 16 * 16; }
        size_t sums_words() const { return (size_t) lay.num_groups * (size_t) lay.num_modes * 2; }
        size_t front_words() const { return (size_t) kHead + sums_words() + (size_t) lay.words; }      // what a reset zeroes
        size_t bytes() const { return front_words() * sizeof(long long) + (size_t) lay.ring_bytes; }
        std::pair<size_t, size_t> slots() const { return {bytes() / sizeof(long long) - lay.num_origins, (size_t) lay.num_origins}; }      // the allocation's last words
        hipError_t alloc(hipStream_t s, size_t* asked) {
            hipError_t e = vv::zeros(d_words, *asked = bytes(), s);
            if (e == hipSuccess) e = vv::zeros(dev.turns, *asked = std::max<size_t>(16, (size_t) lay.scratch_bytes), s);
            if (e == hipSuccess) e = put(dev.index, index, asked);
            if (e == hipSuccess) e = put(dev.weight, weight, asked);
            if (e == hipSuccess) e = put(dev.modes, modes, asked);
            if (e == hipSuccess) e = put(dev.items, items, asked, 32);
            return e == hipSuccess ? empty_slots(s) : e;
        }
    } modes;
    // Contact lifetime correlations (vvhip_contacts_*; vv_dev_contacts.inc), scheduled by cur.step_count.  The site list (ordered by group,
    // inside a group ascending by particle), the sites' molecules and the two kernels' work items are built when the recorder starts;
    // lay holds the shape the mask items were built for (rows_per_tile, words_per_item)
    struct Contacts : Slotted<Contacts> {
        vvhip_contacts_layout lay{};
        vv::ContactsLayout geo{};                 // where every word lies (vv_layout.h)
        int32_t first[vv::CONTACTS_MAX_GROUPS + 1] = {0};      // where a group's sites start in the list
        std::vector<int32_t> index, mol;          // [sites] particle and molecule of every site (mol: with the exclusion on)
        std::vector<vv::ContactsMaskItem> mask_items;
        std::vector<vv::ContactsCorrItem> corr_items;
        struct Dev {
            vv::DevBuf<int32_t> index, mol;
            vv::DevBuf<vv::ContactsMaskItem> mask_items;
            vv::DevBuf<vv::ContactsCorrItem> corr_items;
            vv::DevBuf<double> scratch;           // [3][stride()] rewritten by every sample, not saved
            vv::DevBuf<unsigned long long> mask;  // [sample_words] likewise
        } dev;
        static constexpr int kHead = vv::CONTACTS_HEAD;     // d_words: head, table, ord, the ring of origins, the ring of surviving contacts
        size_t table_offset() const { return kHead; }
        int32_t stride() const { return ((int32_t) index.size() + 15) / 16 * 16; }
        size_t front_words() const { return (size_t) kHead + (size_t) lay.words; }      // what a reset zeroes
        size_t bytes() const { return (size_t) geo.words_bytes; }
        std::pair<size_t, size_t> slots() const { return {front_words(), (size_t) geo.ord_words}; }      // the ord words, right behind the front
        hipError_t alloc(hipStream_t s, size_t* asked) {
            hipError_t e = vv::zeros(d_words, *asked = bytes(), s);
            if (e == hipSuccess) e = vv::zeros(dev.scratch, *asked = std::max<size_t>(16, 3 * (size_t) stride() * sizeof(double)), s);
            if (e == hipSuccess) e = vv::zeros(dev.mask, *asked = std::max<size_t>(16, (size_t) geo.sample_words * sizeof(long long)), s);
            if (e == hipSuccess) e = put(dev.index, index, asked);
            if (e == hipSuccess && lay.exclude_same_molecule) e = put(dev.mol, mol, asked);
            if (e == hipSuccess) e = put(dev.mask_items, mask_items, asked, 32);
            if (e == hipSuccess) e = put(dev.corr_items, corr_items, asked, 32);
            return e == hipSuccess ? empty_slots(s) : e;
        }
    } contacts;
    Acf acf;                                      // (Units, beside the MSD recorder above)
    // The self van Hove function (vvhip_vanhove_*; vv_dev_vanhove.inc): the MSD recorder's units, ring and life cycle, and the squared bin
    // edges as one more device table
    struct VanHove : Units<vvhip_vanhove_layout, vv::VANHOVE_HEAD> {
        std::vector<double> e2;                   // [num_bins + 1] edges[k] * edges[k]
        vv::DevBuf<double> d_e2;
        hipError_t alloc(hipStream_t s, size_t* asked) {
            const hipError_t e = Units::alloc(s, asked);
            return e == hipSuccess ? put(d_e2, e2, asked) : e;
        }
    } vanhove;
    // The distinct van Hove function (vvhip_vanhove_distinct_*; vv_dev_vanhove_distinct.inc): the RDF recorder's sites and work items, and
    // behind the table, in the same allocation, the ring of num_origins + 1 plane sets and the spare set (all of it the rider's late words)
    struct Vhd : Recorder {
        vvhip_vanhove_distinct_layout lay{};
        std::vector<int32_t> index, mol;          // [sites] particle and molecule of every site (mol: with the exclusion on)
        std::vector<vv::RdfItem> items;           // (same != 0: every j-site of the group, the pair of a site with itself is masked)
        int max_jsites = 64;                      // no item has more j-sites
        struct Dev {
            vv::DevBuf<int32_t> index, mol;
            vv::DevBuf<vv::RdfItem> items;
        } dev;
        static constexpr int kHead = vv::VHD_HEAD;          // d_words: [kHead + lay.words] counts, floor and table, then the planes
        size_t table_offset() const { return kHead; }
        int32_t stride() const { return ((int32_t) index.size() + 15) / 16 * 16; }
        size_t bytes() const { return (size_t) (kHead + lay.words) * sizeof(long long) + (size_t) lay.ring_bytes; }
        hipError_t alloc(hipStream_t s, size_t* asked) {
            hipError_t e = vv::zeros(d_words, *asked = bytes(), s);
            if (e == hipSuccess) e = put(dev.index, index, asked);
            if (e == hipSuccess && lay.exclude_same_molecule) e = put(dev.mol, mol, asked);
            if (e == hipSuccess) e = put(dev.items, items, asked, 32);
            return e;
        }
        // (counts, floor and table; with the ordinal back at 0 no slot of the ring is live, so the ring may keep its bits)
        hipError_t reset(hipStream_t s) { return hipMemsetAsync(d_words.get(), 0, (size_t) (kHead + lay.words) * sizeof(long long), s); }
    } vhd;
    // Spatial distribution functions (vvhip_sdf_*; vv_dev_sdf.inc): the RDF recorder's sites and work items with frames for i-sites.  The
    // frame tables (ordered by frame group, inside a group as given) are built when the recorder starts
    struct Sdf : Recorder {
        vvhip_sdf_layout lay{};
        std::vector<int32_t> index, mol;          // [sites] particle and molecule of every site (mol: with the exclusion on)
        std::vector<int32_t> frames, fmol;        // [frames][3] particles o, a, b; [frames] the frame's molecule (with the exclusion on)
        std::vector<unsigned char> fgroup;        // [frames]
        std::vector<vv::RdfItem> items;
        int max_jsites = 64;                      // no item has more j-sites
        struct Dev {
            vv::DevBuf<int32_t> index, mol, frames, fmol;
            vv::DevBuf<unsigned char> fgroup;
            vv::DevBuf<vv::RdfItem> items;
            vv::DevBuf<double> scratch;           // [3][stride()], then [13][fstride()]: rewritten by every sample, not saved
        } dev;
        static constexpr int kHead = vv::SDF_HEAD;          // d_words: [kHead + lay.words] counts, then the table
        size_t table_offset() const { return kHead; }
        int32_t stride() const { return ((int32_t) index.size() + 15) / 16 * 16; }
        int32_t fstride() const { return ((int32_t) fgroup.size() + 15) / 16 * 16; }
        size_t bytes() const { return (size_t) (kHead + lay.words) * sizeof(long long); }
        hipError_t alloc(hipStream_t s, size_t* asked) {
            hipError_t e = vv::zeros(d_words, *asked = bytes(), s);
            if (e == hipSuccess) e = vv::zeros(dev.scratch, *asked = std::max<size_t>(16, (size_t) lay.scratch_bytes), s);
            if (e == hipSuccess) e = put(dev.index, index, asked);
            if (e == hipSuccess) e = put(dev.frames, frames, asked);
            if (e == hipSuccess) e = put(dev.fgroup, fgroup, asked);
            if (e == hipSuccess && lay.exclude_same_molecule) e = put(dev.mol, mol, asked);
            if (e == hipSuccess && lay.exclude_same_molecule) e = put(dev.fmol, fmol, asked);
            if (e == hipSuccess) e = put(dev.items, items, asked, 32);
            return e;
        }
        hipError_t reset(hipStream_t s) { return hipMemsetAsync(d_words.get(), 0, bytes(), s); }
    } sdf;
    // Removal of the centre-of-mass motion (vvhip_cm_motion_*; vv_dev_cmm.inc), scheduled by step_count: scratch and records of its own,
    // allocated by the first call that needs them
    struct CmMotion {
        bool on = false;
        Schedule when;                            // (linear: every when.interval-th step, step 0 included)
        vv::DevBuf<long long> d_words;            // [CMM_WORDS] zero between removals
        vv::DevBuf<vv::CmmDevRecord> d_rec;       // [2] the schedule's record; the record of vvhip_remove_cm_motion's one-off calls
        vv::PinnedBuf<double> h_v;                // pinned: the V of a one-off call as copied back
    } cmm;
    // Monte Carlo barostat (vvhip_barostat_*; vv_barostat.cpp, vv_dev_barostat.inc): tables, scratch and the backup of the last scale, all
    // allocated by the first scale.  `pending`: the backup and box_before still describe the state in front of the last scale -- cleared by
    // vvhip_set_box, vvhip_bind and (through vvhip_set_box) vvhip_checkpoint_load; a moved step counter is seen at the restore itself
    struct Barostat {
        bool pending = false;
        long long scales = 0, restores = 0;
        long long step_at_scale = 0;
        double box_before[3] = {0, 0, 0}, box_after[3] = {0, 0, 0};
        vv::DevBuf<int32_t> d_lane_mol;
        vv::DevBuf<int2> d_laneless;
        vv::DevBuf<double> d_mol_count;
        vv::DevBuf<unsigned long long> d_words;   // [BARO_HEAD + 3 per shard-local molecule]
        vv::PinnedBuf<unsigned long long> h_bad;  // pinned: the bad word as copied back
        vv::DevBuf<void> posq, corr;              // the positions in front of the last scale
    } baro;
    // Maxwell-Boltzmann start velocities (vvhip_set_velocities_to_temperature): HostPlan::therm_laneless, uploaded by the first call
    vv::DevBuf<int32_t> d_therm_laneless;
    // State digest (vvhip_state_digest): one word per section, scratch of its own, allocated by the first call
    vv::DevBuf<unsigned long long> d_digest;
    vv::PinnedBuf<unsigned long long> h_digest;   // pinned: the words as copied back
};

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

struct ScopedTimer {
    vvhip_plan* p;
    int cls;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool on, ranged = false;
    // dispatch = true: the launcher delivers the dispatch's own begin / end timestamps into e0 / e1 (kernels A and B: vv_launch);
    // otherwise the events are recorded around the enqueued work (adds two barrier packets to the stream)
    bool dispatch;
    ScopedTimer(vvhip_plan* p_, int cls_, bool dispatch_ = false);
    ~ScopedTimer();
    ScopedTimer(const ScopedTimer&) = delete;
};

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
#define NEED_FUSABLE(p)                                                                                                   \
    do {                                                                                                                \
        if (!(p)->hp.info.constraints_fused)                                                                            \
            return fail(p, VVHIP_ERR_UNSUPPORTED, std::string("the System has constraints this backend cannot solve in-kernel") + ((p)->hp.unfused_reason.empty() ? "" : " (" + (p)->hp.unfused_reason + ")") + \
                                                  ": use the split entry points around the host's constraint solver"); \
    } while (0)

inline size_t sizeof_real(int prec) { return prec == VVHIP_DOUBLE ? 8 : 4; }
inline size_t sizeof_mixed(int prec) { return prec == VVHIP_SINGLE ? 4 : 8; }
// one-line predicates and stage bits of the plan as it stands
// distance between the two parity copies: only the rows in use (4 without the cos moments)
inline int acc_stride(const vvhip_plan* p) { return (p->hp.params.cos_acceleration != 0 ? vv::NUM_ACC : 4) * vv::ACC_SLOTS; }
inline bool periodic_b(const vvhip_plan* p) { return p->hp.per.enabled && p->periodic_kernels && p->periodic_b; }
inline bool cos_on(const vvhip_plan* p) { return p->hp.params.cos_acceleration != 0; }
// the positions' low halves as a kernel argument: mixed precision only
inline void* posq_corr(const vvhip_plan* p) { return p->hp.precision == VVHIP_MIXED ? p->buf.posq_correction : nullptr; }
// No source of extra forces in a step: its kick adds whatever forceExtra still holds (see Cursor::fextra_virtual)
inline uint32_t stale_fextra(const vvhip_plan* p) { return (p->cur.fextra_dirty || p->fextra_external) ? vv::A_FE_LOAD : 0u; }
inline bool shake_on(const vvhip_plan* p) { return !p->hp.slot_shake.empty(); }
// stage bits of the in-kernel constraints the plan holds: hydrogen-type clusters and / or rigid three-site molecules
inline uint32_t cons_a(const vvhip_plan* p) { return (p->hp.info.num_shake_clusters > 0 ? vv::A_SHAKE_V : 0u) | (p->hp.info.num_settle_clusters > 0 ? vv::A_SETTLE : 0u) | (p->hp.info.num_general_constraints > 0 ? vv::A_GCONS : 0u); }
inline uint32_t cons_b(const vvhip_plan* p) { return (p->hp.info.num_shake_clusters > 0 ? vv::B_SHAKE : 0u) | (p->hp.info.num_settle_clusters > 0 ? vv::B_SETTLE : 0u) | (p->hp.info.num_general_constraints > 0 ? vv::B_GCONS : 0u); }

// vv_api.cpp
int fail(vvhip_plan* p, int code, const std::string& msg);
int hip_fail(vvhip_plan* p, hipError_t e, const char* what);
int settle_recovery(vvhip_plan* p);
int check_exchange_health(vvhip_plan* p);
void drop_graphs(vvhip_plan* p);
// vv_launch.cpp
void fill_scales(vvhip_plan* p);
void pick_launch_shape(vvhip_plan* p);
vv::KArgs make_args(vvhip_plan* p, uint32_t flags, uint32_t random_index);
int upload_lane_const(vvhip_plan* p);
int ensure_mass_table(vvhip_plan* p);
int run_a(vvhip_plan* p, uint32_t flags, uint32_t random_index);
int run_b(vvhip_plan* p, uint32_t flags);
int run_chain(vvhip_plan* p, uint32_t flags);
int run_ke(vvhip_plan* p, uint32_t flags, uint32_t random_index);
int run_chain_and_b(vvhip_plan* p, uint32_t bflags, bool with_bias);
int run_fused(vvhip_plan* p, uint32_t aflags, uint32_t bflags, uint32_t random_index, bool* taken);
ThermoMode thermo_mode(const vvhip_plan* p);
bool use_mailbox(const vvhip_plan* p);
uint32_t chain_in_b(const vvhip_plan* p);
bool fused_shape_ok(const vvhip_plan* p);
bool fused_state_ok(const vvhip_plan* p);
bool fused_active(const vvhip_plan* p);
void forget_fused_checks(vvhip_plan* p);
uint32_t extra_flags(const vvhip_plan* p);
uint32_t after_positions(const vvhip_plan* p);
uint32_t tail_flags(const vvhip_plan* p);
// vv_steps.cpp
ThermoApp middle_application(const vvhip_plan* p);
int run_application_fused(vvhip_plan* p, const ThermoApp& t, uint32_t random_index, bool* taken);
// vv_observe.cpp
int step_begin(vvhip_plan* p);
int step_done(vvhip_plan* p);
int quiesce(vvhip_plan* p, const char* who, bool sync, bool drop);
// The positions (vvhip_barostat_scale / _restore) or the velocities (vvhip_set_velocities_to_temperature) were rewritten outside the steps:
// the origins that the recorders of that quantity stored so far are dead
enum class Rewrote { POSITIONS, VELOCITIES };
int origins_dead(vvhip_plan* p, Rewrote what);
// The box was replaced (vvhip_set_box): the origins of the recorder of pair distances across time are dead (the barostat's moves reach it through origins_dead)
int box_changed(vvhip_plan* p);
// One of the device work items that hang on the plan's step counter.  A new one is a descriptor in riders() with its enqueue function and its
// entry points: the step hooks, the graph keys (vv_run.cpp) and the recovery (recovery_items) walk the list.
struct Rider {
    bool on; Schedule when;         // scheduled, and at which steps
    bool in_front;                  // rides in front of the steps that are due (by their 0-based index) / behind them (by the count they complete)
    void* late; size_t late_bytes;  // device words that a recovery puts back WITH the step counter (null: none to save as the plan stands)
    int (*enqueue)(vvhip_plan*);
    // the steps it rides on among the `steps` steps after step counter c0, counted from c0
    std::vector<int> window(long long c0, int steps) const { return in_front ? due_in(when, c0, c0 + steps - 1, c0) : due_in(when, c0 + 1, c0 + steps, c0); }
};
using Riders = std::array<Rider, kRiders>;
Riders riders(vvhip_plan* p);
// vv_run.cpp
// The plan's physical state, stated ONCE, as {live array, its saved copy of the recovery snapshot, bytes, ...}: the six state arrays (0
// bytes: not in use), both thermostat copies, the random generator's epoch -- in this order the sections VVHIP_CKPT_POSQ ..
// VVHIP_CKPT_EPOCH of a checkpoint (vv_checkpoint.cpp) -- and behind them, for the riders `with` names (null: none), their Rider::late words
// (`late`: those go back with the step counter, after the accumulators are zeroed; a checkpoint does not carry them).  For a series and a
// frame recorder these are the cursors: the repeat writes the same rows and frames at the same places.  For a profile recorder they are the
// whole allocation, counts and table: an accumulating table is not idempotent under the repeat, so it goes back as the snapshot took it.
// For an MSD recorder likewise, the ring of origins included: the repeat needs the origins that the failed window overwrote.  For an RDF
// recorder counts and table; its gather scratch is rewritten by every sample and is not saved.  For a current recorder the whole
// allocation again: head, sums, table and the ring of origins.  For a density-mode recorder likewise.  For a contact recorder head, table,
// the slots' ordinals and both rings of bit matrices: the surviving contacts are not idempotent under the repeat either.  For an
// autocorrelation recorder the whole allocation as for the MSD: head, table and the ring of origins; for a self van Hove recorder likewise; for a distinct van Hove recorder
// counts, table, ring and spare planes; for a spatial distribution recorder counts and table, as for the RDF (up to 64 MiB).
// particle_words: 32-bit words per particle of a per-particle array (its digest's base is shard_begin x that), else 0.
struct RecItem { void* live; vv::DevBuf<void>* saved; size_t bytes; bool late; uint32_t particle_words = 0; };
std::vector<RecItem> recovery_items(vvhip_plan* p, const bool with[kRiders]);
int recover_rendezvous(vvhip_plan* p, bool on_request = false);      // on_request: the test hook vvhip_debug_recover, nothing has failed
int plan_step(vvhip_plan* p, const ForceProvider& fp, bool refill);
// vv_exchange.cpp
int exchange_accumulators(vvhip_plan* p, int phase);
void mailbox_release(vvhip_plan* p);

#pragma GCC visibility pop
