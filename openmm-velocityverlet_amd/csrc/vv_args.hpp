// vv_args.hpp -- stage bits and argument blocks of the HIP kernels (gfx950): everything the device code (vv_device.inc) and its launchers
// share.  Compiled ahead of time into libvvhip.so and, for stage sets outside the compiled list, at run time by hipRTC (vv_rtc.cpp),
// which has no host headers: nothing in here may need more than the fixed-width integer types and the HIP vector types.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>

#include <cstdint>
#endif

#include "../../include/vvhip.h"
#include "vv_layout.h"

namespace vv {

// ---- stage flags of kernel A ("produce": ends in reductions) -----------------------------------
enum : uint32_t {
    A_FE_LOAD = 1u << 0,     // start the extra force from the forceExtra array (else 0)
    A_FE_STORE = 1u << 1,    // write the extra force back to the array
    A_LD = 1u << 2,          // + Langevin drag/noise              (K/drudeLangevin.cu:2-60)
    A_EF = 1u << 3,          // + electric field force             (K/electricField.cu:2-12)
    A_COS = 1u << 4,         // + cosine acceleration force        (K/cosineAccelerate.cu:2-14)
    A_KICK_FULL = 1u << 5,   // v += dt*invM*Fe + dt/2^32*invM*F   (K/middle.cu:6-23)
    A_KICK_HALF = 1u << 6,   // v += 0.5*dt*invM*Fe + fscale*invM*F (K/velocityVerlet.cu:6-29)
    A_POSDELTA_VV = 1u << 7, // posDelta = dt*v                    (K/velocityVerlet.cu:24-26)
    A_POS1 = 1u << 8,        // posDelta = oldDelta = dt/2*v       (K/middle.cu:29-42)
    A_BIAS = 1u << 9,        // accumulate sum m*vx*2cos(kz)       (K/cosineAccelerate.cu:16-61)
    A_KE = 1u << 10,         // molecular COM + per-group sum m v^2 (K/drudeNoseHoover.cu:5-151)
    A_UNBIAS_ACC = 1u << 11, // before the KE, subtract V*cos(kz) with V taken from accumulator 3
    A_COMPART = 1u << 12,    // molecules larger than a wave: add each chunk's sum(m v), sum(m) to the molecule's accumulator
    A_CZ_STORE = 1u << 13,   // keep cos(2 pi z / Lz) of every lane for the later kernels of this step (positions do not move in between)
    A_CZ_LOAD = 1u << 14,    // ... and take it from there instead of evaluating a double-precision cosine again
    A_SHAKE_V = 1u << 16,    // velocity constraints of the hydrogen-type clusters right after the kick (OpenMM applyVelocityConstraints)
    A_SETTLE = 1u << 22,     // ... of the rigid three-site molecules (one or both bits: what the plan holds)
    A_KE_MOM = 1u << 17,     // with A_BIAS | A_KE in ONE launch: the group sums as moments Saa, Sab, Sbb of the still biased velocities
                             // (accumulators 0-2, 4-6, 7-9); kernel B combines them once V is known: 2KE = Saa - 2 V Sab + V^2 Sbb
    A_MTAB = 1u << 18,       // own mass and Drude-pair mass fraction from the static per-lane tables (slot_m, slot_f) instead of
                             // reciprocals / IEEE divisions of velm.w in every step
    A_PERIODIC = 1u << 20,   // particle index, activity and segment index of a lane from the wave index (KArgs::per), role word from the pattern wave:
                             // no slot load in front of the particle loads (vv_host.hpp: PeriodicLayout)
    A_NOSTORE = 1u << 19,    // the kicked velocities stay in registers (KE stage) and are NOT written back: kernel B repeats the kick
                             // itself (B_KICK) from velm + force -- 24 bytes of force read there instead of 32 bytes written here and
                             // 3.5 MB less dirty data behind this launch at the headline size (the kernel boundary waits for it)
    A_SHAKE_GS = 1u << 21,   // hydrogen-type clusters by Gauss-Seidel sweeps of the central lane (OpenMM's iteration; VVHIP_SHAKE_MODE=0, generic
                             // kernel only) instead of the direct solve of the cluster's velocity constraints
    A_KE_PLAIN = 1u << 15,   // sum m v^2 over every massive particle into accumulator 0 (kinetic-energy query)
    A_GCONS = 1u << 23,      // velocity constraints of general clusters (any topology inside a wave): coloured Gauss-Seidel sweeps over the wave's list
};
// ---- stage flags of kernel B ("consume": starts from the scale factors) -------------------------
enum : uint32_t {
    B_SCALE = 1u << 0,        // v = s_atom*(v-V) + s_com*V, Drude pairs split (K/drudeNoseHoover.cu:157-209)
    B_UNBIAS = 1u << 1,       // remove the periodic bias before / restore after the scaling (fused)
    B_BIAS_REMOVE = 1u << 2,  // only vx -= V cos(kz)                (K/cosineAccelerate.cu:63-73)
    B_BIAS_RESTORE = 1u << 3, // only vx += V cos(kz)                (K/cosineAccelerate.cu:76-85)
    B_DRIFT_MIDDLE = 1u << 4, // fused Pos1+Pos2+Pos3 without constraints: x += dt/2*v_old + dt/2*v_new
    B_POS2 = 1u << 5,         // posDelta += dt/2*v; oldDelta += dt/2*v (K/middle.cu:47-60)
    B_POS3 = 1u << 6,         // v += (posDelta-oldDelta)/dt; x += posDelta (K/middle.cu:66-100)
    B_VV_KICK = 1u << 7,      // half kick from the forceExtra array + posDelta = dt*v (fused classic first half)
    B_VV_POS = 1u << 8,       // x += posDelta; v = posDelta/dt        (K/velocityVerlet.cu:35-68)
    B_HARDWALL = 1u << 9,     // (K/middle.cu:106-221)
    B_IMAGE = 1u << 10,       // mirror copy to the image particle     (K/imageCharge.cu:2-28)
    B_CHAIN = 1u << 11,       // run the NH chain in the kernel head from the accumulators (else read nh->scales)
    B_CZ_LOAD = 1u << 12,     // cos(2 pi z / Lz) from the per-lane cache written by kernel A (A_CZ_STORE)
    B_SHAKE = 1u << 13,       // position constraints of the hydrogen-type clusters on the step's displacement (OpenMM applyConstraints)
    B_SETTLE = 1u << 20,      // ... of the rigid three-site molecules
    B_MAILBOX = 1u << 14,     // multi-GPU mailbox: block 0's thermostat wave stores this rank's totals into every peer, all blocks sum all ranks' totals
    B_KE_MOM = 1u << 15,      // the accumulators hold moments (A_KE_MOM): combine them with V, unbias the stored COM velocities with comw
    B_KICK = 1u << 17,        // v += dt*invM*Fe + dt/2^32*invM*F (K/middle.cu:6-23) on the freshly loaded velocities: partner of A_NOSTORE, the
                              // very expression kernel A evaluated (same operands, same order: same bits); Fe = the cos force with B_UNBIAS
    B_PERIODIC = 1u << 18,    // as A_PERIODIC
    B_MTAB = 1u << 16,        // Drude-pair mass fractions from the static per-lane table (slot_f) instead of two IEEE divisions per lane
    B_SHAKE_GS = 1u << 19,    // as A_SHAKE_GS, for the position constraints (instead of the coupled Newton iteration)
    B_GCONS = 1u << 21,       // as A_GCONS, for the position constraints
    B_VSITE = 1u << 22,       // place the plan's virtual sites after the position update (integration.computeVirtualSites(), HOST:214, 374)
};
constexpr uint32_t A_CONS = A_SHAKE_V | A_SETTLE | A_GCONS, B_CONS = B_SHAKE | B_SETTLE | B_GCONS;      // in-kernel constraints of any kind
// ---- chain kernel --------------------------------------------------------------------------------
enum : uint32_t { C_CHAIN = 1u << 0, C_BIAS = 1u << 1 };

constexpr int NUM_ACC = 10;    // fixed-point quantities: 2KE atom, 2KE com, 2KE drude, bias moment; with the cos perturbation the
                               // cross moments Sab (4-6) and the field moments Sbb (7-9) of the three groups (A_KE_MOM)
constexpr int ACC_SLOTS = 256; // each quantity is spread over 256 int64 slots (block b adds into slot b % 256):
                               // thousands of blocks adding into ONE word serialise at ~10 ns per atomic on MI355X
                               // (measured: 17 us for kernel A at 1000 blocks); integer sums stay exact and
                               // order-independent, the chain wave folds the slots.  Layout acc[quantity][slot].
constexpr int RV_REPLICAS = 4; // one-launch step: copies of the rendezvous words [NUM_ACC][ACC_SLOTS] a block publishes -- lane k + NUM_ACC r of
                               // the thermostat wave stores quantity k into copy r, ONE store instruction --, each polled by its share of the blocks
static_assert(RV_REPLICAS * NUM_ACC <= 64, "one lane of the thermostat wave per quantity and replica");

// Multi-GPU accumulator exchange without a collective launch ("mailbox", one node over xGMI).  Every rank owns an UNCACHED
// device allocation box[2 parities][ranks][MB_WORDS] of 8-byte words {sequence number : 32 | payload : 32} that all peers
// have mapped through hipIpc.  At the start of kernel B the thermostat wave of block 0 -- which has just folded the rank's
// accumulators, complete since kernel A ended -- writes the NUM_ACC int64 totals as 2*NUM_ACC words into slot [seq & 1][rank] of
// every OTHER rank's box (one 8-byte store each: payload and flag travel in the same atomic word, the LL idea of RCCL).  The
// thermostat wave of every block then polls the rank's own box until the other ranks' words carry the current sequence number
// and adds them to its own fold of the local accumulators -- integers, so all ranks continue with identical bits.  Nothing is added to kernel A, no launch is
// added to the step.  Two parities suffice: a rank can only be one exchange ahead of the slowest one (it needs everybody's
// words of exchange n to finish its kernel B of exchange n).  The sequence number lives in the double-buffered NHDevState.
constexpr int MB_WORDS = 2 * NUM_ACC;
constexpr int MB_MAX_RANKS = 16;
struct Mailbox {
    unsigned long long* local;            // this rank's box
    unsigned long long* const* peers;     // device array [ranks] of every rank's box as mapped here (own entry = local)
    unsigned int* ctl;                    // [0] set when a wait on the peers ran out
    int32_t ranks, rank;
};

// Device-resident thermostat state (reference keeps it on the host: CudaVVKernels.h:206-215)
struct NHDevState {
    vvhip_nh_state s;
    double scales[4];        // what kernel B consumes: vscale[3] and the periodic bias V
    unsigned int mb_seq;     // mailbox exchanges done so far (advanced with the state by a B_MAILBOX launch)
    unsigned int rv_seq;     // fused steps done so far: the tag of the rendezvous words (advanced with the state by a fused launch)
    unsigned int rv_delay;   // fused step: units of 256 clocks a block waits between its publish and its first poll round (self-tuning, vv_device.inc)
    unsigned int rv_calm;    // ... and fused steps since a block last needed a second round
};

// Constants of the chain (HOST:577-594 fixed at init; temperatures read live as API:728 does)
struct NHConst {
    double eta_mass[VVHIP_NUM_TG][VVHIP_MAX_CHAINS];
    double inv_eta_mass[VVHIP_NUM_TG][VVHIP_MAX_CHAINS];   // 1/eta_mass (0 where the mass is 0): the chain multiplies instead of dividing
    double nkbt[VVHIP_NUM_TG];
    double temperature[VVHIP_NUM_TG];
    double step_size;
    double inv_mass_total;
    double acc_inv_scale[NUM_ACC];
    int32_t num_chains, loops_per_step, num_tg;
    uint32_t flags;
};

// Chain constants of one temperature group as the thermostat wave of kernel B loads them (lane g reads row g with ordinary vector
// loads at its very top, next to the state).  Picking lane g's row out of the kernel-argument block instead compiles to lane-indexed
// loads from the kernarg segment issued after the fold, whose latency sat on the kernel's critical path (timeline in DESIGN.md §7).
struct ChainLaneBlock {
    double eta_mass[4], inv_eta_mass[4];
    double nkbt, kT, acc_inv_scale, active;     // active != 0: the group is thermostatted (HOST:729)
    double dt2, dt4, dt8, pad_;
};

// PeriodicLayout as the kernels take it: per quantity the value of region 0 and the INCREMENTS from region to region, so that the
// value of a wave's region is base + sum of the increments of the region starts at or below the wave -- selects between a loaded
// scalar and zero.  (Selecting among the array elements themselves makes the compiler index the argument block dynamically, which
// it can only do through scratch memory: measured, kernel A 4.2 -> 5.7 us.)
struct PeriodicArgs {
    uint32_t magic;
    int32_t wpc, apc, spc;
    int32_t wave_start[4];                                    // absolute (cell-local); unused regions: INT_MAX
    int32_t d_wave[4], d_atom_start[4], d_atom_end[4], d_seg[4], d_P[4], d_spw[4];
};
// One argument block for kernels A and B (passed by value); pointer types are erased so that the
// same struct serves the three precision modes.
struct KArgs {
    // ---- first 192 bytes: what every wave needs for its first loads and kernel A for its last (three scalar-cache lines)
    const int2* slots;
    void* velm;
    void* posq;
    void* corr;
    const long long* force;
    void* comv;                    // mixed4 [num segments]: COM velocity of each COM segment (dense index, see seg_base), written by A_KE, read by B_SCALE
    unsigned long long* acc;        // accumulators of the current parity (A adds, B consumes)
    const NHDevState* nh;           // thermostat state of the current parity
    const ChainLaneBlock* lane_const;   // [VVHIP_NUM_TG] chain constants, one row per group, in device memory (kernel B's thermostat wave)
    int32_t padded;
    int32_t nwaves;
    uint32_t flags;
    uint32_t random_index;
    PeriodicArgs per;          // arithmetic work-item layout (A_PERIODIC / B_PERIODIC; vv_host.hpp: PeriodicLayout)
    double dt;                 // step size
    double inv_dt_mixed;       // 1 / dt evaluated in the mode's `mixed` type on the host (K/middle.cu:71), widened
    double inv_dt_double;      // 1.0 / dt in double (K/velocityVerlet.cu:43)
    double max_drude, hw_scale;                    // HOST:189-190
    double acc_scale[NUM_ACC];  // fixed-point scales of the accumulated quantities (kernel A's tail)
    // ---- the rest
    void* fextra;
    void* pos_delta;
    void* old_delta;
    double* cosz;                  // [64*nwaves] per-lane cos(2 pi z / Lz) cache of the current step
    const double* seg_mass;        // [2*num segments] (mass, 1/mass) of each COM segment (static; vv_host.hpp)
    const int* seg_base;           // [nwaves+1] segments in the waves before this one: segment index of a lane = seg_base[wave] + leader lanes below it
    double* comw;                  // [num segments] mass-weighted mean of cos(kz) over the same segment (A_KE_MOM -> B_KE_MOM)
    const double* slot_m;           // [64*nwaves] RECIP(velm.w) of the lane's particle in the mode's `mixed` type, widened (0 = massless / idle)
    const double* slot_f;           // [64*nwaves] Drude-pair lanes: invTotalMass * own mass (K/drudeNoseHoover.cu:173-180), else 0
    const int32_t* slot_image;
    const int32_t* slot_rand;
    const int32_t* slot_shake;      // packed cluster word per lane (vv_host.hpp: SHAKE_WORD_*), NULL without in-kernel constraints
    const float4* slot_shake_param; // every lane of a cluster: 1/m_c, 0.5/(1/m_c+1/m_p), d^2, 1/m_p (SETTLE: the two distances)
    double shake_tol;
    const int32_t* slot_big;        // big-molecule index per lane (only with molecules larger than a wave)
    unsigned long long* bigacc;     // int64 fixed point [num_big][4]: sum m vx, m vy, m vz, m
    double big_scale, big_inv_scale;
    const float4* random;
    unsigned long long* acc_next;   // other parity: zeroed by B when it runs the chain inline
    NHDevState* nh_next;            // where an inline chain writes the advanced state
    int32_t acc_rows;                  // accumulator rows in use (4, or NUM_ACC with the cos moments): what kernel B has to clear
    int32_t acc_exclusive;             // kernel A: 1 = a launch of <= ACC_SLOTS blocks stores into its slots instead of adding atomically (launch_a clears it for larger grids)
    double fscale_vv;          // 0.5*dt/2^32 computed in double on the host (HOST:306)
    double drag, randf, drag_drude, randf_drude;   // HOST:835-839
    double efscale;            // E * AVOGADRO (HOST:978)
    double cos_accel;
    double inv_box_z;
    double mirror;
    double inv_mass_total;
    double acc_inv_scale[NUM_ACC];
    NHConst chain;                  // chain constants (used by B_CHAIN)
    Mailbox mb;                     // B_MAILBOX
    unsigned int* status;           // pinned host words, system-scope stores: [0] mailbox wait timed out, [1] accumulator overflow (sticky)
    long long* dbg;                 // timestamp buffer of the instrumented build (-DVV_KERNEL_TIMESTAMPS, tools/probes), else unused
    int32_t dbg_block, dbg_pad_;
    long long* dbg_span;            // instrumented build: [2 launch parities][blocks*8 waves][2] entry / exit stamps of every wave (100 MHz wall clock)
    int32_t dbg_parity, dbg_pad2_;
    uint32_t pos_bytes;             // size of the posq (= posqCorrection) array in bytes if below 4 GB, else 0: kernel A fetches the positions of
    int32_t gc_colors;              // constraint-cluster members through a buffer resource (load_wanted), other lanes fetch nothing; gc_colors:
                                    // colours of the general clusters' sweeps (A_GCONS / B_GCONS)
    double gc_omega;                // A_GCONS / B_GCONS: relaxation factor of the sweeps (vv_layout.h: GC_OMEGA_*)
    const int2* slot_vsite;         // B_VSITE: [64*waves] (site word, vv_layout.h: VS_WORD_*; record number) of the site the lane places
    const double* vsite_params;     // B_VSITE: [12*records] weights / local position of each site (vvhip_system_desc.virtual_site_params)
    const int32_t* vsite_atom;      // B_VSITE: [records] particle index of the site: a lane that places a site for its parent stores it there
    uint32_t flags_a;               // fused step (vv_kernel_b<.., SFA>): kernel A's stage set executed by the same launch, 0 otherwise (launch_b dispatches on it)
    int32_t fused_poll_delay;       // fused step: >= 0 pins the wait between a block's publish and its first poll round (units of 256 clocks); -1: NHDevState::rv_delay
    unsigned int* rv_late_cur;      // fused step: [ACC_SLOTS] uncached words, block b's = 1 if it needed a second poll round in THIS step ...
    const unsigned int* rv_late_prev;   // ... and the previous fused step's
    int32_t fused_late_shift, fused_pad_;   // the wait grows when more than blocks >> shift blocks were late
};

struct TetherArgs {
    const void* posq;
    const void* site;
    const void* velm;
    long long* force;
    const int2* slots;
    int32_t padded, nwaves;
    double k_tether, k_drude;
    long long* dbg_span;            // instrumented build (as KArgs::dbg_span)
    int32_t dbg_parity, dbg_pad_;
};

// Drude temperature report (vv_dev_report.inc, vvhip_drude_temperatures).  Sums in two-word fixed point: with y = x 2^unit_bits a term x
// is split into hi = floor(y) and lo = rint((y - hi) 2^frac_bits) (resolution 2^-(unit_bits + frac_bits), ~1e-18 at 0.1 M particles),
// the words are summed as integers (exact, in any order), and the host joins them.
// out[REP_*]: total of m|v|^2, of the pairs' mu|u_d - u_c|^2, of the molecules' |P|^2/M (hi, lo each), then the overflow flag.
enum { REP_TOTAL = 0, REP_DRUDE = 2, REP_COM = 4, REP_FLAG = 6, REP_WORDS = 7 };
struct ReportArgs {
    const void* velm;
    const int2* slots;
    const int32_t* lane_mol;        // [64*waves] shard-local molecule of the lane's particle, -1: none / massless
    const double* lane_mass;        // [64*waves] mass, 0 where massless
    const double* lane_mu;          // [64*waves] reduced mass of the pair on a Drude lane whose parent is in the same molecule, else 0
    const double* mol_mass;         // [nmol] molecule masses (> 0)
    const int4* cross;              // [ncross] (Drude, parent, molecule of the Drude, of the parent) of pairs across two molecules
    const double* cross_mu;         // [ncross]
    long long* mol_p;               // [nmol][6] momentum (x, y, z) as (hi, lo) word pairs
    long long* out;                 // [REP_WORDS]
    int32_t nwaves, nmol, ncross, frac_bits;
    double unit, frac_scale;        // 2^unit_bits, 2^frac_bits
    double inv_unit, inv_full;      // 2^-unit_bits, 2^-(unit_bits + frac_bits)
    double limit;                   // largest |term| taken (beyond it, or NaN: the flag)
};

// Series row (vv_dev_report.inc: vv_kernel_series_append, include/vvhip.h: vvhip_series_row).  The row index is read from the device-side
// cursor, so a replayed graph (same arguments every time) appends where the last row ended.
struct SeriesArgs {
    long long* rep_out;             // [REP_WORDS] the report's result words, zeroed after they are copied; null: no Drude part
    long long* rep_mol_p;           // [rep_mol_words] the report's momentum words, zeroed for the next row
    const vvhip_nh_state* nh;       // the thermostat copy current after the step; null: no thermostat part
    vvhip_series_row* rows;         // [capacity]
    unsigned long long* cursor;     // [0] rows appended since the start / last reset (past capacity too), [1] rows dropped
    int64_t rep_mol_words;
    int32_t capacity, pad_;
    double box[3], cos_acceleration;
};

// Removal of the centre-of-mass velocity (vv_dev_cmm.inc, vvhip_cm_motion_*): V = sum m v / sum m over every massive lane, v -= V.
// The three momentum sums use the report's two-word fixed point (ReportArgs: each term m v_c is split on its own into hi = floor(y),
// lo = rint((y - hi) 2^frac_bits), y = m v_c 2^unit_bits, and the words are summed as integers), so P is the same bits whatever the
// launch shape or the wave layout.  Quantisation: a term is rounded to 2^-(unit_bits + frac_bits) Da nm/ps, half of that at most per
// term; with unit_bits = 16, frac_bits = 61 - bits(n) and n < 2^bits(n) massive particles
//     |P_fixed - P_exact| <= n 2^-(78 - bits(n)) < 2^(2 bits(n) - 78) Da nm/ps      (5.7e-14 at 0.1 M particles, 9e-10 at 9 M)
// and |V - P_exact / M| <= that / M + 3 ulp(V) (the join of the two words, the product with the host's 1 / M): below 1e-19 nm/ps at
// every size a GPU holds -- ten orders of magnitude under a thermal speed.  A term beyond ReportArgs::limit (or NaN) raises the bad word
// and the removal is skipped: nothing is subtracted.
// words[0..5] = (hi, lo) of P_x, P_y, P_z; [CMM_BAD] != 0: a term was out of range; [CMM_TICKET] = blocks of the subtract kernel that
// have read the words (the last one zeroes all eight: the scratch is zero between removals without a memset in the stream).
enum { CMM_BAD = 6, CMM_TICKET = 7, CMM_WORDS = 8 };
struct CmmDevRecord {
    long long removals, skipped;    // removals done / skipped because of the bad word
    double last_v[3];               // the V of the last removal (NaN after a skipped one)
};
struct CmmArgs {
    ReportArgs rep;                 // velm, slots, lane_mass, nwaves and the fixed point; the report's other tables are not read
    long long* words;               // [CMM_WORDS]
    CmmDevRecord* rec;
    double inv_total_mass;          // 1 / sum of the masses > 0, formed in double on the host (0 without massive particles)
};

// Monte Carlo barostat (vv_dev_barostat.inc, vvhip_barostat_scale): every molecule moved rigidly so that its geometric centre scales with the
// box.  A component X of a stored position becomes Q = llrint(X 2^frac_bits); a molecule's Q are summed as integers (exact, in any order,
// the same bits whatever the launch shape, the wave layout or the shard split) into words[BARO_HEAD + 3 m + component].  frac_bits = 40 -
// ceil(log2(largest molecule of the whole System)) and |X| < 2^22 nm keep |sum| < 2^62; a position beyond that (or not finite) raises
// words[BARO_BAD] and nothing is stored.  Resolution of a centre: 2^-frac_bits nm (< 1e-9 nm for molecules of up to 1024 particles).
enum { BARO_BAD = 0, BARO_HEAD = 1 };
struct BarostatArgs {
    void* posq;                     // real4 [shard particles]
    void* corr;                     // real4, mixed precision only (else null)
    const int2* slots;
    const int32_t* lane_mol;        // [64*waves] shard-local molecule of the lane's particle, -1: idle lane
    const int2* laneless;           // [nlaneless] (shard-relative index, shard-local molecule) of the particles without a lane
    const double* mol_count;        // [nmol] particles per molecule n_m, as double
    unsigned long long* words;      // [BARO_HEAD + 3 nmol], zero on entry of the sum kernel
    int32_t nwaves, nlaneless, nmol, frac_bits;
    double scale, inv_scale;        // 2^frac_bits, 2^-frac_bits
    double e[3];                    // scale[a] - 1.0 per axis, formed in double on the host; 0: the axis keeps its stored bits
};

// Maxwell-Boltzmann start velocities (vv_dev_thermalize.inc, vvhip_set_velocities_to_temperature): a pure function of the seed, the GLOBAL
// particle index (shard_begin + the slot's index), the masses and the two temperatures -- nothing of the wave layout, the launch shape or
// the shard split enters.  lane_mass is the report's table (ReportArgs); a Drude pair shares a wave (META_PARTNER_SHIFT), so the partner's
// mass and index come from its lane.  Massless particles that have no lane (image particles, hosted virtual sites) are listed in `laneless`.
struct ThermalizeArgs {
    void* velm;
    const int2* slots;
    const double* lane_mass;        // [64*waves] mass, 0 where massless
    const int32_t* laneless;        // [nlaneless] shard-relative indices of the massless particles without a lane: velm.xyz = 0
    int32_t nwaves, nlaneless;
    int32_t shard_begin, drude_aware;
    uint32_t key[2];                // seed & 0xffffffff, seed >> 32
    double kt, kt_drude;            // R T and R T_D, kJ/mol (the products formed in double on the host)
};

// State digest (vv_dev_digest.inc, vvhip_state_digest): sum over the section's 32-bit words of mix((base + j) << 32 | w[j]), mod 2^64
// (include/vvhip.h: "Digest").  `out` must be zero on entry; the launch adds to it.
struct DigestArgs {
    const unsigned int* words;      // the section, 4-byte aligned
    unsigned long long nwords;      // base + nwords <= 2^32
    unsigned long long base;
    unsigned long long* out;
};

// Trajectory frame (vv_dev_frames.inc, include/vvhip.h: vvhip_frames_*).  The frame index is read from the device-side cursor, so a
// replayed graph (same arguments every time) records where the last frame ended.
struct FrameArgs {
    const void* posq;               // real4 [shard particles]
    const void* corr;               // real4, mixed precision only (else null)
    const void* velm;               // mixed4
    const int32_t* subset;          // [n] shard-relative indices of the recorded particles, ascending; null: particle i is index i
    unsigned char* frames;          // [capacity] frames of frame_bytes each (+ the guard frame)
    unsigned long long* cursor;     // [0] frames counted since the start / last reset (past capacity too), [1] frames dropped
    int64_t frame_bytes;
    int64_t off_positions, off_velocities;      // of the x plane inside a frame, -1: not recorded
    int32_t n, plane_stride;        // recorded particles; elements per component plane
    int32_t capacity, pad_;
    double box[3];
};

// Profile sample (vv_dev_profile.inc, include/vvhip.h: vvhip_profile_* states the arithmetic).  The sample count is read from the
// device-side words, so a replayed graph (same arguments every time) stops adding at max_samples.
enum { PROFILE_SAMPLES = 0, PROFILE_DROPPED = 1, PROFILE_OUT_OF_RANGE = 2, PROFILE_HEAD = 3 };      // the words in front of the table
struct ProfileArgs {
    const void* posq;               // real4 [shard particles]
    const void* corr;               // real4, mixed precision only (else null)
    const void* velm;               // mixed4 (read only with a velocity quantity on)
    const int32_t* index;           // [n] shard-relative indices of the recorded particles, ascending; null: particle i is index i
    const unsigned char* group;     // [n] group of recorded particle i, 255: not recorded (GROUPED kernels only)
    const double* mass;             // [n] the System's mass of recorded particle i (read only with a mass-weighted quantity on)
    long long* words;               // [PROFILE_HEAD + table_words]: samples, dropped, out_of_range, then table[group][row][nbins]
    int64_t max_samples;
    int32_t n, nbins;               // recorded particles; bins
    int32_t axis, mask;             // VVHIP_PROFILE_* bits
    int32_t rows, table_words;      // rows per group; num_groups * rows * nbins
    double inv_L;                   // 1.0 / box[axis]
    double scale[4], limit[4];      // 2^frac_bits and the limit of charge, mass, momentum, kinetic
};

// MSD sample (vv_dev_msd.inc, include/vvhip.h: vvhip_msd_* states the units, the schedule and the terms).  The sample ordinal and the
// origin floor are read from the device-side words, so a replayed graph (same arguments every time) finds the origins where the last
// sample left them and stops adding at max_samples.
enum { MSD_SAMPLES = 0, MSD_DROPPED = 1, MSD_OUT_OF_RANGE = 2, MSD_FLOOR = 3, MSD_HEAD = 4 };      // the words in front of the table
struct MsdArgs {
    const void* posq;               // real4 [shard particles]
    const void* corr;               // real4, mixed precision only (else null)
    const int32_t* index;           // particles: [n] shard-relative index of unit u, null: unit u is particle u.  Molecules: the member lists
    const int32_t* first;           // molecules: [n + 1] unit u's members are index[first[u]] .. index[first[u + 1] - 1], ascending
    const double* weight;           // molecules: the mass of every member, beside index
    const double* total;            // molecules: [n] M, the members' masses summed in their order
    const unsigned char* group;     // [n] group of unit u (GROUPED kernels only)
    long long* words;               // [MSD_HEAD + table_words]: samples, dropped, out_of_range, origin floor, then table[group][lag][4]
    double* ring;                   // [num_origins][3][stride] the origins' positions, behind the table in the same allocation
    int64_t max_samples;
    int32_t n, stride;              // recorded units; n rounded up to 16
    int32_t num_lags, origin_every;
    int32_t num_origins, table_words;      // ceil(num_lags / origin_every); num_groups * num_lags * 4
    int32_t wave_reduce, pad_;      // 1: a wave whose lanes share a group adds its four sums once
    double scale, limit;            // 2^frac_bits; |delta| at or beyond it is out of range
};

// RDF sample (vv_dev_rdf.inc, include/vvhip.h: vvhip_rdf_* states the sites, the classes, the arithmetic and the bins).  The sample count is
// read from the device-side words, so a replayed graph (same arguments every time) stops adding at max_samples; whether the box still
// holds r_max is the host's decision at enqueue (`live`): the box is an argument, and a box that changes drops the captured graphs.
enum { RDF_SAMPLES = 0, RDF_DROPPED = 1, RDF_INVALID = 2, RDF_INV_VOLUME = 3, RDF_HEAD = 4 };      // the words in front of the table ([3]: the bits of a double)
constexpr int RDF_TILE = 256;       // sites per tile = threads per block of the pair kernel
constexpr int RDF_MAX_CLASSES = 32, RDF_MAX_GROUPS = 16;      // (the arrays of vvhip_rdf_layout)
// A block's work: the sites i0 .. i0 + ni - 1 (one per thread, 1 <= ni <= RDF_TILE) of class cls's group a against the sites b0 + j0 ..
// b0 + j1 - 1 of its group b, which starts at site b0; same != 0: ga == gb, and a pair counts where the i-site's index is below the
// j-site's (the host lists no j-site below i0)
struct RdfItem { int32_t cls, same, i0, ni, b0, j0, j1, pad_; };
struct RdfArgs {
    const void* posq;               // real4 [shard particles]
    const void* corr;               // real4, mixed precision only (else null)
    const int32_t* index;           // [n] particle of site s; the sites are ordered by group, inside a group ascending by particle
    const int32_t* mol;             // [n] molecule of site s (exclusion on, else null)
    const RdfItem* items;           // [num_items]
    double* scratch;                // [3][stride] the sites' x, y, z planes, rewritten by every sample's gather
    long long* words;               // [RDF_HEAD + num_classes * nbins]: samples, dropped, invalid, inv_volume_sum, then table[class][nbins]
    int64_t max_samples;
    int32_t n, stride;              // sites; n rounded up to 16
    int32_t nbins, num_items;
    int32_t copies, live;           // private histograms per block (1, or one per wave); 0: the box no longer holds r_max, the sample is dropped
    int32_t max_jsites, pad_;       // no item has more j-sites: RDF_TILE * max_jsites pairs fit a private histogram's 32-bit words
    double L[3], inv_L[3];          // the plan's box at enqueue and 1.0 / L[a], formed on the host
    double dr, cut2;                // r_max / nbins; e(nbins)
    float inv_dr;                   // 1 / dr, for the guess of the bin only
    float pad2_;
    double inv_volume;              // 1.0 / ((Lx * Ly) * Lz), formed on the host
};

// Current sample (vv_dev_current.inc, include/vvhip.h: vvhip_current_* states the sums, the table and the order of its float64 adds).  The
// sample ordinal, the origin floor and the ring are device-side words, so a replayed graph (same arguments every time) finds the origins
// where the last sample left them and stops adding at max_samples.  One allocation: head, sums, table, ring, holds.
enum { CUR_SAMPLES = 0, CUR_DROPPED = 1, CUR_OUT_OF_RANGE = 2, CUR_INVALID = 3, CUR_FLOOR = 4, CUR_INV_VOLUME = 5,      // ([5]: the bits of a double)
       CUR_BAD = 6,                 // the out-of-range particles of the sample in flight (the advance kernel zeroes it)
       CUR_HEAD = 8 };              // the words in front of the sample's sums
constexpr int CUR_MAX_GROUPS = 8;
struct CurrentArgs {
    const void* posq;               // real4 [particles]
    const void* corr;               // real4, mixed precision only (else null)
    const void* velm;               // mixed4
    const int32_t* index;           // [n] the recorded particles, ordered by group, inside a group ascending
    const double* weight;           // [n] beside index
    const unsigned char* group;     // [n] beside index
    long long* words;               // [CUR_HEAD] head, [G][6] the sample's sums P_x P_y P_z U_x U_y U_z, then the table, the ring, the holds
    long long* table;               // [num_lags + 1][row_words]
    long long* ring;                // [num_origins][G][6] the origins' sums
    long long* hold;                // [num_origins] the ordinal of the sample a slot holds, -1: none that is usable
    long long* slabs;               // two-level form: [num_slabs][G * 6 + 1] every reduce block's sums and bad count, rewritten by every sample; null: one level
    int64_t max_samples;
    int32_t n, num_groups;
    int32_t num_lags, origin_every;
    int32_t num_origins, row_words; // ceil(num_lags / origin_every); 1 + 3 (ND + NC)
    int32_t num_slabs, pad_;        // the reduce's blocks (set by the launcher)
    double scale_p, scale_v;        // 2^Fp, 2^Fv
    double inv_scale_p, inv_scale_v;
    double limit_p, limit_v;        // |X_a| / |v_a| at or beyond it is out of range
    double inv_volume;              // 1.0 / ((Lx * Ly) * Lz), formed on the host
};

// Density-mode sample (vv_dev_modes.inc, include/vvhip.h: vvhip_modes_* states the turns, the phase, the phasor, the sums, the table and the
// order of its float64 adds).  As for a current sample the ordinal, the origin floor and the ring are device-side words.  One allocation:
// head, sums, table, ring, holds; the turns are scratch of their own, rewritten by every sample.
enum { MODES_SAMPLES = 0, MODES_DROPPED = 1, MODES_OUT_OF_RANGE = 2, MODES_INVALID = 3, MODES_FLOOR = 4,
       MODES_BOX_SUM = 5,           // [5 .. 7]: the bits of three doubles
       MODES_BAD = 8,               // the out-of-range sites of the sample in flight (the advance kernel zeroes it)
       MODES_HEAD = 12 };           // the words in front of the sample's sums
constexpr int MODES_MAX_GROUPS = 8, MODES_MAX_K_TILE = 1024;
// A block's work: the sites s0 .. s1 - 1 of the compact list, all of group `group`, against the modes k0 .. k1 - 1 (k1 - k0 <= MODES_MAX_K_TILE,
// s1 - s0 <= threads per block * sites per thread)
struct ModesItem { int32_t group, s0, s1, k0, k1, pad_[3]; };
struct ModesArgs {
    const void* posq;               // real4 [particles]
    const void* corr;               // real4, mixed precision only (else null)
    const int32_t* index;           // [n] the recorded sites, ordered by group, inside a group ascending by particle
    const double* weight;           // [n] beside index
    const int32_t* modes;           // [num_modes][3]
    const ModesItem* items;         // [num_items]
    unsigned int* turns;            // [3][stride] the sites' T_x, T_y, T_z planes, rewritten by every sample's gather
    long long* words;               // [MODES_HEAD] head, then sums[G][K][2] (A, B), the table, the ring, the holds
    long long* table;               // [num_lags + 1][row_words]
    long long* ring;                // [num_origins][G][K][2] the origins' sums
    long long* hold;                // [num_origins] the ordinal of the sample a slot holds, -1: none that is usable
    int64_t max_samples;
    int32_t n, stride;              // sites; n rounded up to 16
    int32_t num_groups, num_modes;
    int32_t num_lags, origin_every;
    int32_t num_origins, row_words; // ceil(num_lags / origin_every); 1 + G^2 K
    int32_t num_items, pad_;
    double inv_L[3], box[3];        // 1.0 / L[a], formed on the host, and the plan's box at enqueue
    double limit;                   // |X_a| at or beyond it is out of range
    double scale, inv_scale;        // 2^F, 2^-F
};

// Contact sample (vv_dev_contacts.inc, include/vvhip.h: vvhip_contacts_* states the sites, the classes, the contact, the slots and the table).
// The ordinal and the slots' ordinals are device-side words, so a replayed graph (same arguments every time) finds the origins where the last
// sample left them and stops adding at max_samples; whether the box still holds the largest cutoff is the host's decision at enqueue
// (`live`), as for an RDF sample.  One allocation: head, table, ord, the ring of origins, the ring of surviving contacts (vv_layout.h:
// ContactsLayout); the sample's matrix and the gather's planes are scratch of their own, rewritten by every sample.
enum { CONTACTS_SAMPLES = 0, CONTACTS_DROPPED = 1, CONTACTS_INVALID = 2, CONTACTS_HEAD = 4 };      // the words in front of the table
constexpr int CONTACTS_MAX_ROWS_PER_TILE = 1024;      // the mask kernel's staged rows: 28 B each in LDS
struct ContactsArgs {
    const void* posq;               // real4 [particles]
    const void* corr;               // real4, mixed precision only (else null)
    const int32_t* index;           // [n] particle of site s; the sites are ordered by group, inside a group ascending by particle
    const int32_t* mol;             // [n] molecule of site s (exclusion on, else null)
    const ContactsMaskItem* mask_items;     // [num_mask_items]
    const ContactsCorrItem* corr_items;     // [num_corr_items]
    double* scratch;                // [3][stride] the sites' x, y, z planes, rewritten by every sample's gather
    unsigned long long* mask;       // [sample_words] h(j), rewritten by every sample's mask kernel
    long long* words;               // [CONTACTS_HEAD] samples, dropped, invalid, then the table, ord and the rings
    long long* table;               // [num_classes][num_lags][4]
    long long* ord;                 // [num_origins] the ordinal of the sample a slot holds, -1: none
    unsigned long long* origin;     // [num_origins][sample_words]
    unsigned long long* cont;       // [num_origins][sample_words], null without the continuous correlation
    int64_t max_samples;
    int64_t sample_words;
    int32_t n, stride;              // sites; n rounded up to 16
    int32_t num_mask_items, num_corr_items;
    int32_t num_classes, num_lags;
    int32_t origin_every, num_origins;
    int32_t live, skip_zero;        // 0: the box no longer holds the largest cutoff, the sample is dropped; 1: a zero origin word costs no further load
    int32_t rows_per_tile, pad_;
    double L[3], inv_L[3];          // the plan's box at enqueue and 1.0 / L[a], formed on the host
    double cut2[CONTACTS_MAX_CLASSES];               // r_cut[c] * r_cut[c]
    int64_t class_offset[CONTACTS_MAX_CLASSES];      // ContactsLayout
    int32_t rows_padded[CONTACTS_MAX_CLASSES];
    int32_t rows[CONTACTS_MAX_CLASSES], cols[CONTACTS_MAX_CLASSES];          // N_a, N_b
    int32_t first_row[CONTACTS_MAX_CLASSES], first_col[CONTACTS_MAX_CLASSES];  // where the class's groups start in the site list
};

// Autocorrelation sample (vv_dev_acf.inc, include/vvhip.h: vvhip_acf_* states the units and their vector, the schedule and the terms).  The
// sample ordinal and the origin floor are read from the device-side words, so a replayed graph (same arguments every time) finds the
// origins where the last sample left them and stops adding at max_samples.  One allocation: head, table, ring.
enum { ACF_SAMPLES = 0, ACF_DROPPED = 1, ACF_OUT_OF_RANGE = 2, ACF_FLOOR = 3, ACF_HEAD = 4 };      // the words in front of the table
enum { ACF_VELOCITY_PARTICLES = 0, ACF_VELOCITY_MOLECULES = 1, ACF_ORIENTATION = 2 };               // = VVHIP_ACF_*
constexpr int ACF_MAX_SLOTS_IN_FLIGHT = 8;
struct AcfArgs {
    const void* velm;               // mixed4 [shard particles] (the velocity modes)
    const void* posq;               // real4 [shard particles] (orientation mode)
    const void* corr;               // real4, mixed precision only (else null)
    const int32_t* index;           // particles: [n] shard-relative index of unit u, null: unit u is particle u.  Molecules: the member
                                    // lists.  Orientation: [2 n] head and tail of unit u at 2 u, 2 u + 1
    const int32_t* first;           // molecules: [n + 1] unit u's members are index[first[u]] .. index[first[u + 1] - 1], ascending
    const double* weight;           // molecules: the mass of every member, beside index
    const double* total;            // molecules: [n] M, the members' masses summed in their order
    const unsigned char* group;     // [n] group of unit u (GROUPED kernels only)
    long long* words;               // [ACF_HEAD + table_words]: samples, dropped, out_of_range, origin floor, then table[group][lag][row_words]
    double* ring;                   // [num_origins][3][stride] the origins' vectors, behind the table in the same allocation
    int64_t max_samples;
    int32_t n, stride;              // recorded units; n rounded up to 16
    int32_t num_lags, origin_every;
    int32_t num_origins, table_words;      // ceil(num_lags / origin_every); num_groups * num_lags * row_words
    int32_t wave_reduce, slots_in_flight;  // 1: a wave whose lanes share a group adds its sums once; ring loads issued together, 1 .. ACF_MAX_SLOTS_IN_FLIGHT
    double scale, limit;            // 2^frac_bits; the velocity modes: |component| at or beyond it is bad
};

// Self van Hove sample (vv_dev_vanhove.inc, include/vvhip.h: vvhip_vanhove_* states the units, the schedule, the bins and the moments).  The
// sample ordinal and the origin floor are read from the device-side words, as for the MSD.  One allocation: count words, head[G][L][6],
// hist[G][L][num_bins], ring.
enum { VANHOVE_SAMPLES = 0, VANHOVE_DROPPED = 1, VANHOVE_OUT_OF_RANGE = 2, VANHOVE_FLOOR = 3, VANHOVE_HEAD = 4 };      // the words in front of the table
enum { VANHOVE_PAIRS = 0, VANHOVE_BELOW = 1, VANHOVE_BEYOND = 2, VANHOVE_R2 = 3, VANHOVE_R4_HI = 4, VANHOVE_R4_LO = 5, VANHOVE_ROW = 6 };   // the words of head[g][l]
constexpr int VANHOVE_MAX_BINS = 1024;
constexpr int VANHOVE_LDS_WORDS = 4096;      // the block's private histogram: 32-bit words, 16 KiB (num_bins x the groups that fit; vv_dev_vanhove.inc)
struct VanHoveArgs {
    const void* posq;               // real4 [shard particles]
    const void* corr;               // real4, mixed precision only (else null)
    const int32_t* index;           // as MsdArgs: particles [n] or null; molecules: the member lists
    const int32_t* first;           // molecules: [n + 1]
    const double* weight;           // molecules: the mass of every member, beside index
    const double* total;            // molecules: [n] M
    const unsigned char* group;     // [n] group of unit u (GROUPED kernels only); ascending in u
    const double* e2;               // [num_bins + 1] the squared edges
    long long* words;               // [VANHOVE_HEAD + head_words + hist_words]
    double* ring;                   // [num_origins][3][stride] the origins' positions, behind the table in the same allocation
    int64_t max_samples;
    int64_t head_words;             // num_groups * num_lags * 6: where hist starts behind the count words
    int32_t n, stride;              // recorded units; n rounded up to 16
    int32_t num_lags, origin_every;
    int32_t num_origins, num_bins;  // ceil(num_lags / origin_every); 1 .. VANHOVE_MAX_BINS
    int32_t wave_reduce, lds_groups;// 1: a wave whose lanes share a group adds its six head words once; groups whose bins the block's LDS histogram holds, 0: every increment is a global add
    double scale2, scale_hi, scale_lo, limit;      // 2^frac2_bits, 2^r4_hi_bits, 2^r4_lo_bits; |delta| at or beyond limit is out of range
};

// Distinct van Hove sample (vv_dev_vanhove_distinct.inc, include/vvhip.h: vvhip_vanhove_distinct_* states the sites, the classes, the
// schedule, the arithmetic and the bins).  The sample ordinal and the origin floor are read from the device-side words, as for the self
// recorder; whether the box still holds r_max is the host's decision at enqueue (`live`), as for an RDF sample.  One allocation: count
// words, head[num_lags + 1][2], hist[num_classes][num_lags + 1][nbins], then num_origins + 2 plane sets double[3][stride]: the ring of
// num_origins + 1 slots and the spare set of a sample that is no origin.  The work items are the RDF's (RdfItem; same != 0: ga == gb, the
// item lists every j-site and the pair of a site with itself is masked).
enum { VHD_SAMPLES = 0, VHD_DROPPED = 1, VHD_INVALID = 2, VHD_FLOOR = 3, VHD_HEAD = 4 };      // the words in front of the table
enum { VHD_VISITS = 0, VHD_INV_VOLUME = 1, VHD_ROW = 2 };                                     // the words of head[l] ([1]: the bits of a double)
struct VhdArgs {
    const void* posq;               // real4 [shard particles]
    const void* corr;               // real4, mixed precision only (else null)
    const int32_t* index;           // [n] particle of site s; the sites are ordered by group, inside a group ascending by particle
    const int32_t* mol;             // [n] molecule of site s (exclusion on, else null)
    const RdfItem* items;           // [num_items]
    long long* words;               // [VHD_HEAD + head_words + hist_words]
    double* ring;                   // [num_origins + 2][3][stride], behind the table in the same allocation
    int64_t max_samples;
    int64_t head_words;             // (num_lags + 1) * 2: where hist starts behind the count words
    int32_t n, stride;              // sites; n rounded up to 16
    int32_t nbins, num_items;
    int32_t num_lags, origin_every;
    int32_t num_origins, copies;    // R = ceil(num_lags / origin_every); private histograms per block (1, or one per wave)
    int32_t live, max_jsites;       // 0: the box no longer holds r_max, the sample is dropped; no item has more j-sites
    double L[3], inv_L[3];          // the plan's box at enqueue and 1.0 / L[a], formed on the host
    double dr, cut2;                // r_max / nbins; e(nbins)
    float inv_dr;                   // 1 / dr, for the guess of the bin only
    float pad_;
    double inv_volume;              // 1.0 / ((Lx * Ly) * Lz), formed on the host
};

// Spatial distribution sample (vv_dev_sdf.inc, include/vvhip.h: vvhip_sdf_* states the frames, the sites, the classes, the arithmetic and
// the voxels).  The sample count is read from the device-side words and whether the box still holds the cube is the host's decision at
// enqueue (`live`), as for an RDF sample.  The work items are the RDF's (RdfItem; i: frames of the class's frame group, j: sites of its
// site group, same = 0).  Scratch: the sites' planes double[3][stride], then the frames' double[SDF_FRAME_PLANES][fstride].
enum { SDF_SAMPLES = 0, SDF_DROPPED = 1, SDF_INVALID = 2, SDF_BAD_FRAMES = 3, SDF_INV_VOLUME = 4, SDF_VISITS = 5, SDF_HEAD = 21 };      // the words in front of the table ([4]: the bits of a double; [5 .. 20]: frame_visits)
constexpr int SDF_MAX_GROUPS = 16, SDF_MAX_CLASSES = 16, SDF_MAX_BINS = 128;      // (the arrays of vvhip_sdf_layout and vvhip_sdf_counts)
constexpr int SDF_FRAME_PLANES = 13;      // origin, e1, e2, e3, and the frame's cutoff for the pair kernel's cheap test
static_assert(SDF_VISITS + SDF_MAX_GROUPS == SDF_HEAD, "");
struct SdfArgs {
    const void* posq;               // real4 [shard particles]
    const void* corr;               // real4, mixed precision only (else null)
    const int32_t* index;           // [n] particle of site s; the sites are ordered by site group, inside a group ascending by particle
    const int32_t* mol;             // [n] molecule of site s (exclusion on, else null)
    const int32_t* frames;          // [nf][3] particles o, a, b of frame f; the frames are ordered by frame group, inside a group as given
    const int32_t* fmol;            // [nf] molecule of frame f (exclusion on, else null)
    const unsigned char* fgroup;    // [nf] frame group of frame f
    const RdfItem* items;           // [num_items]
    double* scratch;                // [3][stride], then [SDF_FRAME_PLANES][fstride]: rewritten by every sample's gather
    long long* words;               // [SDF_HEAD + num_classes * nbins^3]
    int64_t max_samples;
    int32_t n, stride;              // sites; n rounded up to 16
    int32_t nf, fstride;            // frames; nf rounded up to 16
    int32_t nbins, num_items;
    int32_t live, max_jsites;       // 0: the box no longer holds the cube, the sample is dropped; no item has more j-sites
    double L[3], inv_L[3];          // the plan's box at enqueue and 1.0 / L[a], formed on the host
    double h, inv_w;                // extent; (double) nbins / (2.0 * extent)
    double cut2;                    // (3 h^2) (1 + 2^-20): the cheap test's cutoff of an exactly orthonormal frame
    double inv_volume;              // 1.0 / ((Lx * Ly) * Lz), formed on the host
};

}  // namespace vv
