// vv_dev_kernel_b.inc -- part of vv_device.inc: kernel B ("consume") and the one-launch step: rendezvous words, thermostat wave, tile waves
// ================================================================================ kernel B
// Rendezvous words of the fused step: row k (a quantity), slot s (a block) -- the layout of the two-launch step's accumulators.
__device__ __forceinline__ int rv_index(int k, int slot) { return k * ACC_SLOTS + slot; }
// The word (round 6): {tag:6 | payload:58} with payload = q + 2^57 -- offset binary; q is the block's fixed-point sum, |q| < 2^57 -- and EVERY
// one of the ACC_SLOTS slots of a row in use carries a word of the step: the slots beyond the grid get the neutral word (q = 0) from the first
// blocks (rv_pad_slots).  Then (i) a poller holds a complete row when the smallest and the largest HIGH word of what it loaded both carry the
// step's tag -- one v_min3_u32 / v_max3_u32 pair per three words, no per-slot mask against the grid size --, and (ii) the row's total is the
// WRAPPING sum of the 256 raw words: 256 (tag << 58) = tag << 66 and 256 << 57 = 2^65 vanish modulo 2^64, and |sum of q| < 2^62 by the
// accumulators' headroom -- no decoding, no masking.  Round 5 decoded and masked every word behind the poll: with the tag test ~85 instructions
// of one wave, at ~5 clocks per instruction of a single wave (tools/probes/icache_probe.cpp) 0.18 us on the critical path of every step.
// "a rendezvous of this plan has failed" (uncached device word behind the two rows of "polled twice" words -- the host's kRvDeadWord, vv_plan.hpp): raised by the wave whose wait ran
// out, next to the sticky word in host memory; every later poll round that is incomplete gives up at once instead of waiting its own 0.2 s --
// a 100-step graph behind the failure drains in microseconds, and the host (which restores its snapshot and goes on with two launches per
// step, vv_api.cpp: recovery) gets the GPU back.
__device__ __forceinline__ unsigned int* rv_dead_word(const KArgs& a) {
    return const_cast<unsigned int*>(a.rv_late_cur < a.rv_late_prev ? a.rv_late_cur : a.rv_late_prev) + 2 * ACC_SLOTS;
}
constexpr unsigned long long RV_BIAS = 1ull << 57;
__device__ __forceinline__ unsigned long long rv_word(unsigned long long tag58, long long q) { return tag58 + RV_BIAS + (unsigned long long) q; }
__device__ __forceinline__ unsigned rv_hi(unsigned long long w) { return (unsigned) (w >> 32); }
// smallest / largest high word of N words (the backend forms v_min3_u32 / v_max3_u32 from the nested calls)
template <int N>
__device__ __forceinline__ void rv_tag_range(const unsigned long long (&w)[N], unsigned& lo, unsigned& hi) {
    static_assert(N % 4 == 0, "whole rows");
#pragma unroll
    for (int i = 0; i + 1 < N; i += 2) { lo = min(min(lo, rv_hi(w[i])), rv_hi(w[i + 1])); hi = max(max(hi, rv_hi(w[i])), rv_hi(w[i + 1])); }
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long dpp_fetch_u64(unsigned long long x) {
    const unsigned lo = (unsigned) dpp_fetch32<CTRL, ROW_MASK>((int) (unsigned) x);
    const unsigned hi = (unsigned) dpp_fetch32<CTRL, ROW_MASK>((int) (unsigned) (x >> 32));
    return ((unsigned long long) hi << 32) | lo;
}
// wave total of a 64-bit word per lane, modulo 2^64, in every lane
__device__ __forceinline__ unsigned long long wrap_reduce_lane_sum(unsigned long long s) {
    s += dpp_fetch_u64<0x111, 0xF>(s);
    s += dpp_fetch_u64<0x112, 0xF>(s);
    s += dpp_fetch_u64<0x114, 0xF>(s);
    s += dpp_fetch_u64<0x118, 0xF>(s);
    s += dpp_fetch_u64<0x142, 0xA>(s);
    s += dpp_fetch_u64<0x143, 0xC>(s);
    return __shfl(s, 63, 64);
}
__device__ __forceinline__ void lane_swap32(unsigned long long& x, unsigned long long& y) {
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned) x, (unsigned) y, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned) (x >> 32), (unsigned) (y >> 32), false, false);
    x = ((unsigned long long) hi[0] << 32) | lo[0]; y = ((unsigned long long) hi[1] << 32) | lo[1];
}
__device__ __forceinline__ void lane_swap16(unsigned long long& x, unsigned long long& y) {
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned) x, (unsigned) y, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned) (x >> 32), (unsigned) (y >> 32), false, false);
    x = ((unsigned long long) hi[0] << 32) | lo[0]; y = ((unsigned long long) hi[1] << 32) | lo[1];
}
// copies of the words (RV_REPLICAS, vv_args.hpp), each polled by its share of the blocks
constexpr int RV_REPLICA_WORDS = NUM_ACC * ACC_SLOTS;
// SFA != 0: the FUSED step -- this launch also executes kernel A's stage set SFA on its tiles, in front of an in-kernel rendezvous of the
// (co-resident) blocks that takes the place of the A -> B kernel boundary (see "fused step" below); pre_acc is then the rendezvous buffer.
constexpr int THERMO_HEAD_SLEEP = 8;      // x 64 clocks: how long the one-launch step's thermostat wave steps aside at the kernel's head (HEAD_ASIDE)
// MAP OF THIS KERNEL, in the order of its timeline (the body is ONE function on purpose: round 6 split it into forced-inline stage functions over
// register structs -- same operations, 125 bit-for-bit tests green -- and the compiled instances came out 1-6.5 % SLOWER (other selects, other schedule:
// C3 100.0 -> 96.2 k steps/s, C5 116 -> 108.6 k, C2 149 -> 142.9 k, profiles/r06m_split_ab.txt); the stages are lambdas and labelled sections instead):
//   preamble          instance facts (FUSED, FA_KICK, ...), the block's LDS, pattern rows
//   THERMOSTAT WAVE   (wave 0 of a block with B_CHAIN; returns at its end)
//     head            priority / stepping aside; which lane advances which temperature group (LANE_LOCAL)
//     load_batch      state, chain constants, accumulator slots [two launches: + chain_head]
//     thermostat_tail one-launch step: hoists -> BARRIER 1 -> block sums -> publish -> [idle accumulators, chain_head in the wait's shadow]
//                     -> poll (all rows in use) | fold -> [mailbox] -> 2KE -> chain with release_tiles (BARRIER 2) in its middle
//     record          block 0 stores the advanced thermostat and the wait's controller
//   TILE WAVES        (grid-stride loop; one pass in the one-launch step)
//     fetch           slot word, the tile's loads in one batch (positions behind the kick where kernel A's stages do not read them), role, masks
//     [B_KICK]        two launches: kernel A's kick again from the same bits
//     kernel A stages one-launch step: extra forces, kick, velocity constraints, Koenig-form sums -> LDS -> BARRIER 1
//     scale_prep      the factor-independent half of the scaling (early unless a bias must be removed first)
//     scales          BARRIER 2: the scale factors from LDS
//     kernel B stages bias removal, scaling, restore | classic first half | positions (+ constraints) | hard wall | virtual sites | stores | image mirror
template <class real, class mixed, uint32_t SF, uint32_t SFA = 0u>
__global__ void __launch_bounds__(512) vv_kernel_b(const int2* __restrict__ pre_slots, const int pre_nwaves, const int pre_wpb, const unsigned long long* __restrict__ pre_acc,
                                                   const NHDevState* __restrict__ pre_nh, const ChainLaneBlock* __restrict__ pre_lane_const, const int* __restrict__ pre_seg_base,
                                                   const KArgs a) {
    using real4 = typename Vec<real>::v4;
    using real3 = typename Vec<real>::v3;
    using mixed4 = typename Vec<mixed>::v4;
    using P = Prec<real>;
    using IO = PosIO<real, mixed>;
    const int lane = threadIdx.x & 63;
    const uint32_t F = SF ? SF : a.flags;
    // ---- fused step (round 5).  One launch per step where the grid is co-resident: every tile wave runs kernel A's stages (extra forces,
    // kick, velocity constraints, the Koenig-form kinetic-energy sums) on its tile and KEEPS the tile in registers; the block's partial
    // sums go -- through the very arithmetic of kernel A's tail, so the fixed-point words are the ones kernel A would have stored -- into
    // the block's slot of an uncached rendezvous buffer as {tag:6 | payload:58} words (flag and data in ONE 8-byte atomic store, the LL
    // idea of the mailbox); every block's thermostat wave polls all blocks' slots (one batch of loads per round), folds them with the
    // two-launch path's fold (integers: same totals) and advances the chain; the tile waves meanwhile hold velocity, force-free kick,
    // position and molecular COM velocity and finish with kernel B's stages.  Against A + B: no velm / force re-read, no COM-velocity
    // round trip through memory, no cold start of a second kernel, and the rendezvous costs what the kernel boundary cost
    // (tools/probes/rendezvous_probe.cpp: ~2.0 us for 251 blocks and three quantities).  Bit for bit the two-launch step.
    constexpr uint32_t FA = SFA;
    constexpr bool FUSED = SFA != 0u;
    static_assert(!FUSED || (SF != 0u && (SF & B_CHAIN) && (SF & B_SCALE) && !(SF & (B_KICK | B_PERIODIC | B_CZ_LOAD))), "fused step: kernel B's stage set must carry the thermostat wave");
    static_assert(!FUSED || ((SFA & A_KE) && !((SFA & A_KICK_FULL) && (SFA & A_KICK_HALF)) &&
                             !(SFA & (A_MTAB | A_PERIODIC | A_NOSTORE | A_UNBIAS_ACC | A_COMPART | A_CZ_LOAD | A_KE_PLAIN | A_POS1 | A_POSDELTA_VV | A_SHAKE_GS))),
                  "fused step: kernel A's stage set must be a kick (middle scheme: full; classic second half: half; classic first half: none) + the sums");
    constexpr bool FA_KICK = FUSED && (SFA & (A_KICK_FULL | A_KICK_HALF)) != 0;
    constexpr bool VV1_EARLY = FUSED && (SF & B_VV_KICK) != 0;      // classic first half in one launch: the VV kick's force and forceExtra come with the tile's batch
    __shared__ double sh_red[FUSED ? 8 : 1][NUM_ACC];       // the tile waves' partial sums (fused step)
    // The rendezvous' poll (thermostat_tail): every block's thermostat wave collects ALL rows in use itself, one batch of 4 loads per row per lane
    // and round, and folds them.  (Round 5 shared the rows out among the block's waves -- the tile waves have nothing to do until the scale factors
    // arrive -- behind a second barrier and a hand-over of the totals through LDS; since the rows add up without decoding (rv_word) round 6 measured
    // that a wash on the full boxes and a loss on a rank's share of a sharded run, and removed it.  TUNING_LOG.md has the numbers.)
    // Bounded: after ~0.2 s without the other blocks' words (they are not resident: the launch shape was wrong for this device, or another
    // process holds CUs) the wave raises the sticky flag and carries on -- the host reports the run as void, nothing hangs.
    // The first round is sent a little BEHIND the block's publish.  The blocks publish over ~0.4 us and a word is ~0.6 us on its way: a round
    // sent at once finds the late blocks' words missing in all but the last blocks, and a round is ~1.1 us with every block polling -- the
    // whole grid then leaves a round late.  Measured on one box, steps/s against the wait in units of 256 clocks (tools/probes/fused_delay.py,
    // one polling wave): C3 90.0 / 93.4 / 96.3 / 96.5 / 97.4 / 96.5 / 96.1 k at 0 / 3 / 4 / 5 / 6 / 7 / 8 (two launches 86.7 k), C5 104.5 -> 114.1 k
    // at 6, C2 132.5 -> 150.3 k at 5, C1 143.8 -> 159.1 k at 5, with HBonds (more skew between the blocks) best beyond 8.  The wait tunes
    // itself (rv_delay in the device-resident state): every block reports whether its thermostat wave needed a second round; many late blocks,
    // and the step after next waits one unit longer; 64 steps without a late block, one unit shorter.  a.fused_poll_delay >= 0 pins it.
    // Block layout.  With B_CHAIN the FIRST wave of every block is the block's thermostat wave: it folds the
    // accumulators and advances the NH chain (a ~2 us serial fp64 dependency chain) while the other waves of the
    // block load their particles and do the scale-independent preparation; one barrier joins them.  Without this,
    // every tile wave pays the chain on its own critical path (measured: 9.7 -> see DESIGN.md §7).
    const int nwb = pre_wpb;                      // = blockDim.x >> 6, preloaded (blockDim is a hidden kernel argument: an s_load)
    const bool has_cw = (F & B_CHAIN) != 0;
    // the thermostat wave is wave 0: the waves of a block start in order, and the block's critical path runs through this one
    const bool chain_wave = has_cw && (threadIdx.x >> 6) == 0;
    const int wib = (int) (threadIdx.x >> 6) - (has_cw ? 1 : 0);      // index among the block's tile waves
    const int tiles_per_block = has_cw ? nwb - 1 : nwb;
    __shared__ double sh_scales[4];
    double sc0 = 1.0, sc1 = 1.0, sc2 = 1.0, scb = 0.0;
    // Periodic layout: role words and pair mass fractions of the regions' pattern waves, copied into LDS once per block (kernel A)
    __shared__ unsigned sh_pat_meta[4][64];
    __shared__ double sh_pat_f[4][64];
    __shared__ unsigned sh_pat_shake[4][64];        // constraint cluster words / parameters of the pattern waves (B_SHAKE)
    __shared__ float4 sh_pat_prm[4][64];
    if (F & B_PERIODIC) {
        for (int row = threadIdx.x >> 6; row < 4; row += nwb) {
            const int ws = a.per.wave_start[row];
            unsigned m = 0;
            double f = 0;
            if (ws != 0x7fffffff) {
                m = (unsigned) pre_slots[(size_t) ws * 64 + lane].y;
                if ((F & B_MTAB) && (F & B_SCALE)) f = a.slot_f[(size_t) ws * 64 + lane];
            }
            sh_pat_meta[row][lane] = m;
            sh_pat_f[row][lane] = f;
            if (F & B_CONS) {
                const bool member = ws != 0x7fffffff && (m & META_SHAKE);
                sh_pat_shake[row][lane] = member ? (unsigned) a.slot_shake[(size_t) ws * 64 + lane] : 0u;
                sh_pat_prm[row][lane] = member ? a.slot_shake_param[(size_t) ws * 64 + lane] : make_float4(0, 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // ---------------- thermostat wave: scale factors for the whole block, then done
    VV_SPAN_BEGIN;
    if (chain_wave) {
        // One-launch step: nothing waits for this wave before barrier 1, ~2 us away, while the tile waves' first batches queue on the CU's one
        // address path: it steps aside at the kernel's head -- its own loads go out behind theirs -- and takes the priority at the barrier.  Where the
        // tiles' front is long anyway (constraints, cos perturbation) that measured a loss (C4 83.3 -> 82.8 k, C3 + HBonds 79.6 -> 79.0 k steps/s
        // against C3 99.2 -> 100.2 k, C2 150.0 -> 151.4 k; profiles/r05p_thermostat_head_ab.txt) and the wave keeps its priority from the start.
        constexpr bool HEAD_ASIDE = FUSED && (FA & (A_CONS | A_COS | A_BIAS)) == 0;
        if constexpr (HEAD_ASIDE) {
            __builtin_amdgcn_s_sleep(THERMO_HEAD_SLEEP);
        } else {
            __builtin_amdgcn_s_setprio(3);        // the block waits for this wave: let it win the issue arbitration on its SIMD
        }
        VV_STAMP(7, 0);
        // Which lane advances which temperature group.  Two-launch kernel B (and the one-launch step next to the mailbox): lane g, group g; the totals arrive in scalar registers.  One-launch step otherwise (round 6): the fold leaves the total of row g in
        // lane 16 g + 15, and THAT lane runs group g's chain -- six v_readlane, the per-lane selects and the copies back into vector registers
        // (~20 instructions of one wave between "words held" and the release) are gone.  The other lanes of a row run the same instructions on the
        // row's partial sums and are ignored (no store, no vote in the chain's range test).
        // (With the cos moments the rows are grouped so that group g's three totals -- rows g, 4 + g, 7 + g -- meet in lane 16 g + 15 too; the bias
        // moment, row 3, is fetched from lane 63 for all of them.)
        constexpr bool LANE_LOCAL = FUSED && (SF & B_MAILBOX) == 0;
        const int cg = LANE_LOCAL ? ((lane >> 4) < VVHIP_NUM_TG ? (lane >> 4) : VVHIP_NUM_TG - 1) : (lane < VVHIP_NUM_TG ? lane : VVHIP_NUM_TG - 1);
        const bool group_lane = LANE_LOCAL ? ((lane & 15) == 15 && lane < 16 * VVHIP_NUM_TG) : lane < VVHIP_NUM_TG;
        constexpr int BIAS_LANE = LANE_LOCAL ? 63 : 3;
        constexpr int NCT = SF != 0 ? VV_SF_CHAIN_LINKS : 0;
        // what the wave's first batch of loads fills (load_batch) and what its tail produces (thermostat_tail)
        long long raw[NUM_ACC][ACC_SLOTS / 64] = {};
        unsigned int rv_seq = 0;       // fused step: rendezvous number (the tag of this step's words)
        unsigned int rv_delay = 0, rv_calm = 0, rv_late = 0;      // ... and the self-tuning wait in front of the first poll round (below)
        ChainRegs cr = {}, cr_loaded = {};
        ChainLaneBlock lc = {};
        double bias_carried = 0, ke2_prev = 0;
        unsigned int mb_seq = 0, mb_dead = 0;
        unsigned long long mb_peer_box = 0;
        ChainPrefix cpre = {1.0, 0.0};
        unsigned chain_max_hi = 0;
        ChainExpK ek = chain_exp_k();
        double ke2 = 0, bias = 0, factor = 1.0;
        // every load of this wave -- thermostat state, chain constants, the accumulator slots of all rows in use -- is issued here, in
        // front of a scheduling barrier: left to itself the backend sank part of the state loads BEHIND the first row's reduction
        // (register pressure), i.e. behind a wait for the cold accumulator loads, and the chain started a second memory round trip late
        // The chain's ke2-free prefix and the exp polynomial's coefficients in registers.  Two-launch kernel B: with the loads, in front of the fold.
        // One-launch step: BEHIND the publish, in the shadow of the wait for the other blocks' words -- in front of barrier 1 it made the thermostat
        // wave late at the barrier where the tiles' front is short (C2 -6 %, C1 -3 %, round 6), behind the poll it is ~70 instructions of the
        // kernel's serial path.  Pinned: left to itself the backend sinks this arithmetic to its first use, behind the poll (seen in the ISA).
        auto clear_idle_accumulators = [&]() {
            if (gridDim.x >= 64) {
                for (int sl = blockIdx.x; sl < ACC_SLOTS; sl += gridDim.x)
                    if (lane < a.acc_rows) a.acc_next[lane * ACC_SLOTS + sl] = 0;
            } else {
                for (int k = 0; k < a.acc_rows; k++)
                    for (int sl = blockIdx.x + lane * gridDim.x; sl < ACC_SLOTS; sl += 64 * gridDim.x) a.acc_next[k * ACC_SLOTS + sl] = 0;
            }
        };
        auto chain_head = [&]() {
            ek = chain_exp_k_pinned();
            if constexpr (NCT >= 1 && NCT <= 4) {
                cpre = chain_prefix<NCT>(lc, cr, chain_max_hi, ek);
                asm volatile("" :: "v"(cpre.expfac0), "v"(cpre.t0), "v"(cr.eta_dot[1]), "v"(cr.eta_dot[2]), "v"(cr.eta_dot[3]), "v"(chain_max_hi));
            }
        };
        auto load_batch = [&]() {
#pragma unroll
            for (int k = 0; k < NUM_ACC; k++) {
                const bool wanted = (k < 3 || (k == 3 && (F & B_UNBIAS)) || (k > 3 && (F & B_KE_MOM)));
#pragma unroll
                for (int j = 0; j < ACC_SLOTS / 64; j++) raw[k][j] = (wanted && !FUSED) ? (long long) pre_acc[k * ACC_SLOTS + lane + 64 * j] : 0ll;
            }
            rv_seq = pre_nh->rv_seq;
            rv_delay = pre_nh->rv_delay; rv_calm = pre_nh->rv_calm;
            if constexpr (FUSED) {          // how many blocks of the previous fused step needed a second poll round (every block reports in a word of its own)
                unsigned int lw[ACC_SLOTS / 64];
#pragma unroll
                for (int j = 0; j < ACC_SLOTS / 64; j++) lw[j] = __hip_atomic_load(&a.rv_late_prev[lane + 64 * j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                rv_late = 0;
#pragma unroll
                for (int j = 0; j < ACC_SLOTS / 64; j++) rv_late += (unsigned int) __popcll(__ballot(lane + 64 * j < (int) gridDim.x && lw[j] != 0u));
            }
#pragma unroll
            for (int i = 0; i < 4; i++) { cr.eta[i] = pre_nh->s.eta[cg][i]; cr.eta_dot[i] = pre_nh->s.eta_dot[cg][i]; cr.eta_dotdot[i] = pre_nh->s.eta_dotdot[cg][i]; }
            cr.eta_dot[4] = pre_nh->s.eta_dot[cg][4];
            lc = pre_lane_const[cg];
            bias_carried = pre_nh->scales[3];
            // multi-GPU: the exchange's sequence number and the "a wait ran out" word (uncached memory) come with the same batch -- requested
            // inside mailbox_exchange, i.e. behind the fold, they were two more dependent round trips on the kernel's critical path
            mb_seq = pre_nh->mb_seq;
            if (F & B_MAILBOX) { mb_dead = a.mb.ctl[0]; if (lane < a.mb.ranks) mb_peer_box = (unsigned long long) a.mb.peers[lane]; }
            // (what block 0 needs when it records the advanced state: requested here, not behind the chain at the very end of the kernel)
            ke2_prev = pre_nh->s.ke2[cg];
            __builtin_amdgcn_sched_barrier(0);
            // the chain's ke2-free prefix (chain_prefix), in front of the fold: its two exps and link updates run on the state that came with the
            // same batch of loads, and the scheduler is free to interleave them with the fold's lane exchanges
            cr_loaded = cr;
            if constexpr (!FUSED) chain_head();
        };
        auto thermostat_tail = [&]() {
        if constexpr (FUSED) {
            // ---- rendezvous.  The tile waves have laid their partial sums into sh_red (barrier 1); lane k adds quantity k over the block's
            // tile waves -- kernel A's tail, operation for operation -- and publishes it; then all blocks' words are collected.
            const bool en[NUM_ACC] = {true, true, true, (FA & A_BIAS) != 0, (FA & A_KE_MOM) != 0, (FA & A_KE_MOM) != 0, (FA & A_KE_MOM) != 0, (FA & A_KE_MOM) != 0, (FA & A_KE_MOM) != 0, (FA & A_KE_MOM) != 0};
            unsigned long long* rv = const_cast<unsigned long long*>(pre_acc);
            const unsigned long long tag = (unsigned long long) (1u + rv_seq % 62u) << 58;
            const int nblocks = (int) gridDim.x;
            // (what the publish needs from the kernel-argument block -- the quantity's fixed-point scale, the status pointer, the block count as a
            // double -- is fetched HERE, while the wave waits for the tiles anyway: behind the barrier those scalar loads were ~0.2 us of the
            // 0.37 us between barrier 1 and the publish, on the kernel's critical path; in-kernel stamps, round 5)
            const double my_scale = block_quantity_scale<NUM_ACC>(en, a.acc_scale, lane % NUM_ACC);
            const double block_limit = (double) (nblocks > 32 ? nblocks : 32);
            const int wait_units = a.fused_poll_delay >= 0 ? a.fused_poll_delay : (int) rv_delay;
            // (rows of tile waves this block does not have: zero, so that the sum behind barrier 1 needs no selects -- block_fixed_point_sum_padded)
            if (lane < NUM_ACC)
                for (int i = nwb - 1; i < 8; i++) sh_red[i][lane] = 0.0;
            // Lane k + NUM_ACC r publishes quantity k into replica r of the words (RV_REPLICAS copies, ONE store instruction); block b polls replica
            // b % RV_REPLICAS, so that every line is asked for by 1 / RV_REPLICAS of the blocks.  (The slot's address and the neutral word are formed here too.)
            const int my_q = lane % NUM_ACC, my_rep = lane / NUM_ACC;
            unsigned long long* const my_slot = rv + my_rep * RV_REPLICA_WORDS + rv_index(my_q, (int) blockIdx.x);
            const double* const my_partials = &sh_red[0][my_q];
            const unsigned long long word0 = rv_word(tag, 0);
            asm volatile("" :: "v"(my_scale), "s"(a.status), "v"(block_limit), "s"(wait_units), "v"(my_slot), "v"(my_partials), "s"(word0));
            __builtin_amdgcn_sched_barrier(0);
            VV_STAMP_NOWAIT(7, 6);
            __builtin_amdgcn_s_setprio(3);
            __syncthreads();
            VV_STAMP_NOWAIT(7, 7);
            if (my_rep < RV_REPLICAS && block_quantity_enabled<NUM_ACC>(en, my_q)) {
                // (a block may contribute 2^62 / blocks and must fit the 58-bit payload: 2^57 at most)
                const long long q = block_fixed_point_sum_padded<NUM_ACC>(sh_red, my_q, my_scale, a.status, block_limit);
                __hip_atomic_store(my_slot, word0 + (unsigned long long) q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                // the slots beyond the grid: the neutral word, from the first blocks (behind the block's own word; a grid of 251 blocks has five of them)
                for (int sl = nblocks + (int) blockIdx.x; sl < ACC_SLOTS; sl += nblocks)
                    __hip_atomic_store(my_slot + (sl - (int) blockIdx.x), word0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            VV_STAMP_NOWAIT(7, 8);      // "published"
            clear_idle_accumulators();
            chain_head();
            // ---- the poll: this wave collects every row in use itself, one batch of 4 loads per row per lane and round, and folds them below
            const unsigned long long* rvp = rv + ((int) blockIdx.x % RV_REPLICAS) * RV_REPLICA_WORDS;
            for (int d = 0; d < wait_units; d++) __builtin_amdgcn_s_sleep(4);
            unsigned long long word[NUM_ACC][ACC_SLOTS / 64];
            long long t0 = 0;
            int rounds = 0;
            const unsigned tag_lo = (unsigned) (tag >> 32), tag_hi = tag_lo | 0x03FFFFFFu;
            for (;;) {
                rounds++;
                // (Two rows of a slot side by side and ONE 16-byte load for both -- 8 / 20 loads per round instead of 12 / 40 -- was built and measured:
                // C3 90.4 k against 97.3 k steps/s, C4 58.7 k against 81.5 k, C5 108.1 against 114.7 k, two rotations on one box,
                // profiles/r05d_paired_vs_unpaired.txt.  16-byte accesses of the uncached allocation are the slower ones; 8-byte loads stay.)
#pragma unroll
                for (int k = 0; k < NUM_ACC; k++)
#pragma unroll
                    for (int j = 0; j < ACC_SLOTS / 64; j++) word[k][j] = en[k] ? __hip_atomic_load(&rvp[rv_index(k, lane + 64 * j)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : tag;
                // complete: every slot of every row in use carries this step's tag (rv_word) -- smallest and largest high word inside the tag's range
                // (every eighth round, with the round's batch -- a block that is merely late needs two or three: in EVERY round 251 blocks asking for this ONE word
                // cost the small and mid configurations 1-3 %, profiles/r06n_dead_word_ab.txt)
                const unsigned int dead = (rounds & 7) == 0 ? __hip_atomic_load(rv_dead_word(a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
                unsigned lo = 0xFFFFFFFFu, hi = 0u;
#pragma unroll
                for (int k = 0; k < NUM_ACC; k++) if (en[k]) rv_tag_range(word[k], lo, hi);
                if (!__any(lo < tag_lo || hi > tag_hi)) break;
                if (__any(dead != 0u)) break;
                if (t0 == 0) t0 = wall_clock64();
                if (wall_clock64() - t0 > 20000000LL) {                                  // 100 MHz counter
                    if (a.status) __hip_atomic_store(&a.status[2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(rv_dead_word(a), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            // (no decoding, no mask: the wrapping sum of a row's 256 raw words is the row's total, see rv_word)
#pragma unroll
            for (int k = 0; k < NUM_ACC; k++)
#pragma unroll
                for (int j = 0; j < ACC_SLOTS / 64; j++) raw[k][j] = en[k] ? (long long) word[k][j] : 0ll;
            // (this block's report to the wait's controller of the step after next: a word of its own -- 251 blocks flagging ONE word serialise
            // at the memory side for microseconds, first version of this.  HERE, not behind the release where nothing would wait for it: there it cost
            // the small configurations 4-5 % (C2 150 against 158 k steps/s, profiles/r06e_ek_late_ab.txt; unexplained))
            if (lane == 0) __hip_atomic_store(&a.rv_late_cur[blockIdx.x], rounds > 1 ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            VV_STAMP_AFTER(7, 9, raw[0][0]);
            VV_STAMP_VALUE(7, 10, rounds);
        }
        long long tot[NUM_ACC] = {};
        unsigned long long row_total_here = 0;      // LANE_LOCAL: the total of row (lane >> 4) in the row's last lane ...
        unsigned long long row_total_ab = 0, row_total_bb = 0;      // ... and, with the cos moments, of rows 4 + (lane >> 4) and 7 + (lane >> 4)
        // totals of the rows in use, four per wave reduction and the (up to three) groups of four step by step side by side, as kernel A's
        // tail does (wave_reduce4_groups): with the cos moments the fold is three rounds, and one after the other they kept this wave --
        // the block's critical path -- 0.3 us longer than C3's single round (in-kernel stamps, round 4).  Every total ends in a scalar register.
        constexpr int FG = (NUM_ACC + 3) / 4;
        static_assert(NUM_ACC == 10 && FG == 3, "the regrouping below is written for 4 + 3 + 3 rows");
        // which row sits in quarter i of group g: 4 g + i, or -- with the cos moments, so that the three rows of a temperature group share a lane --
        // {0, 1, 2, 3} | {4, 5, 6, -} | {7, 8, 9, -}
        const bool regroup = (F & B_KE_MOM) != 0;
        auto fold_row = [&](int g, int i) { return !regroup ? 4 * g + i : (g == 0 ? i : (i < 3 ? 3 * g + 1 + i : NUM_ACC)); };
        unsigned long long fa[FG], fb[FG], fc[FG], fd[FG], ft[FG];      // (unsigned: the one-launch step's words are summed modulo 2^64, rv_word)
        bool fon[FG];
#pragma unroll
        for (int g = 0; g < FG; g++) {
            unsigned long long part[4] = {0, 0, 0, 0};
            fon[g] = false;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int k = fold_row(g, i);
                const bool wanted = k < NUM_ACC && (k < 3 || (k == 3 && (F & B_UNBIAS)) || (k > 3 && (F & B_KE_MOM)));
                if (wanted) {
                    fon[g] = true;
#pragma unroll
                    for (int j = 0; j < ACC_SLOTS / 64; j++) part[i] += (unsigned long long) raw[k < NUM_ACC ? k : 0][j];
                }
            }
            fa[g] = part[0]; fb[g] = part[1]; fc[g] = part[2]; fd[g] = part[3]; ft[g] = 0;
        }
#pragma unroll
        for (int g = 0; g < FG; g++) if (fon[g]) { lane_swap32(fa[g], fc[g]); lane_swap32(fb[g], fd[g]); }
#pragma unroll
        for (int g = 0; g < FG; g++) if (fon[g]) { fa[g] += fc[g]; fb[g] += fd[g]; }
#pragma unroll
        for (int g = 0; g < FG; g++) if (fon[g]) lane_swap16(fa[g], fb[g]);
#pragma unroll
        for (int g = 0; g < FG; g++) if (fon[g]) ft[g] = fa[g] + fb[g];
#define VV_FOLD_STEP(CTRL) { unsigned long long f_[FG]; _Pragma("unroll") for (int g = 0; g < FG; g++) f_[g] = fon[g] ? dpp_fetch_u64<CTRL, 0xF>(ft[g]) : 0ull; _Pragma("unroll") for (int g = 0; g < FG; g++) if (fon[g]) ft[g] += f_[g]; }
        VV_FOLD_STEP(0x111) VV_FOLD_STEP(0x112) VV_FOLD_STEP(0x114) VV_FOLD_STEP(0x118)
#undef VV_FOLD_STEP
        row_total_here = ft[0]; row_total_ab = ft[1]; row_total_bb = ft[2];
#pragma unroll
        for (int k = 0; k < NUM_ACC; k++) {
            // (LANE_LOCAL: only the bias moment -- row 3, lane 63 of the first group -- is needed in every lane)
            if (LANE_LOCAL && k != 3) continue;
            const int g = !regroup ? k / 4 : (k < 4 ? 0 : (k < 7 ? 1 : 2)), i = !regroup ? k % 4 : (k < 4 ? k : (k < 7 ? k - 4 : k - 7));
            tot[k] = !fon[g] ? 0ll
                             : (long long) (((unsigned long long) (unsigned) __builtin_amdgcn_readlane((int) (ft[g] >> 32), 16 * i + 15) << 32) |
                                            (unsigned) __builtin_amdgcn_readlane((int) (unsigned) ft[g], 16 * i + 15));
        }
        if (F & B_MAILBOX) {                      // multi-GPU: block 0 publishes this rank's totals, every block collects all ranks'
            __shared__ unsigned int mb_words[MB_MAX_RANKS * MB_WORDS];
            __shared__ unsigned long long mb_peer_boxes[MB_MAX_RANKS];
            if (lane < a.mb.ranks) mb_peer_boxes[lane] = mb_peer_box;
            VV_WAVE_LDS_FENCE();
            mailbox_exchange(a, lane, mb_seq + 1u, mb_dead != 0, mb_peer_boxes, mb_words, tot);
        }
        VV_STAMP_AFTER(7, 1, row_total_here);      // "folded" (not VV_STAMP: that one waits for the wave's outstanding stores -- the "polled twice" word -- as well)
        ke2 = 0;
        if constexpr (LANE_LOCAL) {
            ke2 = (double) (long long) row_total_here * lc.acc_inv_scale;
        } else {
#pragma unroll
            for (int k = 0; k < VVHIP_NUM_TG; k++)
                if (cg == k) ke2 = (double) tot[k] * lc.acc_inv_scale;
        }
        if (F & B_KE_MOM) {                       // 2KE of the bias-free velocities from the moments of the biased ones
            const double V = (double) tot[3] * a.chain.acc_inv_scale[3] * a.chain.inv_mass_total;
            double sab = 0, sbb = 0;
            if constexpr (LANE_LOCAL) {
                sab = (double) (long long) row_total_ab * a.chain.acc_inv_scale[4]; sbb = (double) (long long) row_total_bb * a.chain.acc_inv_scale[7];
            } else {
#pragma unroll
                for (int k = 0; k < VVHIP_NUM_TG; k++)
                    if (cg == k) { sab = (double) tot[4 + k] * a.chain.acc_inv_scale[4]; sbb = (double) tot[7 + k] * a.chain.acc_inv_scale[7]; }
            }
            ke2 = ke2 - 2.0 * V * sab + V * V * sbb;
        }
        // the bias is requested before the chain starts (when it is carried over it is a load from the state)
        bias = (F & B_UNBIAS) ? (double) tot[3] * a.chain.acc_inv_scale[3] * a.chain.inv_mass_total   // K/cosineAccelerate.cu:57-59
                              : bias_carried;                                                    // carried over unchanged
        VV_STAMP_AFTER(7, 4, ke2);
        // Hands the scale factors to the block's tile waves the moment they are final -- in the MIDDLE of the chain update (see
        // propagate_preloaded): this wave's only barrier.  The second half of the chain runs while the tile waves scale and drift.
        auto release_tiles = [&](double f) {
            if (group_lane) sh_scales[cg] = f;
            if (lane == BIAS_LANE) sh_scales[3] = bias;
            VV_STAMP_AFTER(7, 5, f);
            __syncthreads();
        };
        factor = propagate_group_small<NCT>(a.chain, lc, ke2, cr, cr_loaded, cpre, chain_max_hi, !LANE_LOCAL || group_lane, ek, release_tiles);
        };
        // (One-launch step: a warm-up pass of the tail on zeros in the shadow of the tiles' loads -- the fold, 2KE and the chain up to the scale factor are
        // ~1.1 us of serial work behind the rendezvous where their arithmetic is ~0.3 us, and a cold instruction cache was the suspect --
        // was built and measured in round 5: the real pass was no faster (publish 0.28 / fold 0.26 / chain 0.49 us against 0.37 / 0.24 /
        // 0.54), and the wave reached barrier 1 0.3 us AFTER the tiles: C2 -11 %, C1 -5 %, C3 +-0.  Not the instruction cache; dropped.)
        load_batch();
        thermostat_tail();
        VV_STAMP_AFTER(7, 2, factor);
        // Every block clears ITS share of the idle accumulator copy (slots b, b + grid, ... of the rows in use): one store instruction
        // per thermostat wave.  Block 0 used to clear all of it -- 16 store instructions per lane, 40 with the cos moments -- behind its
        // chain, and was the last wave of the kernel by 0.4 us (C3) / 0.8 us (C4) (round 4, in-kernel stamps: "state stored" at 3.0 / 3.9 us
        // against 2.6 / 3.0 us for the tiles' last store).
        // (The fused step keeps this up although its own sums travel through the rendezvous words: a plan may alternate one-launch steps and
        // two-launch / split-entry-point steps -- a host that changes a parameter in the middle of a step, tests/test_cpp_plugin.py -- and the next
        // kernel A must find its copy clean whichever kind of step ran in between.)
        // (One-launch step, round 6: issued in the shadow of the rendezvous' wait instead -- a store issued at the end of the wave that ends last keeps
        // the whole kernel open for its trip to memory; the same goes for the "polled twice" word: behind the chain's second half it cost the small
        // configurations 2-5 %, profiles/r06e_ek_late_ab.txt.)
        if constexpr (!FUSED) clear_idle_accumulators();
        if (blockIdx.x == 0) {                    // one block records the advanced thermostat
            NHDevState* out = a.nh_next;
            if (group_lane) {
#pragma unroll
                for (int i = 0; i < 4; i++) { out->s.eta[cg][i] = cr.eta[i]; out->s.eta_dot[cg][i] = cr.eta_dot[i]; out->s.eta_dotdot[cg][i] = cr.eta_dotdot[i]; }
                out->s.eta_dot[cg][4] = cr.eta_dot[4];
                out->s.ke2[cg] = cg < a.chain.num_tg ? ke2 : ke2_prev;
                out->s.vscale[cg] = factor;
                out->scales[cg] = factor;
            }
            if (lane == 3) { out->s.v_bias = bias; out->scales[3] = bias; }
            if (lane == 4) out->mb_seq = mb_seq + ((F & B_MAILBOX) ? 1u : 0u);
            if (lane == 5) out->rv_seq = rv_seq + (FUSED ? 1u : 0u);
            if (lane == 6) {          // the wait's controller (fused step): one unit up behind a late block, one down after 256 quiet steps
                unsigned int nd = rv_delay, nc = rv_calm;
                if constexpr (FUSED) {
                    const unsigned int many = (gridDim.x >> (a.fused_late_shift & 31)) + 1u;
                    if (rv_late >= many) { nd = rv_delay < 16u ? rv_delay + 1u : rv_delay; nc = 0; }      // (capped: blocks that START unevenly are late whatever the wait)
                    else if (rv_late != 0) nc = 0;
                    else if (rv_calm >= 63u) { nd = rv_delay > 0u ? rv_delay - 1u : 0u; nc = 0; }
                    else nc = rv_calm + 1u;
                }
                out->rv_delay = nd; out->rv_calm = nc;
            }
        }
        VV_STAMP(7, 3);
        VV_STAMP_DUMP(7);
        VV_SPAN_END;
        return;
    }

    // ---------------- tile waves: grid-stride over 64-lane tiles.  The grid is capped (launch_b), so at large N every block
    // pays the fold + chain once and then streams many tiles; the first tile's loads overlap the thermostat wave.
    bool need_scales = true;
    VV_STAMP(wib, 0);
    // (fused step: ONE pass -- the launcher gives every tile a wave of its own, because the tile stays in registers across the rendezvous)
    for (int wave = blockIdx.x * tiles_per_block + wib; need_scales || (!FUSED && wave < pre_nwaves); wave += gridDim.x * tiles_per_block) {
        const bool valid = wave < pre_nwaves;
        int atom = -1;
        unsigned meta = 0;
        PeriodicWave pw = {0, 0, 0, 0};
        mixed4* velm = (mixed4*) a.velm;
        mixed4 v = {0, 0, 0, 0};
        int segb = 0;
        // table words that lead to a dependent load (image particle, Langevin random numbers): requested WITH the slot word -- their address needs
        // the wave index only --, so that what they point to travels with the tile's batch instead of one more round trip behind it
        int img_early = -1, rand_early = 0;
        if (F & B_PERIODIC) {
            if (valid) {          // (uniform) particle index from the wave index: the particle loads do not wait for a slot word
                pw = periodic_wave(a.per, wave);
                const bool in = lane < pw.count;
                atom = in ? pw.atom0 + lane : -1;
                meta = in ? sh_pat_meta[pw.region][lane] : 0u;
                segb = pw.seg0;
            }
        } else if (valid) {
            // (pre_seg_base: a preloaded argument; requested FIRST, it returns with the slot word)
            if (F & B_SCALE) segb = pre_seg_base[__builtin_amdgcn_readfirstlane(wave)];
            const int2 slot = pre_slots[(size_t) wave * 64 + lane];
            if (F & B_IMAGE) img_early = a.slot_image[(size_t) wave * 64 + lane];
            if constexpr (FUSED) { if (FA & A_LD) rand_early = a.slot_rand[(size_t) wave * 64 + lane]; }
            atom = slot.x; meta = (unsigned) slot.y;
        }
        const unsigned role = meta & META_ROLE_MASK;
        const int partner = (meta >> META_PARTNER_SHIFT) & 63;
        const bool act = atom >= 0;
        const mixed stepSize = (mixed) a.dt;
        // (fused step: kernel A's stages read the position too -- constraint directions, the charge for the field, z for the cos perturbation)
        const bool touches_pos = (F & (B_DRIFT_MIDDLE | B_POS3 | B_VV_POS | B_VV_KICK | B_HARDWALL | B_IMAGE | B_UNBIAS | B_BIAS_REMOVE | B_BIAS_RESTORE | B_VSITE)) ||
                                 (FUSED && (FA & (A_CONS | A_EF | A_COS | A_BIAS)) != 0);
        // ---- every load of the tile that needs nothing but the slot word (or nothing at all, with the arithmetic layout), in ONE
        // batch of unconditional loads from clamped indices closed by a scheduling barrier (see kernel A): velocity, position and
        // correction, force, the molecule's COM velocity, the pair's mass fraction, the constraint cluster words.  Six dependent
        // memory round trips per tile became two.
        const int ai = act ? atom : 0;
        const size_t li = valid ? (size_t) wave * 64 + lane : (size_t) lane;
        v = velm[ai];
        // One-launch step: a CU's seven tile waves put ~90 vector loads through ONE address / L1 path at the kernel's head (the youngest waves' data
        // arrives 0.25 us behind the oldest's, profiles/r05p_timeline_all_waves.txt), and barrier 1 waits for the youngest.  What the sums in front of
        // barrier 1 need goes first (velocity, force); positions -- a third of the bytes -- are requested BEHIND the kick where kernel A's stages do
        // not read them (no constraints, field, cos perturbation) and arrive during the rendezvous.
        constexpr bool POS_LATE = FUSED && (FA & (A_CONS | A_EF | A_COS | A_BIAS)) == 0;
        // ... and the pair's mass fraction, an operand of the scaling behind barrier 1, where that measured a gain: with the positions, and in the
        // constrained kernels (one box, three builds in rotation, profiles/r05p_late_loads_ab.txt: C3 97.4 -> 99.5 k steps/s, C2 145.4 -> 149.1 k,
        // C3 + HBonds 78.4 -> 79.8 k; the electrode slab and the cos perturbation lose 0.3-1 % with it and keep their single batch)
        constexpr bool TABF_LATE = POS_LATE || (FUSED && (FA & A_CONS) != 0 && (FA & (A_EF | A_COS | A_BIAS)) == 0);
        // (field / cos perturbation without constraints: kernel A's stages read posq alone -- the charge, z --, the correction follows behind the kick)
        constexpr bool CORR_LATE = FUSED && !POS_LATE && (FA & A_CONS) == 0;
        real4 p1 = {0, 0, 0, 0}, p2 = {0, 0, 0, 0};
        if (touches_pos && !POS_LATE) {
            p1 = ((const real4*) a.posq)[ai];
            if (IO::kMixed && !CORR_LATE) p2 = ((const real4*) a.corr)[ai];
        }
        long long kfx = 0, kfy = 0, kfz = 0;
        if ((F & B_KICK) || FA_KICK || VV1_EARLY) { kfx = a.force[ai]; kfy = a.force[ai + a.padded]; kfz = a.force[ai + 2 * a.padded]; }
        const unsigned long long leaders = (F & B_SCALE) ? __ballot((meta & META_COM_LEADER) != 0) : 0ull;     // in every lane: a wave-wide vote
        // COM velocity of this lane's molecule as kernel A's KE stage left it (of the bias-free velocities when a bias is
        // removed): one 32-byte entry per molecule, the same address for every lane of the segment (lanes behind the wave's last
        // leader read the tables' spare entry)
        mixed4 cv = {0, 0, 0, 0};
        double cw_raw = 0;
        double2 seg_mw = {0, 0};                 // fused step: (mass, 1 / mass) of this lane's COM segment, as kernel A reads it
        if (F & B_SCALE) {
            const int segi = segb + (int) lanes_below(leaders);
            if constexpr (FUSED) {
                seg_mw = ((const double2*) a.seg_mass)[segi];
            } else {
                cv = ((const mixed4*) a.comv)[segi];
                if (F & B_KE_MOM) cw_raw = a.comw[segi];
            }
        }
        // B_MTAB: the pair's mass fractions are static (vv_kernel_mass_table formed them with the operations of K/drudeNoseHoover.cu:173-180
        // on the same inverse masses, so they are the per-step values bit for bit): one 8-byte load per lane, requested with the
        // particle data, instead of two IEEE fp64 divisions per pair lane and step
        mixed tab_f = 0;
        if ((F & B_MTAB) && (F & B_SCALE) && !TABF_LATE) tab_f = (F & B_PERIODIC) ? (mixed) sh_pat_f[pw.region][lane] : (mixed) a.slot_f[li];      // (one-launch step: requested behind the kick, like the positions)
        // cluster word and parameters of the in-kernel constraints
        // (one-launch step: the hydrogen-type clusters' old bonds are formed ONCE per launch, by the velocity constraints of the front; vv_dev_constraints.inc: ClusterGeom)
        constexpr bool GEOM_SHARED = FUSED && (FA & A_SHAKE_V) != 0 && (FA & (A_GCONS | A_SHAKE_GS)) == 0 && (F & B_SHAKE) != 0 && (F & (B_GCONS | B_SHAKE_GS)) == 0;
        ClusterGeom<mixed> geom;      // (written and read by cluster members only)
        unsigned shake_word = 0;
        float4 shake_prm = make_float4(0, 0, 0, 0);
        if ((F & B_CONS) || (FUSED && (FA & A_CONS) != 0)) {
            shake_word = (F & B_PERIODIC) ? sh_pat_shake[pw.region][lane] : (unsigned) a.slot_shake[li];
            shake_prm = (F & B_PERIODIC) ? sh_pat_prm[pw.region][lane] : a.slot_shake_param[li];
        }
        // cos(2 pi z / Lz) of this lane, cached by kernel A (A_CZ_STORE)
        double cz_early = 0;
        if (F & B_CZ_LOAD) cz_early = a.cosz[li];
        int img = -1;
        if (F & B_IMAGE) img = (F & B_PERIODIC) ? a.slot_image[li] : img_early;
        int2 vsite = {0, 0};
        if (F & B_VSITE) vsite = a.slot_vsite[li];
        // fused step: what kernel A's extra-force stages read
        real3 fe_a = {0, 0, 0};
        int rand_slot = 0;
        if constexpr (FUSED) {
            if ((FA & A_FE_LOAD) || VV1_EARLY) fe_a = ((const real3*) a.fextra)[ai];
            if (FA & A_LD) rand_slot = rand_early;
        }
        __builtin_amdgcn_sched_barrier(0);
        float4 rnd_a = make_float4(0, 0, 0, 0), rnd_b = make_float4(0, 0, 0, 0);
        if constexpr (FUSED && (FA & A_LD) != 0) {      // Langevin lanes: the normal deviates behind their slot (keyed by the role word), as in kernel A
            if (act && (role == ROLE_LD_NORMAL || role == ROLE_LD_DRUDE || role == ROLE_LD_PARENT)) {
                const unsigned ri = a.random_index + (unsigned) rand_slot;
                rnd_a = a.random[ri];
                if (role != ROLE_LD_NORMAL) rnd_b = a.random[ri + 1];
            }
        }
        // image particle of this lane's particle: its present content (the charge and the correction's w survive the mirror update)
        // is requested now -- in the tile's batch: its index came with the slot word --, so that nothing has to be read after the position store at the
        // end of the tile
        real4 img_p = {0, 0, 0, 0}, img_c = {0, 0, 0, 0};
        if (!((F & B_IMAGE) && act && (meta & META_HAS_IMAGE))) img = -1;
        if ((F & B_IMAGE) && img >= 0) {
            img_p = ((const real4*) a.posq)[img];
            if (IO::kMixed) img_c = ((const real4*) a.corr)[img];
        }
        if (!act) { v = mixed4{0, 0, 0, 0}; fe_a = real3{0, 0, 0}; }
        if (!((F & B_GCONS) || (FUSED && (FA & A_GCONS) != 0)) && !(act && (meta & META_SHAKE))) shake_word = 0;      // (a general cluster's word is a constraint of the wave's list)
        if (!valid) shake_word = 0;      // (a tile wave without a tile only passes through for the block's barriers: no list, no sweeps)
        const bool massive = act && v.w != 0;
        mixed x = 0, y = 0, z = 0, q = 0;
        real zraw = 0;
        auto form_position = [&]() {
            if (act && touches_pos) {          // K/middle.cu:81-96: positions are posq (+ posqCorrection in mixed mode)
                zraw = p1.z;
                if (IO::kMixed) { x = p1.x + (mixed) p2.x; y = p1.y + (mixed) p2.y; z = p1.z + (mixed) p2.z; q = p1.w; }
                else { x = p1.x; y = p1.y; z = p1.z; q = p1.w; }
            }
        };
        if (!POS_LATE && !CORR_LATE) form_position();
        // B_KICK: kernel A kept its kicked velocities in registers (A_NOSTORE); the same kick again here, from the same velm and force
        // bits with the same expression (K/middle.cu:11-21; forceExtra is zero on this path), gives the same velocities bit for bit.
        // (a massless particle's force is read and not used)
        if ((F & B_KICK) && act) {
            const long long fx = kfx, fy = kfy, fz = kfz;
            real3 fe = {0, 0, 0};
            if (F & B_UNBIAS) fe.x += (real) a.cos_accel * cz_early * P::RECIP(v.w);      // K/cosineAccelerate.cu:9, kernel A's A_COS term to the bit
            const mixed fscale = stepSize / (mixed) 0x100000000;
            if (v.w != 0) {          // K/middle.cu:11: massive particles only
                v.x += stepSize * v.w * fe.x + fscale * v.w * fx;
                v.y += stepSize * v.w * fe.y + fscale * v.w * fy;
                v.z += stepSize * v.w * fe.z + fscale * v.w * fz;
            }
        }
        const bool nh = role == ROLE_NH_NORMAL || role == ROLE_NH_DRUDE || role == ROLE_NH_PARENT;
        const bool use_com = ((meta >> META_SEGFIRST_SHIFT) & 63) != ((meta >> META_SEGLAST_SHIFT) & 63) || (meta & META_COM_LEADER);
        // per-wave LDS page of the in-kernel constraint solvers (collective over the wave: every lane walks through it)
        extern __shared__ double vv_dyn_lds[];
        mixed* shake_page_b = (mixed*) vv_dyn_lds + wib * (7 * 64);      // one page per tile wave, sized at launch
        double czl = 0;                  // fused step: cos(2 pi z / Lz) of this lane, evaluated once
        if constexpr (FUSED) {
            // ================= kernel A's stage set on this tile: each stage the expression of vv_kernel_a, on the same operands =================
            if (FA & (A_COS | A_BIAS)) {
                czl = cos_kz<real>(p1.z, (real) a.inv_box_z);
                if ((FA & A_CZ_STORE) && valid) a.cosz[li] = czl;          // (kept for vvhip_set_params: the stale forceExtra of a switched-off perturbation)
            }
            real3 fe = (FA & A_FE_LOAD) ? fe_a : real3{0, 0, 0};             // extra force (VVIntegrator.cpp:238-245), accumulated in `real` like forceExtra
            if (FA & A_LD) langevin_force<real, mixed>(a, role, massive, partner, v, false, (mixed) 0, rnd_a, rnd_b, fe);
            if ((FA & A_EF) && act && (meta & META_EFIELD))                      // K/electricField.cu:8-10
                fe.z += (real) a.efscale * p1.w;
            if ((FA & A_COS) && massive)                                         // K/cosineAccelerate.cu:9
                fe.x += (real) a.cos_accel * czl * P::RECIP(v.w);
            if ((FA & A_FE_STORE) && act) ((real3*) a.fextra)[atom] = fe;          // the first half of the NEXT classic step kicks with these (API:316-323)
            VV_STAMP(wib, 6);
            if ((FA & A_KICK_FULL) && massive) {                                 // K/middle.cu:11-21
                const mixed fscale = stepSize / (mixed) 0x100000000;
                v.x += stepSize * v.w * fe.x + fscale * v.w * kfx;
                v.y += stepSize * v.w * fe.y + fscale * v.w * kfy;
                v.z += stepSize * v.w * fe.z + fscale * v.w * kfz;
            }
            if ((FA & A_KICK_HALF) && massive) {                                 // K/velocityVerlet.cu:20-22 (0.5 is a double literal)
                const mixed fscale = (mixed) a.fscale_vv;
                v.x += 0.5 * stepSize * v.w * fe.x + fscale * v.w * kfx;
                v.y += 0.5 * stepSize * v.w * fe.y + fscale * v.w * kfy;
                v.z += 0.5 * stepSize * v.w * fe.z + fscale * v.w * kfz;
            }
            if (POS_LATE && touches_pos) {          // (see POS_LATE: in flight while the sums are formed, used behind barrier 1)
                p1 = ((const real4*) a.posq)[ai];
                if (IO::kMixed) p2 = ((const real4*) a.corr)[ai];
            }
            if (CORR_LATE && IO::kMixed && touches_pos) p2 = ((const real4*) a.corr)[ai];
            if (TABF_LATE && (F & B_MTAB) && (F & B_SCALE)) tab_f = (mixed) a.slot_f[li];
            if (FA & A_CONS) {                      // integration.applyVelocityConstraints(tol) (HOST:151), clusters solved in the wave
                mixed sx, sy, sz;
                if (IO::kMixed) { sx = p1.x + (mixed) p2.x; sy = p1.y + (mixed) p2.y; sz = p1.z + (mixed) p2.z; }
                else { sx = p1.x; sy = p1.y; sz = p1.z; }
                if (FA & A_GCONS)
                    general_velocities<mixed>(lane, shake_word, shake_prm, (mixed) a.shake_tol, (mixed) a.gc_omega, a.gc_colors, act && (meta & META_SHAKE), sx, sy, sz, v.x, v.y, v.z, shake_page_b, a.status);
                else
                    shake_velocities<mixed, GEOM_SHARED>(lane, shake_word, shake_prm, (mixed) a.shake_tol, sx, sy, sz, v.w, v.x, v.y, v.z, shake_page_b,
                                                         (FA & A_SHAKE_V) != 0, (FA & A_SETTLE) != 0, false, &geom);
            }
            double k_atom = 0, k_com = 0, k_drude = 0, k_bias = 0, m_ab[3] = {0, 0, 0}, m_bb[3] = {0, 0, 0};
            if ((FA & A_BIAS) && massive) {                                      // K/cosineAccelerate.cu:24-27
                const mixed t = P::RECIP(v.w) * v.x * 2 * czl;
                k_bias += (double) t;
            }
            // ---- kinetic energies of the thermostat groups in Koenig form (vv_kernel_a's A_KE stage; K/drudeNoseHoover.cu:33-151); the COM
            // velocity the segment's leader lane forms goes to the segment's lanes over the shuffle network instead of through `comv`
            mixed lVx = 0, lVy = 0, lVz = 0, lVw = 0, lWx = 0;
            {
                const bool fuse_ke = !(FA & A_CONS);
                auto dot_ke = [&](mixed a0, mixed a1, mixed a2, mixed b0, mixed b1, mixed b2) -> mixed {
                    return fuse_ke ? vfma(a2, b2, vfma(a1, b1, a0 * b0)) : a0 * b0 + a1 * b1 + a2 * b2;
                };
                const mixed kux = v.x;
                const int first = (meta >> META_SEGFIRST_SHIFT) & 63, last = (meta >> META_SEGLAST_SHIFT) & 63;
                const bool leader = use_com && (meta & META_COM_LEADER);       // the last lane of its segment
                const bool contrib = nh && massive;
                const mixed own_mass = massive ? P::RECIP_SUM(v.w) : (mixed) 0;
                const mixed wx = ((FA & A_KE_MOM) && act) ? (mixed) czl : (mixed) 0;      // the field of the cos perturbation, (cos kz, 0, 0)
                mixed px = 0, py = 0, pz = 0, pw = 0;
                if (contrib) {
                    px = kux * own_mass; py = v.y * own_mass; pz = v.z * own_mass;
                    k_atom += (double) dot_ke(px, py, pz, kux, v.y, v.z);
                    if (FA & A_KE_MOM) { pw = wx * own_mass; m_ab[0] += (double) (px * wx); m_bb[0] += (double) (pw * wx); }
                }
                if (__any(role == ROLE_NH_DRUDE)) {
                    const mixed ox = shfl(kux, partner), oy = shfl(v.y, partner), oz = shfl(v.z, partner);
                    const mixed om = shfl(own_mass, partner);
                    const mixed ow = (FA & A_KE_MOM) ? shfl(wx, partner) : (mixed) 0;
                    if (role == ROLE_NH_DRUDE) {
                        const mixed reducedMass = own_mass * om * P::RECIP_SUM(own_mass + om);
                        const mixed qx = ox - kux, qy = oy - v.y, qz = oz - v.z;
                        k_drude += (double) (dot_ke(qx, qy, qz, qx, qy, qz) * reducedMass);
                        if (FA & A_KE_MOM) { const mixed rb = ow - wx; m_ab[2] += (double) (qx * rb * reducedMass); m_bb[2] += (double) (rb * rb * reducedMass); }
                    }
                }
                if (__any(use_com)) {
                    const bool in_seg = contrib && use_com;
                    mixed Sx = in_seg ? px : (mixed) 0, Sy = in_seg ? py : (mixed) 0, Sz = in_seg ? pz : (mixed) 0;
                    wave_scan3(Sx, Sy, Sz);
                    const int prev = first > 0 ? first - 1 : 0;
                    mixed Tx = Sx - shfl(Sx, prev), Ty = Sy - shfl(Sy, prev), Tz = Sz - shfl(Sz, prev);
                    if (first == 0) { Tx = Sx; Ty = Sy; Tz = Sz; }
                    mixed Tw = 0;
                    if (FA & A_KE_MOM) {      // the shuffle must run in ALL lanes: a lane reads its left neighbour segment's last lane
                        const mixed Sw = wave_scan(in_seg ? pw : (mixed) 0);
                        const mixed Lw = shfl(Sw, prev);
                        Tw = first > 0 ? Sw - Lw : Sw;
                    }
                    if (leader && act) {
                        const mixed Vm = (mixed) seg_mw.x;
                        lVw = (mixed) seg_mw.y;      // static: summed once on the host in particle order (vv_host.hpp: seg_mass)
                        lVx = Tx * lVw; lVy = Ty * lVw; lVz = Tz * lVw;                  // V = P * RECIP(M), comVelm.w = RECIP(M)
                        if (lVw != 0) k_com += (double) (dot_ke(lVx, lVy, lVz, lVx, lVy, lVz) * Vm);
                        if (FA & A_KE_MOM) {
                            lWx = Tw * lVw;                                              // mass-weighted mean of cos(kz) over the molecule
                            if (lVw != 0) { m_ab[1] += (double) (lVx * lWx * Vm); m_bb[1] += (double) (lWx * lWx * Vm); }
                        }
                    }
                    // what kernel B would read back from comv / comw: the leader's values, for every lane of its segment
                    lVx = shfl(lVx, last); lVy = shfl(lVy, last); lVz = shfl(lVz, last);
                    if (FA & A_KE_MOM) lWx = shfl(lWx, last);
                }
            }
            const double vals[NUM_ACC] = {k_atom - k_drude - k_com, k_com, k_drude, k_bias, m_ab[0] - m_ab[2] - m_ab[1], m_ab[1], m_ab[2],
                                          m_bb[0] - m_bb[2] - m_bb[1], m_bb[1], m_bb[2]};
            const bool mom = (FA & A_KE_MOM) != 0;
            const bool en[NUM_ACC] = {true, true, true, (FA & A_BIAS) != 0, mom, mom, mom, mom, mom, mom};
            VV_STAMP_AFTER(wib, 7, vals[0]);
            wave_partials_to_lds<NUM_ACC>(vals, en, sh_red, wib, lane);
            VV_STAMP_NOWAIT(wib, 8);
            __syncthreads();             // barrier 1: the block's thermostat wave publishes the block's sums
            VV_STAMP_NOWAIT(wib, 9);
            cv.x = lVx; cv.y = lVy; cv.z = lVz; cv.w = lVw;
            cw_raw = (double) lWx;
            if (POS_LATE || CORR_LATE) form_position();
        }
        const mixed4 v_old = v;          // velocity after the kick, before the thermostat (Pos1 uses it)
        bool vel_dirty = (F & B_KICK) != 0 || FA_KICK || (FUSED && (FA & A_CONS) != 0), pos_dirty = false;

        mixed Vx = 0, Vy = 0, Vz = 0, Vw = 0, com_w = 0;
        if ((F & B_SCALE) && nh && use_com) {
            Vx = cv.x; Vy = cv.y; Vz = cv.z; Vw = cv.w;
            if (F & B_KE_MOM) com_w = (mixed) cw_raw;
        }

        // Factor-independent half of the scaling: velocities relative to the molecular COM, the Drude partner's over the shuffle
        // network, mass fractions, COM / relative split of the pair.  Without a bias to remove first it runs here, i.e. while
        // the tile waves of the first iteration wait for the thermostat wave.
        // The pair arithmetic is written in terms of "own" and "partner", not "atom 1 (Drude)" and "atom 2 (parent)": the reference's
        //     cm = a1 * mass1fract + a2 * mass2fract,  r = a2 - a1,  v1 = s - t * mass2fract + ...,  v2 = s + t * mass1fract + ...   (t = vscaleDrude * r)
        // are, for either lane, cm = own * f_own + partner * f_partner (the sum of the same two products: IEEE addition commutes) and
        // v = s - (vscaleDrude * (partner - own)) * f_partner + ... (the parent's r is -(partner - own), and a sign passes through a product and
        // turns the addition into the subtraction exactly) -- the same bits without the sixteen 64-bit selects per lane that sorting the operands
        // into 1 and 2 costs in a kernel bound by its instruction count.
        mixed ux = 0, uy = 0, uz = 0, cmx = 0, cmy = 0, cmz = 0, rx = 0, ry = 0, rz = 0, par_f = 0;
        if (!(act && (role == ROLE_NH_DRUDE || role == ROLE_NH_PARENT))) tab_f = 0;
        // (With the cos perturbation the bias V is only known at the release, so this half runs behind it.  Preparing it before -- every
        // quantity is linear in the velocities, u(V) = u_a - V u_b with u_b from the field (cos kz, 0, 0) through the same map, three fused
        // multiply-adds per lane left behind the release -- was built and measured in round 4: C4 74.3 k against 74.9 k steps/s with the
        // force provider, 91.2 k against 90.5 k without, three rotations on one box (profiles/r04b_ab_C4_cos_variants.txt): not kept.)
        auto scale_prep = [&]() {
            ux = v.x; uy = v.y; uz = v.z;
            if (nh) { ux -= Vx; uy -= Vy; uz -= Vz; }
            // each lane forms the reciprocal of its own inverse mass, the partner's arrives by shuffle: the same IEEE quotients as
            // RECIP(a1w), RECIP(a2w) of K/drudeNoseHoover.cu:173-174 with one division per lane instead of two
            const bool pair_lane = role == ROLE_NH_DRUDE || role == ROLE_NH_PARENT;
            const mixed own_m = (F & B_MTAB) ? tab_f : (pair_lane ? P::RECIP(v.w) : (mixed) 0);     // with the table: the own FRACTION travels
            const mixed px = shfl(ux, partner), py = shfl(uy, partner), pz = shfl(uz, partner), pm = shfl(own_m, partner);
            if (pair_lane) {
                mixed own_f;
                if (F & B_MTAB) {
                    own_f = own_m; par_f = pm;
                } else {
                    const mixed invTotalMass = P::RECIP(own_m + pm);      // mass1 + mass2 in either order
                    own_f = invTotalMass * own_m; par_f = invTotalMass * pm;
                }
                cmx = ux * own_f + px * par_f;
                cmy = uy * own_f + py * par_f;
                cmz = uz * own_f + pz * par_f;
                rx = px - ux; ry = py - uy; rz = pz - uz;      // Drude lane: r; parent lane: -r
            }
        };
        const bool prep_early = (F & B_SCALE) && !(F & (B_UNBIAS | B_BIAS_REMOVE));
        VV_STAMP(wib, 1);
        if (prep_early) scale_prep();
        // (rigid triangles: what their position solve needs from the OLD positions alone -- vv_dev_constraints.inc: settle_prepare -- while the wave waits anyway)
        constexpr bool SETTLE_PREP = FUSED && (FA & A_CONS) != 0 && (F & B_SETTLE) != 0 && (F & (B_SHAKE_GS | B_GCONS)) == 0;
        SettleFrame<mixed> sframe;
        if constexpr (SETTLE_PREP) settle_prepare<mixed>(lane, shake_word, shake_prm, x, y, z, v.w, shake_page_b, sframe);
        VV_STAMP(wib, 2);

        if (need_scales) {
            need_scales = false;
            if (has_cw) {
                __syncthreads();
                sc0 = sh_scales[0]; sc1 = sh_scales[1]; sc2 = sh_scales[2]; scb = sh_scales[3];
                VV_STAMP(wib, 3);
            } else if (F & (B_SCALE | B_UNBIAS | B_BIAS_REMOVE | B_BIAS_RESTORE)) {
                sc0 = a.nh->scales[0]; sc1 = a.nh->scales[1]; sc2 = a.nh->scales[2]; scb = a.nh->scales[3];
            }
            if (!valid) break;
        }

        // ---------------- bias removal (K/cosineAccelerate.cu:63-73); cos uses posq.z (real), all particles
        double cz = 0;
        mixed Vb = 0;
        if (F & (B_UNBIAS | B_BIAS_REMOVE | B_BIAS_RESTORE)) {
            Vb = (mixed) scb;
            cz = FUSED ? czl : ((F & B_CZ_LOAD) ? cz_early : cos_kz<real>(zraw, (real) a.inv_box_z));
            if ((F & (B_UNBIAS | B_BIAS_REMOVE)) && act) { v.x -= Vb * cz; vel_dirty = true; }
            if (F & B_KE_MOM) Vx -= Vb * com_w;       // kernel A stored the COM velocity of the biased velocities: COM(u) = COM(v) - V COM(w)
        }

        // ---------------- NH velocity scaling (K/drudeNoseHoover.cu:157-209): the factor-independent half was prepared above
        if (F & B_SCALE) {
            if (!prep_early) scale_prep();
            const mixed vscaleAtom = (mixed) sc0, vscaleCOM = (mixed) sc1, vscaleDrude = (mixed) sc2;
            // (One expression for both kinds of lane -- a particle outside a pair as its own pair centre with r = 0 -- is the same bits
            // and nine instructions less behind the thermostat wave's release; it measured no faster.)
            if (role == ROLE_NH_NORMAL) {
                if (massive) {
                    v.x = vscaleAtom * ux + vscaleCOM * Vx;
                    v.y = vscaleAtom * uy + vscaleCOM * Vy;
                    v.z = vscaleAtom * uz + vscaleCOM * Vz;
                    vel_dirty = true;
                }
            } else if (role == ROLE_NH_DRUDE || role == ROLE_NH_PARENT) {
                const mixed sx = vscaleAtom * cmx, sy = vscaleAtom * cmy, sz = vscaleAtom * cmz;
                const mixed tx = vscaleDrude * rx, ty = vscaleDrude * ry, tz = vscaleDrude * rz;
                v.x = sx - tx * par_f + vscaleCOM * Vx;
                v.y = sy - ty * par_f + vscaleCOM * Vy;
                v.z = sz - tz * par_f + vscaleCOM * Vz;
                vel_dirty = true;
            }
        }
        if ((F & (B_UNBIAS | B_BIAS_RESTORE)) && act) { v.x += Vb * cz; vel_dirty = true; }   // K/cosineAccelerate.cu:76-85

        // ---------------- classic VV first half: kick from the stored extra force, then posDelta (K/velocityVerlet.cu:6-29)
        mixed dx = 0, dy = 0, dz = 0;
        if ((F & B_VV_KICK) && massive) {
            real3 fe;
            long long fx, fy, fz;
            if constexpr (VV1_EARLY) { fe = fe_a; fx = kfx; fy = kfy; fz = kfz; }
            else { fe = ((const real3*) a.fextra)[atom]; fx = a.force[atom]; fy = a.force[atom + a.padded]; fz = a.force[atom + 2 * a.padded]; }
            const mixed fscale = (mixed) a.fscale_vv;
            v.x += 0.5 * stepSize * v.w * fe.x + fscale * v.w * fx;
            v.y += 0.5 * stepSize * v.w * fe.y + fscale * v.w * fy;
            v.z += 0.5 * stepSize * v.w * fe.z + fscale * v.w * fz;
            dx = stepSize * v.x; dy = stepSize * v.y; dz = stepSize * v.z;
            vel_dirty = true;
        }
        // ---------------- position updates
        if ((F & B_POS2) && massive) {                                          // K/middle.cu:51-58
            const mixed halfdt = 0.5f * stepSize;
            mixed4 d = {halfdt * v.x, halfdt * v.y, halfdt * v.z, 0};
            mixed4 pd = ((mixed4*) a.pos_delta)[atom], od = ((mixed4*) a.old_delta)[atom];
            pd.x += d.x; pd.y += d.y; pd.z += d.z; pd.w += d.w;
            od.x += d.x; od.y += d.y; od.z += d.z; od.w += d.w;
            ((mixed4*) a.pos_delta)[atom] = pd;
            ((mixed4*) a.old_delta)[atom] = od;
        }
        if (F & B_DRIFT_MIDDLE) {
            // Pos1 (K/middle.cu:36-38) with the pre-thermostat velocity, Pos2 (:54-56) with the scaled one.  Without constraints
            // posDelta == oldDelta and Pos3's velocity correction (K/middle.cu:77-79) adds (d - d)/dt == 0 exactly; with the
            // in-kernel SHAKE the constrained displacement differs and the correction is the constraint force's kick.
            const mixed halfdt = 0.5f * stepSize;
            mixed ddx = 0, ddy = 0, ddz = 0;
            if (massive) {
                ddx = halfdt * v_old.x; ddy = halfdt * v_old.y; ddz = halfdt * v_old.z;
                ddx += halfdt * v.x; ddy += halfdt * v.y; ddz += halfdt * v.z;
            }
            const mixed odx = ddx, ody = ddy, odz = ddz;
            if (F & B_GCONS)                                                       // integration.applyConstraints(tol), HOST:176
                general_positions<mixed>(lane, shake_word, shake_prm, (mixed) a.shake_tol, (mixed) a.gc_omega, a.gc_colors, act && (meta & META_SHAKE), x, y, z, ddx, ddy, ddz, shake_page_b, a.status);
            else if (F & B_CONS)
                shake_positions<mixed, GEOM_SHARED, SETTLE_PREP>(lane, shake_word, shake_prm, (mixed) a.shake_tol, x, y, z, v.w, ddx, ddy, ddz, shake_page_b,
                                                                 (F & B_SHAKE) != 0, (F & B_SETTLE) != 0, (F & B_SHAKE_GS) != 0, a.status, &geom, &sframe);
            if (massive) {
                const mixed invDt = (mixed) a.inv_dt_mixed;      // = 1 / stepSize, formed once on the host
                v.x += (ddx - odx) * invDt; v.y += (ddy - ody) * invDt; v.z += (ddz - odz) * invDt;
                x += ddx; y += ddy; z += ddz;
                pos_dirty = true; vel_dirty = true;
            }
            // (one-launch step without constraints: the velocity is final here unless the hard wall is hit -- its 32 bytes per lane leave now, in front of the wall's
            // and the position's arithmetic, instead of in one burst with the position's at the wave's end; a lane the wall does hit stores again below)
            if constexpr (FUSED && (F & B_CONS) == 0) {
                if (act && vel_dirty) store_vec(velm, atom, v);
                vel_dirty = false;
            }
        }
        if ((F & B_POS3) && massive) {                                          // K/middle.cu:70-96
            const mixed invDt = (mixed) a.inv_dt_mixed;      // = 1 / stepSize, formed once on the host
            const mixed4 d = ((const mixed4*) a.pos_delta)[atom], od = ((const mixed4*) a.old_delta)[atom];
            v.x += (d.x - od.x) * invDt; v.y += (d.y - od.y) * invDt; v.z += (d.z - od.z) * invDt;
            x += d.x; y += d.y; z += d.z;
            pos_dirty = true; vel_dirty = true;
        }
        if (F & (B_VV_POS | B_VV_KICK)) {                                       // K/velocityVerlet.cu:41-66
            if (!(F & B_VV_KICK) && massive) {
                const mixed4 d = ((const mixed4*) a.pos_delta)[atom];
                dx = d.x; dy = d.y; dz = d.z;
            }
            if (F & B_GCONS)                                                       // integration.applyConstraints(tol), HOST:351
                general_positions<mixed>(lane, shake_word, shake_prm, (mixed) a.shake_tol, (mixed) a.gc_omega, a.gc_colors, act && (meta & META_SHAKE), x, y, z, dx, dy, dz, shake_page_b, a.status);
            else if (F & B_CONS)
                shake_positions<mixed, GEOM_SHARED, SETTLE_PREP>(lane, shake_word, shake_prm, (mixed) a.shake_tol, x, y, z, v.w, dx, dy, dz, shake_page_b,
                                                                 (F & B_SHAKE) != 0, (F & B_SETTLE) != 0, (F & B_SHAKE_GS) != 0, a.status, &geom, &sframe);
            if (massive) {
                const mixed invStepSize = (mixed) a.inv_dt_double; // = 1.0 / stepSize, formed once on the host
                x += dx; y += dy; z += dz;
                v.x = (mixed) (invStepSize * dx); v.y = (mixed) (invStepSize * dy); v.z = (mixed) (invStepSize * dz);
                pos_dirty = true; vel_dirty = true;
            }
        }

        // ---------------- hard wall on Drude pairs (K/middle.cu:106-221); pair.x = Drude = "1", parent = "2"
        if (F & B_HARDWALL) {
            const mixed ox = shfl(x, partner), oy = shfl(y, partner), oz = shfl(z, partner);
            if (act && (meta & META_PAIR)) {
                const bool isd = (meta & META_IS_DRUDE) != 0;
                const mixed maxDrudeDistance = (mixed) a.max_drude, hardwallscaleDrude = (mixed) a.hw_scale;
                // delta = pos1 - pos2 is own - partner in the Drude lane and its exact negative in the parent lane: r2, a sum of squares, is the
                // same bits either way, so the fall-through path sorts nothing into "1" and "2" (the hit path below does)
                const mixed ownx = x - ox, owny = y - oy, ownz = z - oz;
                const mixed r2 = ownx * ownx + owny * owny + ownz * ownz;
                // The reference decides on rInv * maxDrudeDistance < 1 with r = SQRT(r2), rInv = RECIP(r) (K/middle.cu:126-131): a square
                // root and an IEEE division per pair and step.  r2 <= (0.9999 max)^2 implies r <= 0.99999 max (SQRT is a float sqrt in
                // mixed mode: relative error 1.2e-7), which implies rInv * max >= 1.00001 (1 - 2^-23)^2 > 1 in every mode, i.e. "no hit"
                // without forming either; only pairs within 1e-4 of the wall or beyond it take the exact test.  Same decisions, same bits.
                mixed r = 0, rInv = 0;
                bool hit = false;
                const mixed nearWall = maxDrudeDistance * (mixed) 0.9999;
                if (__builtin_expect(r2 > nearWall * nearWall, 0)) {
                    r = P::SQRT(r2);
                    rInv = P::RECIP(r);
                    hit = rInv * maxDrudeDistance < 1;
                }
                if (__builtin_expect(hit, 0)) {      // rare: keep the hit path out of the fall-through code
                    // both lanes of a pair see the same r, so both are in here: the partner's velocity is fetched only now
                    const mixed ovx = shfl(v.x, partner), ovy = shfl(v.y, partner), ovz = shfl(v.z, partner), ovw = shfl(v.w, partner);
                    mixed p1x = isd ? x : ox, p1y = isd ? y : oy, p1z = isd ? z : oz;
                    mixed p2x = isd ? ox : x, p2y = isd ? oy : y, p2z = isd ? oz : z;
                    const mixed vel1w = isd ? v.w : ovw, vel2w = isd ? ovw : v.w;
                    const mixed deltax = p1x - p2x, deltay = p1y - p2y, deltaz = p1z - p2z;
                    mixed vel1x = isd ? v.x : ovx, vel1y = isd ? v.y : ovy, vel1z = isd ? v.z : ovz;
                    mixed vel2x = isd ? ovx : v.x, vel2y = isd ? ovy : v.y, vel2z = isd ? ovz : v.z;
                    const mixed bx = deltax * rInv, by = deltay * rInv, bz = deltaz * rInv;
                    const mixed mass1 = P::RECIP(vel1w), mass2 = P::RECIP(vel2w);
                    const mixed deltaR = r - maxDrudeDistance;
                    mixed deltaT = stepSize;
                    mixed dotvr1 = vel1x * bx + vel1y * by + vel1z * bz;
                    const mixed vb1x = bx * dotvr1, vb1y = by * dotvr1, vb1z = bz * dotvr1;
                    const mixed vp1x = vel1x - vb1x, vp1y = vel1y - vb1y, vp1z = vel1z - vb1z;
                    if (vel2w == 0) {                                           // massless parent (K/middle.cu:151-173)
                        if (dotvr1 != 0) deltaT = deltaR / fabs((double) dotvr1);
                        if (deltaT > stepSize) deltaT = stepSize;
                        dotvr1 = -dotvr1 * hardwallscaleDrude / (fabs((double) dotvr1) * P::SQRT(mass1));
                        const mixed dr = -deltaR + deltaT * dotvr1;
                        p1x += bx * dr; p1y += by * dr; p1z += bz * dr;
                        vel1x = vp1x + bx * dotvr1; vel1y = vp1y + by * dotvr1; vel1z = vp1z + bz * dotvr1;
                        if (isd) { x = p1x; y = p1y; z = p1z; v.x = vel1x; v.y = vel1y; v.z = vel1z; pos_dirty = true; vel_dirty = true; }
                    } else {                                                    // both move (K/middle.cu:174-218)
                        const mixed invTotalMass = P::RECIP(mass1 + mass2);
                        mixed dotvr2 = vel2x * bx + vel2y * by + vel2z * bz;
                        const mixed vb2x = bx * dotvr2, vb2y = by * dotvr2, vb2z = bz * dotvr2;
                        const mixed vp2x = vel2x - vb2x, vp2y = vel2y - vb2y, vp2z = vel2z - vb2z;
                        const mixed vbCMass = (mass1 * dotvr1 + mass2 * dotvr2) * invTotalMass;
                        dotvr1 -= vbCMass;
                        dotvr2 -= vbCMass;
                        if (dotvr1 != dotvr2) deltaT = deltaR / fabs((double) (dotvr1 - dotvr2));
                        if (deltaT > stepSize) deltaT = stepSize;
                        const mixed vBond = hardwallscaleDrude / P::SQRT(mass1);
                        dotvr1 = -dotvr1 * vBond * mass2 * invTotalMass / fabs((double) dotvr1);
                        dotvr2 = -dotvr2 * vBond * mass1 * invTotalMass / fabs((double) dotvr2);
                        const mixed dr1 = -deltaR * mass2 * invTotalMass + deltaT * dotvr1;
                        const mixed dr2 = deltaR * mass1 * invTotalMass + deltaT * dotvr2;
                        dotvr1 += vbCMass;
                        dotvr2 += vbCMass;
                        if (isd) {
                            x = p1x + bx * dr1; y = p1y + by * dr1; z = p1z + bz * dr1;
                            v.x = vp1x + bx * dotvr1; v.y = vp1y + by * dotvr1; v.z = vp1z + bz * dotvr1;
                        } else {
                            x = p2x + bx * dr2; y = p2y + by * dr2; z = p2z + bz * dr2;
                            v.x = vp2x + bx * dotvr2; v.y = vp2y + by * dotvr2; v.z = vp2z + bz * dotvr2;
                        }
                        pos_dirty = true; vel_dirty = true;
                    }
                }
            }
        }

        // ---------------- virtual sites (integration.computeVirtualSites(), HOST:214, 374): after the hard wall, before the images
        if (F & B_VSITE) {
            const unsigned vword = act ? (unsigned) vsite.x : 0u;
            // (the weights and the site's index are fetched HERE, behind the position update: requested right after the tile's first batch --
            // 24 more live registers through the whole tile -- the same box ran 81.6 k steps/s against 84.1 k, round 4)
            real vs_w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            int vs_atom = -1;
            if (vword & VS_WORD_VALID) {
                const double* rec = a.vsite_params + (size_t) vsite.y * 12;
#pragma unroll
                for (int k = 0; k < 12; k++) vs_w[k] = (real) rec[k];
                if (vword & VS_WORD_HOSTED) vs_atom = a.vsite_atom[vsite.y];
            }
            bool placed;
            mixed sx, sy, sz;
            place_virtual_site<real, mixed>(lane, vword, vs_w, pos_dirty, x, y, z, sx, sy, sz, placed, shake_page_b);
            if (placed && (vword & VS_WORD_HOSTED)) IO::store_xyz(a.posq, a.corr, vs_atom, sx, sy, sz);
            else if (placed) { x = sx; y = sy; z = sz; pos_dirty = true; }
        }
        // ---------------- write back
        VV_STAMP(wib, 4);
        if (act && vel_dirty) store_vec(velm, atom, v);
        if (act && pos_dirty) IO::store(a.posq, a.corr, atom, x, y, z, q);
        if ((F & B_VV_KICK) && massive) {
            mixed4 d = {dx, dy, dz, 0};
            if (a.pos_delta) ((mixed4*) a.pos_delta)[atom] = d;
        }
        VV_STAMP(wib, 5);

        // ---------------- image charges (K/imageCharge.cu:10-26): x, y are bit copies of the parent's stored position, z is mirrored
        if ((F & B_IMAGE) && act && (meta & META_HAS_IMAGE)) {
            real4* posq = (real4*) a.posq;
            real4 pp, cp = {0, 0, 0, 0};
            if (pos_dirty) {                   // what IO::store has just written, conversion for conversion (no re-read needed)
                pp.x = (real) x; pp.y = (real) y; pp.z = (real) z; pp.w = (real) q;
                if (IO::kMixed) { cp.x = (real) (x - (real) x); cp.y = (real) (y - (real) y); cp.z = (real) (z - (real) z); }
            } else {                           // untouched parent (massless): its stored bits
                pp = posq[atom];
                if (IO::kMixed) cp = ((const real4*) a.corr)[atom];
            }
            real4 pi = img_p;
            pi.x = pp.x; pi.y = pp.y;
            if (IO::kMixed) {
                real4* corr = (real4*) a.corr;
                real4 ci = img_c;
                ci.x = cp.x; ci.y = cp.y;
                mixed zz = (mixed) pp.z + (mixed) cp.z;
                zz = (mixed) a.mirror * 2 - zz;
                pi.z = (real) zz;
                ci.z = (real) (zz - (real) zz);
                corr[img] = ci;
            } else {
                pi.z = 2 * (mixed) a.mirror - pp.z;
            }
            posq[img] = pi;
        }
    }   // tile loop
    VV_STAMP_DUMP(wib);
    VV_SPAN_END;
}
