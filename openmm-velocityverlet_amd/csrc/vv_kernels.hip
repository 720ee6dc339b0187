// vv_kernels.hip -- hand-written HIP kernels for gfx950 (MI355X, wave64).
//
// Work-item layout.  One work-item per particle; a 64-lane wave holds whole "clusters": every Drude
// pair, and (with the COM temperature group) every molecule, sits inside ONE wave (vv_host.cpp).
// Hence
//   * the Drude partner's velocity/position comes from a cross-lane shuffle, not a second gather;
//   * the molecular centre-of-mass velocity is a segmented wave scan, not the reference's serial
//     per-molecule read-modify-write in global memory (K/drudeNoseHoover.cu:15-25);
//   * per-group kinetic energies are reduced wave -> LDS -> one 64-bit fixed-point atomic per block,
//     so the global sums do not depend on arrival order (bit-reproducible) and need no second
//     "single block" pass (K/drudeNoseHoover.cu:121-151) nor a host round trip (HOST:709-746).
// Global loads are 16/32-byte per lane and, for contiguous molecules, fully coalesced.
//
// Arithmetic.  Each expression keeps the operand types and association of the reference kernel it
// replaces (cited per stage; K/ = platforms/cuda/src/kernels/) and the library is built with
// -ffp-contract=off, so element-wise results equal the CPU oracle bit for bit; only the reductions
// differ (their order, and the reciprocals that feed nothing but sums: Prec::RECIP_SUM).  No MFMA:
// there is no contraction on this path (HBM / latency / fp64-issue bound).
// Build: the Makefile compiles this file twice, in parallel -- VV_KERNELS_PART=1: launch_a / launch_b and the small launchers, =2: launch_fused
// (the one-launch step's instances of vv_kernel_b are half of the device code) -- and links both objects; without the macro one translation
// unit holds everything (make asm, instrumented probe builds).
#ifndef VV_KERNELS_PART
#define VV_KERNELS_PART 0
#endif
#if VV_KERNELS_PART == 2
#define VV_DEVICE_NO_PLAIN_KERNELS      // (vv_kernel_chain / vv_kernel_bump_epoch are not templates: one definition, in part 1)
#endif
#include "vv_kernels.hpp"

#include <hip/hip_ext.h>

#include <algorithm>

#include "vv_host.hpp"
#include "vv_rtc.hpp"

namespace vv {

#include "vv_device.inc"

// ================================================================================ launchers
extern unsigned vv_last_grid_value;      // grid of the most recent A / B launch (instrumented builds read it back)
static inline dim3 grid_for(int nwaves, int block_threads) {
    const int wpb = block_threads / 64;
    return dim3((unsigned) ((nwaves + wpb - 1) / wpb));
}
// Launch with the dispatch's own begin / end timestamps delivered into a pair of events (hipExtLaunchKernelGGL: no barrier packets
// around the kernel, the times are those of the dispatch packet's completion signal -- what rocprofv3's kernel trace reports);
// without events, the plain launch (also the only form used inside a graph capture).
template <typename F, typename... Args>
static inline void vv_launch(F kernel, dim3 g, dim3 b, unsigned lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1, Args... args) {
    if (e0 || e1) hipExtLaunchKernelGGL(kernel, g, b, lds, s, e0, e1, 0, args...);
    else hipLaunchKernelGGL(kernel, g, b, lds, s, args...);
}
// The same for a kernel compiled at run time (vv_rtc.cpp): module launch with the parameter list of the kernel's signature.
static inline hipError_t vv_launch_module(hipFunction_t f, dim3 g, dim3 b, unsigned lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1, void** params) {
    if (e0 || e1) return hipExtModuleLaunchKernel(f, g.x * b.x, 1, 1, b.x, 1, 1, lds, s, params, nullptr, e0, e1, 0);
    return hipModuleLaunchKernel(f, g.x, 1, 1, b.x, 1, 1, lds, s, params, nullptr);
}
// The precision modes.  A kernel template's leading parameters are the mode's types (real, mixed) = (float, float) / (float, double) /
// (double, double); every launcher of this file picks its instance here -- VV_PER_PRECISION names the three, PerPrecision chooses.
template <class K> struct PerPrecision {
    K single, mixed, dbl;
    constexpr K operator()(int precision) const { return precision == VVHIP_SINGLE ? single : precision == VVHIP_MIXED ? mixed : dbl; }
};
#define VV_PER_PRECISION(KERNEL, ...) {&KERNEL<float, float, ##__VA_ARGS__>, &KERNEL<float, double, ##__VA_ARGS__>, &KERNEL<double, double, ##__VA_ARGS__>}
#define VV_PICK(PRECISION, KERNEL, ...) (PerPrecision<decltype(&KERNEL<float, float, ##__VA_ARGS__>)> VV_PER_PRECISION(KERNEL, ##__VA_ARGS__)(PRECISION))
// Kernels A and B have one signature each, whatever the precision mode and the stage sets (vv_dev_kernel_a.inc / vv_dev_kernel_b.inc)
using KernelA = void (*)(const int2*, int, int, void*, const long long*, int, KArgs);
using KernelB = void (*)(const int2*, int, int, const unsigned long long*, const NHDevState*, const ChainLaneBlock*, const int*, KArgs);

// ================================================================================ the compiled stage sets
// Stage-bit sets with their own compiled kernel, one list per kernel kind: VV_SF_A_LIST (kernel A), VV_SF_B_LIST (kernel B) and
// VV_SF_FUSED_LIST (the one-launch step: B's set with A's).  A line X(name, bits) both defines the constant `name` and puts a kernel for
// it, in the three precision modes, into the library: a new specialisation is one line here.  A launch whose stage set is in no list gets
// a kernel compiled at run time (vv_rtc.cpp) or, failing that, the generic kernel with run-time stage bits, which is 15-20 % slower (C5
// went from 74 k to 88 k steps/s when it got its own pair).  The lookup takes a list in order, so the headline sets stand first; a name may
// be built from names above it.
#define VV_SF_A_LIST(X) \
    /* the headline path: the fused middle step without a velm round trip between the kernels (A_NOSTORE / B_KICK), with the arithmetic */ \
    /* work-item layout (runs of identical molecules: every BASELINE bulk configuration) and without; these spell their bits in full */ \
    X(SF_A_MIDDLE_NS_P, A_KICK_FULL | A_KE | A_NOSTORE | A_PERIODIC) \
    X(SF_A_COS_MOM_NS_P, A_KICK_FULL | A_COS | A_BIAS | A_CZ_STORE | A_KE | A_KE_MOM | A_NOSTORE | A_PERIODIC) \
    X(SF_A_MIDDLE_NS, A_KICK_FULL | A_KE | A_NOSTORE) \
    X(SF_A_COS_MOM_NS, A_KICK_FULL | A_COS | A_BIAS | A_CZ_STORE | A_KE | A_KE_MOM | A_NOSTORE)         /* ... and with the cos perturbation (BASELINE C4) */ \
    /* the fused middle step with the round trip (BASELINE configs C1 - C3), the cos perturbation (C4), the electrode slab (C5), constraints */ \
    X(SF_A_MIDDLE, A_KICK_FULL | A_KE) \
    X(SF_A_COS1, A_KICK_FULL | A_COS | A_BIAS | A_CZ_STORE)                                             /* cos acceleration (BASELINE C4): kick + bias moment */ \
    X(SF_A_COS2, A_KE | A_UNBIAS_ACC | A_CZ_LOAD)                                                       /* ... kinetic energies of the bias-free velocities */ \
    X(SF_A_COS_MOM, A_KICK_FULL | A_COS | A_BIAS | A_CZ_STORE | A_KE | A_KE_MOM)                        /* cos acceleration in one launch (moments) */ \
    X(SF_A_EDL, A_KICK_FULL | A_LD | A_EF | A_KE)                                                       /* electrode slab (BASELINE C5): Langevin subset + field */ \
    X(SF_A_MIDDLE_SHAKE, SF_A_MIDDLE | A_SHAKE_V)                                                       /* HBonds constraints solved in-kernel */ \
    X(SF_A_MIDDLE_SHAKE_P, SF_A_MIDDLE_SHAKE | A_PERIODIC) \
    X(SF_A_MIDDLE_SETTLE, SF_A_MIDDLE | A_SETTLE)                                                       /* rigid water (BASELINE C2 made physical): SETTLE only */ \
    X(SF_A_MIDDLE_SETTLE_P, SF_A_MIDDLE_SETTLE | A_PERIODIC) \
    /* ... and the combinations the reference's example scripts actually run: HBonds constraints next to the cos perturbation */ \
    /* (run-bulk.py) and next to the electrode machinery (run-edl.py) */ \
    X(SF_A_COS_MOM_SHAKE, SF_A_COS_MOM | A_SHAKE_V) \
    X(SF_A_EDL_SHAKE, SF_A_EDL | A_SHAKE_V) \
    X(SF_A_LD, A_KICK_FULL | A_LD | A_KE)                                                               /* a Langevin subset without the field (thermostatted wall) */ \
    X(SF_A_EF, A_KICK_FULL | A_EF | A_KE)                                                               /* a field on the bulk without Langevin particles */ \
    X(SF_A_LD_SHAKE, SF_A_LD | A_SHAKE_V) \
    X(SF_A_EF_SHAKE, SF_A_EF | A_SHAKE_V) \
    /* the classic scheme's two halves and the stages of the un-fused entry points */ \
    X(SF_A_KE, A_KE)                                                                                    /* vvhip_scale_velocity / classic first half: sums only */ \
    X(SF_A_VV2, A_KICK_HALF | A_KE)                                                                     /* classic second half */ \
    X(SF_A_KICK, A_KICK_FULL)                                                                           /* vvhip_middle_kick (forceExtra known to be zero) */ \
    X(SF_A_KICK_FE, A_FE_LOAD | A_KICK_FULL)                                                            /* ... with extra forces */ \
    X(SF_A_POS1, A_POS1)                                                                                /* vvhip_middle_half_drift1 */ \
    /* The classic scheme (two thermostat applications per step) of every BASELINE configuration with what the example scripts add to it: */ \
    /* second half = half kick (+ extra forces kept for the next first half) + sums, first half = scale + half kick + positions. */ \
    X(SF_A_KE_P, A_KE | A_PERIODIC)                                                                     /* large boxes */ \
    X(SF_A_VV2_P, SF_A_VV2 | A_PERIODIC) \
    X(SF_A_VV2_SHAKE, SF_A_VV2 | A_SHAKE_V)                                                             /* + HBonds */ \
    X(SF_A_VV2_SETTLE, SF_A_VV2 | A_SETTLE)                                                             /* rigid water */ \
    X(SF_A_VV2_EDL, SF_A_VV2 | A_FE_STORE | A_LD | A_EF)                                                /* electrode slab */ \
    X(SF_A_VV2_EDL_SHAKE, SF_A_VV2_EDL | A_SHAKE_V) \
    X(SF_A_COS_MOM_VV1, A_BIAS | A_KE | A_CZ_STORE | A_KE_MOM)                                          /* cos perturbation: sums of the first half */ \
    X(SF_A_COS_MOM_VV2, SF_A_COS_MOM_VV1 | A_FE_STORE | A_COS | A_KICK_HALF)                            /* ... half kick + sums of the second half */ \
    X(SF_A_COS_MOM_VV2_SHAKE, SF_A_COS_MOM_VV2 | A_SHAKE_V)
#define VV_SF_B_LIST(X) \
    /* the headline path (A_NOSTORE / B_KICK) with the arithmetic work-item layout: plain, without hard wall, very large (the chain as its */ \
    /* own launch), cos perturbation, then next to the mailbox exchange of sharded runs (the chain stays in kernel B's head there, */ \
    /* whatever the size); these spell their bits in full */ \
    X(SF_B_MIDDLE_HW_K_P, B_CHAIN | B_SCALE | B_DRIFT_MIDDLE | B_HARDWALL | B_KICK | B_PERIODIC) \
    X(SF_B_MIDDLE_K_P, B_CHAIN | B_SCALE | B_DRIFT_MIDDLE | B_KICK | B_PERIODIC) \
    X(SF_B_MIDDLE_HW_NC_K_P, B_SCALE | B_DRIFT_MIDDLE | B_HARDWALL | B_KICK | B_PERIODIC) \
    X(SF_B_COS_HW_MOM_K_P, B_CHAIN | B_SCALE | B_UNBIAS | B_CZ_LOAD | B_DRIFT_MIDDLE | B_HARDWALL | B_KE_MOM | B_KICK | B_PERIODIC) \
    X(SF_B_MIDDLE_HW_MB_K_P, B_CHAIN | B_SCALE | B_DRIFT_MIDDLE | B_HARDWALL | B_MAILBOX | B_KICK | B_PERIODIC) \
    X(SF_B_MIDDLE_MB_K_P, B_CHAIN | B_SCALE | B_DRIFT_MIDDLE | B_MAILBOX | B_KICK | B_PERIODIC) \
    X(SF_B_COS_HW_MOM_MB_K_P, B_CHAIN | B_SCALE | B_UNBIAS | B_CZ_LOAD | B_DRIFT_MIDDLE | B_HARDWALL | B_KE_MOM | B_MAILBOX | B_KICK | B_PERIODIC) \
    X(SF_B_VV1_HW_P, B_CHAIN | B_SCALE | B_VV_KICK | B_HARDWALL | B_PERIODIC)                           /* classic scheme, arithmetic layout, chain in the kernel (1.1 - 2.6 M particles) */ \
    X(SF_B_SCALE_P, B_CHAIN | B_SCALE | B_PERIODIC) \
    /* ... the same with loaded slot words */ \
    X(SF_B_MIDDLE_HW_K, B_CHAIN | B_SCALE | B_DRIFT_MIDDLE | B_HARDWALL | B_KICK) \
    X(SF_B_MIDDLE_K, B_CHAIN | B_SCALE | B_DRIFT_MIDDLE | B_KICK) \
    X(SF_B_MIDDLE_HW_NC_K, B_SCALE | B_DRIFT_MIDDLE | B_HARDWALL | B_KICK) \
    X(SF_B_MIDDLE_HW_MB_K, B_CHAIN | B_SCALE | B_DRIFT_MIDDLE | B_HARDWALL | B_MAILBOX | B_KICK) \
    X(SF_B_MIDDLE_MB_K, B_CHAIN | B_SCALE | B_DRIFT_MIDDLE | B_MAILBOX | B_KICK) \
    X(SF_B_COS_HW_MOM_K, B_CHAIN | B_SCALE | B_UNBIAS | B_CZ_LOAD | B_DRIFT_MIDDLE | B_HARDWALL | B_KE_MOM | B_KICK) \
    X(SF_B_COS_HW_MOM_MB_K, B_CHAIN | B_SCALE | B_UNBIAS | B_CZ_LOAD | B_DRIFT_MIDDLE | B_HARDWALL | B_KE_MOM | B_MAILBOX | B_KICK) \
    /* the fused middle step of a Drude system with / without hard wall (BASELINE configs C3 / C1, C2), with the cos perturbation (C4) */ \
    X(SF_B_MIDDLE_HW, B_CHAIN | B_SCALE | B_DRIFT_MIDDLE | B_HARDWALL) \
    X(SF_B_MIDDLE, B_CHAIN | B_SCALE | B_DRIFT_MIDDLE) \
    X(SF_B_COS_HW, B_CHAIN | B_SCALE | B_UNBIAS | B_CZ_LOAD | B_DRIFT_MIDDLE | B_HARDWALL) \
    X(SF_B_COS_HW_MOM, SF_B_COS_HW | B_KE_MOM) \
    X(SF_B_EDL, SF_B_MIDDLE_HW | B_IMAGE)                                                               /* ... + image mirror */ \
    X(SF_B_MIDDLE_HW_NC, B_SCALE | B_DRIFT_MIDDLE | B_HARDWALL)                                         /* large systems: the chain runs as its own 1-wave launch in front */ \
    X(SF_B_MIDDLE_HW_MB, SF_B_MIDDLE_HW | B_MAILBOX) \
    X(SF_B_MIDDLE_MB, SF_B_MIDDLE | B_MAILBOX)                                                          /* sharded runs of systems without Drude pairs */ \
    /* HBonds constraints solved in-kernel; large constrained boxes (the chain as its own launch): clusters solved without the thermostat wave */ \
    X(SF_B_MIDDLE_HW_SHAKE, SF_B_MIDDLE_HW | B_SHAKE) \
    X(SF_B_MIDDLE_HW_NC_SHAKE, SF_B_MIDDLE_HW_NC | B_SHAKE) \
    /* ... and the other stage sets large boxes produce (no thermostat wave in kernel B): without Drude pairs (water, plain ionic liquids), */ \
    /* rigid water, the cos perturbation in its three-launch form -- each with loaded and with computed slot words */ \
    X(SF_B_MIDDLE_NC_K, B_SCALE | B_DRIFT_MIDDLE | B_KICK) \
    X(SF_B_MIDDLE_NC_K_P, SF_B_MIDDLE_NC_K | B_PERIODIC) \
    X(SF_B_MIDDLE_NC_SHAKE, B_SCALE | B_DRIFT_MIDDLE | B_SHAKE) \
    X(SF_B_MIDDLE_NC_SHAKE_P, SF_B_MIDDLE_NC_SHAKE | B_PERIODIC) \
    X(SF_B_MIDDLE_SETTLE, SF_B_MIDDLE | B_SETTLE) \
    X(SF_B_MIDDLE_NC_SETTLE, B_SCALE | B_DRIFT_MIDDLE | B_SETTLE) \
    X(SF_B_MIDDLE_NC_SETTLE_P, SF_B_MIDDLE_NC_SETTLE | B_PERIODIC) \
    X(SF_B_COS_HW_NC, B_SCALE | B_UNBIAS | B_CZ_LOAD | B_DRIFT_MIDDLE | B_HARDWALL) \
    X(SF_B_COS_HW_NC_P, SF_B_COS_HW_NC | B_PERIODIC) \
    /* the classic scheme's two thermostat applications in large boxes: scale + half kick + positions (+ hard wall), and scale alone */ \
    X(SF_B_VV1_HW_NC, B_SCALE | B_VV_KICK | B_HARDWALL) \
    X(SF_B_VV1_HW_NC_P, SF_B_VV1_HW_NC | B_PERIODIC) \
    X(SF_B_SCALE_NC, B_SCALE) \
    X(SF_B_SCALE_NC_P, SF_B_SCALE_NC | B_PERIODIC) \
    X(SF_B_MIDDLE_HW_NC_SHAKE_P, SF_B_MIDDLE_HW_NC_SHAKE | B_PERIODIC) \
    X(SF_B_MIDDLE_HW_SHAKE_P, SF_B_MIDDLE_HW_SHAKE | B_PERIODIC) \
    X(SF_B_MIDDLE_SHAKE, SF_B_MIDDLE | B_SHAKE) \
    /* ... and the combinations the reference's example scripts actually run: HBonds constraints next to the cos perturbation */ \
    /* (run-bulk.py) and next to the electrode machinery (run-edl.py), and the sharded variants of the constrained / perturbed box */ \
    X(SF_B_COS_HW_MOM_SHAKE, SF_B_COS_HW_MOM | B_SHAKE) \
    X(SF_B_EDL_SHAKE, SF_B_EDL | B_SHAKE) \
    X(SF_B_COS_HW_MOM_MB, SF_B_COS_HW_MOM | B_MAILBOX) \
    X(SF_B_MIDDLE_HW_SHAKE_MB, SF_B_MIDDLE_HW_SHAKE | B_MAILBOX) \
    /* the classic scheme's two halves and the stages of the un-fused entry points */ \
    X(SF_B_SCALE, B_CHAIN | B_SCALE)                                                                    /* vvhip_scale_velocity / classic second half */ \
    X(SF_B_VV1_HW, B_CHAIN | B_SCALE | B_VV_KICK | B_HARDWALL)                                          /* classic first half */ \
    X(SF_B_VV1, B_CHAIN | B_SCALE | B_VV_KICK) \
    X(SF_B_POS2, B_POS2)                                                                                /* vvhip_middle_half_drift2 */ \
    X(SF_B_POS3_HW, B_POS3 | B_HARDWALL)                                                                /* vvhip_middle_finish */ \
    X(SF_B_POS3, B_POS3) \
    /* the classic scheme of every BASELINE configuration with what the example scripts add to it: HBonds, rigid water, electrode slab, cos */ \
    X(SF_B_VV1_HW_SHAKE, SF_B_VV1_HW | B_SHAKE) \
    X(SF_B_VV1_SETTLE, SF_B_VV1 | B_SETTLE) \
    X(SF_B_VV1_EDL, SF_B_VV1_HW | B_IMAGE) \
    X(SF_B_VV1_EDL_SHAKE, SF_B_VV1_EDL | B_SHAKE) \
    X(SF_B_COS_SCALE_MOM, B_CHAIN | B_SCALE | B_UNBIAS | B_CZ_LOAD | B_KE_MOM)                          /* cos perturbation: second half's scaling */ \
    X(SF_B_COS_VV1_HW_MOM, SF_B_COS_SCALE_MOM | B_VV_KICK | B_HARDWALL)                                 /* ... first half */ \
    X(SF_B_COS_VV1_HW_MOM_SHAKE, SF_B_COS_VV1_HW_MOM | B_SHAKE) \
    X(SF_B_MIDDLE_SETTLE_P, SF_B_MIDDLE_SETTLE | B_PERIODIC)                                            /* rigid water with the arithmetic layout and the chain in the kernel (forced layouts: automatic ones start where the chain is its own launch) */
#define VV_SF_NAME(NAME, BITS) constexpr uint32_t NAME = (BITS);
VV_SF_A_LIST(VV_SF_NAME)
VV_SF_B_LIST(VV_SF_NAME)
#undef VV_SF_NAME
// The one-launch step's kernel-B sets that no two-launch step uses: the cos perturbation keeps no cos(kz) cache between the halves
constexpr uint32_t SF_B_COS_HW_MOM_F = B_CHAIN | B_SCALE | B_UNBIAS | B_DRIFT_MIDDLE | B_HARDWALL | B_KE_MOM;
constexpr uint32_t SF_B_COS_SCALE_MOM_F = B_CHAIN | B_SCALE | B_UNBIAS | B_KE_MOM;                                  // classic scheme: second half / first half
constexpr uint32_t SF_B_COS_VV1_HW_MOM_F = SF_B_COS_SCALE_MOM_F | B_VV_KICK | B_HARDWALL;
#define VV_SF_FUSED_LIST(X) \
    X(SF_B_MIDDLE_HW, SF_A_MIDDLE)                               /* BASELINE C3 */ \
    X(SF_B_MIDDLE, SF_A_MIDDLE)                                  /* C1, C2 */ \
    X(SF_B_EDL, SF_A_EDL)                                        /* C5 */ \
    X(SF_B_COS_HW_MOM_F, SF_A_COS_MOM)                           /* C4 */ \
    X(SF_B_MIDDLE_HW_SHAKE, SF_A_MIDDLE_SHAKE)                   /* ... with their HBonds / rigid water */ \
    X(SF_B_MIDDLE_SETTLE, SF_A_MIDDLE_SETTLE) \
    X(SF_B_EDL_SHAKE, SF_A_EDL_SHAKE) \
    X(SF_B_COS_HW_MOM_F | B_SHAKE, SF_A_COS_MOM_SHAKE) \
    X(SF_B_MIDDLE_HW_MB, SF_A_MIDDLE)                            /* sharded runs (xGMI mailbox behind the local rendezvous): C3, C4, water */ \
    X(SF_B_COS_HW_MOM_F | B_MAILBOX, SF_A_COS_MOM) \
    X(SF_B_MIDDLE_MB, SF_A_MIDDLE) \
    X(SF_B_MIDDLE_HW_SHAKE_MB, SF_A_MIDDLE_SHAKE) \
    X(SF_B_VV1_HW, SF_A_KE)                                      /* classic scheme, first half: sums + scaling + half kick + drift (C3) */ \
    X(SF_B_VV1, SF_A_KE)                                         /* ... C1, C2 */ \
    X(SF_B_SCALE, SF_A_VV2)                                      /* classic scheme, second half: half kick + sums + scaling */ \
    X(SF_B_SCALE, SF_A_KE)                                       /* a thermostat application on its own (vvhip_scale_velocity) */ \
    X(SF_B_VV1_HW_SHAKE, SF_A_KE)                                /* ... the classic scheme of the other BASELINE configurations and their constraints */ \
    X(SF_B_SCALE, SF_A_VV2_SHAKE) \
    X(SF_B_VV1_SETTLE, SF_A_KE) \
    X(SF_B_SCALE, SF_A_VV2_SETTLE) \
    X(SF_B_VV1_EDL, SF_A_KE) \
    X(SF_B_SCALE, SF_A_VV2_EDL) \
    X(SF_B_VV1_EDL_SHAKE, SF_A_KE) \
    X(SF_B_SCALE, SF_A_VV2_EDL_SHAKE) \
    X(SF_B_COS_VV1_HW_MOM_F, SF_A_COS_MOM_VV1) \
    X(SF_B_COS_SCALE_MOM_F, SF_A_COS_MOM_VV2) \
    X(SF_B_COS_VV1_HW_MOM_F | B_SHAKE, SF_A_COS_MOM_VV1) \
    X(SF_B_COS_SCALE_MOM_F, SF_A_COS_MOM_VV2_SHAKE)

// Which specialised kernels are compiled with the static mass tables; a launch whose flags disagree with the build falls through to
// the generic kernel.  Measured on MI355X (gpurun_out/r02c-e): kernel B gains at every size (two IEEE fp64 divisions per pair lane
// gone, 140 -> 101 VGPRs; C3 5.74 -> 5.29 us with the chain fix, 8.9 M particles unchanged), kernel A does not -- with the Koenig
// form of its KE stage it needs one cheap reciprocal per lane, and the 16 bytes per lane of table traffic cost it 13 % at
// 8.9 M particles (217 -> 247 us) for nothing at 111 k.  So: B with the table (VV_SF_MTAB_B=1), A without (VV_SF_MTAB_A=0).
#ifndef VV_SF_MTAB_A
#define VV_SF_MTAB_A 0
#endif
#ifndef VV_SF_MTAB_B
#define VV_SF_MTAB_B 1
#endif
constexpr uint32_t SF_AM = VV_SF_MTAB_A ? A_MTAB : 0u, SF_BM = VV_SF_MTAB_B ? B_MTAB : 0u;
#if VV_KERNELS_PART != 2
bool sf_kernels_use_mass_table(int kernel) { return kernel == 0 ? VV_SF_MTAB_A != 0 : VV_SF_MTAB_B != 0; }
#endif

// A list as a table: per row the stage set a launch must ask for (kernel B's and, in the one-launch step, kernel A's) and its kernels.
template <class K> struct SfRow { uint32_t bits, bits_a; PerPrecision<K> kernel; };
template <class K, size_t N>
static K compiled_kernel(const SfRow<K> (&rows)[N], int precision, uint32_t bits, uint32_t bits_a = 0u) {
    for (const SfRow<K>& r : rows)
        if (r.bits == bits && r.bits_a == bits_a) return r.kernel(precision);
    return nullptr;
}
template <class K, size_t N>
constexpr bool rows_differ(const SfRow<K> (&rows)[N]) {
    for (size_t i = 0; i < N; i++)
        for (size_t j = 0; j < i; j++)
            if (rows[i].bits == rows[j].bits && rows[i].bits_a == rows[j].bits_a) return false;
    return true;
}
// The compiled kernels carry the three-link chain only
static inline bool chain_is_compiled(const KArgs& a) { return !(a.flags & B_CHAIN) || a.chain.num_chains == 3; }
// LDS of the in-kernel constraint / virtual-site solvers: one page per tile wave, 7 values of the mode's `mixed` type per lane
static inline unsigned solver_lds(int precision, int block_threads, bool used) {
    return used ? (unsigned) (block_threads / 64) * 64u * 7u * (precision == VVHIP_SINGLE ? 4u : 8u) : 0u;
}
// A kernel compiled at run time for exactly the launch's stage sets (vv_rtc.cpp), with the parameter list of kernel A's / kernel B's signature
static hipError_t launch_module_a(hipFunction_t f, dim3 g, dim3 b, unsigned lds, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, const KArgs& a, int* route) {
    const int2* slots = a.slots; int nwaves = a.nwaves, wpb = (int) (b.x >> 6), padded = a.padded;
    void* velm = a.velm; const long long* force = a.force;
    void* params[] = {&slots, &nwaves, &wpb, &velm, &force, &padded, const_cast<KArgs*>(&a)};
    vv_rtc_launches[0]++;
    if (route) *route = ROUTE_RUNTIME;
    return vv_launch_module(f, g, b, lds, s, ev0, ev1, params);
}
static hipError_t launch_module_b(hipFunction_t f, dim3 g, dim3 b, unsigned lds, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, const unsigned long long* acc, const KArgs& a, int* route) {
    const int2* slots = a.slots; int nwaves = a.nwaves, wpb = (int) (b.x >> 6);
    const NHDevState* nh = a.nh; const ChainLaneBlock* lane_const = a.lane_const; const int* seg_base = a.seg_base;
    void* params[] = {&slots, &nwaves, &wpb, &acc, &nh, &lane_const, &seg_base, const_cast<KArgs*>(&a)};
    vv_rtc_launches[1]++;
    if (route) *route = ROUTE_RUNTIME;
    return vv_launch_module(f, g, b, lds, s, ev0, ev1, params);
}

#if VV_KERNELS_PART != 2
// (a row names its set by NAME, which VV_SF_NAME has defined as BITS)
#define VV_SF_ROW_A(NAME, BITS) {NAME | SF_AM, 0u, VV_PER_PRECISION(vv_kernel_a, NAME | SF_AM)},
#define VV_SF_ROW_B(NAME, BITS) {NAME | SF_BM, 0u, VV_PER_PRECISION(vv_kernel_b, NAME | SF_BM)},
// kernel A's table and generic kernel (the stage bits are read at run time), then kernel B's
constexpr SfRow<KernelA> sf_rows_a[] = {VV_SF_A_LIST(VV_SF_ROW_A)};
constexpr PerPrecision<KernelA> generic_kernel_a = VV_PER_PRECISION(vv_kernel_a, 0u);
constexpr PerPrecision<KernelB> generic_kernel_b = VV_PER_PRECISION(vv_kernel_b, 0u);
constexpr SfRow<KernelB> sf_rows_b[] = {VV_SF_B_LIST(VV_SF_ROW_B)};
#undef VV_SF_ROW_A
#undef VV_SF_ROW_B
static_assert(rows_differ(sf_rows_a) && rows_differ(sf_rows_b), "a stage set is listed twice");

// Launches that found no compiled specialisation of their stage set and ran the generic kernel: the caller counts them per plan
// through `route` (vvhip_generic_launches reads the counts; VVHIP_WARN_GENERIC=1 also prints one line on stderr per stage set).
static void note_generic(int* route) {
    if (route) *route = ROUTE_GENERIC;
}

// The routes of a launch, in this order: a kernel compiled at run time where VVHIP_RTC=2 asks for one always, the compiled list, a kernel
// compiled at run time for a stage set the list has not (VVHIP_RTC=1, default), the generic kernel.
hipError_t launch_a(int precision, const KArgs& a_in, int block_threads, int grid_cap, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, int* route) {
    KArgs a = a_in;
    if (route) *route = ROUTE_COMPILED;
    dim3 g = grid_for(a.nwaves, block_threads);
    if ((int) g.x > grid_cap) g.x = (unsigned) grid_cap;          // beyond that the kernel strides over tiles
    vv_last_grid_value = g.x;
    if (g.x > (unsigned) ACC_SLOTS) a.acc_exclusive = 0;          // several blocks per accumulator slot: atomics (block_accumulate)
    const dim3 b(block_threads);
    const unsigned lds = solver_lds(precision, block_threads, (a.flags & A_CONS) != 0);
    hipFunction_t f = rtc_mode() >= 2 ? rtc_kernel('A', precision, a.flags, 3) : nullptr;
    KernelA k = f ? nullptr : compiled_kernel(sf_rows_a, precision, a.flags);
    if (!f && !k && rtc_mode() == 1) f = rtc_kernel('A', precision, a.flags, 3);
    if (f) return launch_module_a(f, g, b, lds, s, ev0, ev1, a, route);
    if (!k) { note_generic(route); k = generic_kernel_a(precision); }
    vv_launch(k, g, b, lds, s, ev0, ev1, a.slots, a.nwaves, (int) (b.x >> 6), a.velm, a.force, a.padded, a);
    return hipGetLastError();
}
hipError_t launch_b(int precision, const KArgs& a, int block_threads, int grid_cap, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, int* route) {
    if (route) *route = ROUTE_COMPILED;
    // block_threads counts the tile waves; B_CHAIN adds the block's thermostat wave.  Beyond grid_cap blocks the kernel strides
    // over tiles and the per-block thermostat work is amortised.
    dim3 g = grid_for(a.nwaves, block_threads);
    if ((int) g.x > grid_cap) g.x = (unsigned) grid_cap;
    vv_last_grid_value = g.x;
    const dim3 b(block_threads + ((a.flags & B_CHAIN) ? 64 : 0));
    const unsigned lds = solver_lds(precision, block_threads, (a.flags & (B_CONS | B_VSITE)) != 0);
    // (a run-time kernel's thermostat wave is built for the plan's chain length)
    hipFunction_t f = rtc_mode() >= 2 ? rtc_kernel('B', precision, a.flags, a.chain.num_chains) : nullptr;
    KernelB k = f || !chain_is_compiled(a) ? nullptr : compiled_kernel(sf_rows_b, precision, a.flags);
    if (!f && !k && rtc_mode() == 1) f = rtc_kernel('B', precision, a.flags, a.chain.num_chains);
    if (f) return launch_module_b(f, g, b, lds, s, ev0, ev1, a.acc, a, route);
    if (!k) { note_generic(route); k = generic_kernel_b(precision); }
    vv_launch(k, g, b, lds, s, ev0, ev1, a.slots, a.nwaves, (int) (b.x >> 6), (const unsigned long long*) a.acc, a.nh, a.lane_const, a.seg_base, a);
    return hipGetLastError();
}
#endif      // VV_KERNELS_PART != 2
#if VV_KERNELS_PART != 1
// ---- fused step: kernel A's stage set `a.flags_a` and kernel B's `a.flags` in ONE launch (vv_device.inc: "fused step").  Every tile needs a
// wave of its own (it stays in registers across the rendezvous) and the blocks must be resident together: the caller (vv_api.cpp:
// use_fused) has checked the launch shape; `blocks_per_cu` != nullptr only ASKS how many blocks of this kernel a CU holds and launches
// nothing.  hipErrorNotSupported: no kernel for this pair of stage sets (the caller then takes the two-launch path).
#define VV_SF_ROW_FUSED(SFB, SFA) {(SFB) | SF_BM, SFA, VV_PER_PRECISION(vv_kernel_b, (SFB) | SF_BM, SFA)},
constexpr SfRow<KernelB> sf_rows_fused[] = {VV_SF_FUSED_LIST(VV_SF_ROW_FUSED)};
#undef VV_SF_ROW_FUSED
template <size_t N>
constexpr bool rows_are_pairs(const SfRow<KernelB> (&rows)[N]) {
    for (const SfRow<KernelB>& r : rows)
        if (!(r.bits & B_CHAIN) || r.bits_a == 0) return false;
    return true;
}
static_assert(rows_differ(sf_rows_fused), "a pair of stage sets is listed twice");
static_assert(rows_are_pairs(sf_rows_fused), "the one-launch step needs the thermostat wave (B_CHAIN) and a stage set of kernel A");
hipError_t launch_fused(int precision, const KArgs& a, int block_threads, const unsigned long long* rendezvous, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, int* route, int* blocks_per_cu) {
    if (route) *route = ROUTE_COMPILED;
    const dim3 g = grid_for(a.nwaves, block_threads);
    const dim3 b(block_threads + 64);                      // the tile waves + the block's thermostat wave
    if (!(a.flags & B_CHAIN) || a.flags_a == 0 || (int) g.x > ACC_SLOTS || b.x > 512) return hipErrorNotSupported;
    const unsigned lds = solver_lds(precision, block_threads, (a.flags & (B_CONS | B_VSITE)) || (a.flags_a & A_CONS));
    vv_last_grid_value = g.x;
    if (KernelB k = (rtc_mode() < 2 && chain_is_compiled(a)) ? compiled_kernel(sf_rows_fused, precision, a.flags, a.flags_a) : nullptr) {
        if (blocks_per_cu) return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k, (int) b.x, lds);
        vv_launch(k, g, b, lds, s, ev0, ev1, a.slots, a.nwaves, (int) (b.x >> 6), rendezvous, a.nh, a.lane_const, a.seg_base, a);
        return hipGetLastError();
    }
    // any other pair of stage sets (and every pair with VVHIP_RTC=2): compiled at run time from the library's own source
    if (hipFunction_t f = rtc_mode() >= 1 ? rtc_kernel('B', precision, a.flags, a.chain.num_chains, a.flags_a) : nullptr) {
        if (blocks_per_cu) return hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, f, (int) b.x, lds);
        return launch_module_b(f, g, b, lds, s, ev0, ev1, rendezvous, a, route);
    }
    return hipErrorNotSupported;
}
#endif      // VV_KERNELS_PART != 1
#if VV_KERNELS_PART != 2
hipError_t launch_chain(const NHConst& c, NHDevState* st, unsigned long long* acc, hipStream_t s) {
    hipLaunchKernelGGL(vv_kernel_chain, dim3(1), dim3(64), 0, s, c, st, acc);
    return hipGetLastError();
}
hipError_t launch_tether(int precision, const TetherArgs& t, int block_threads, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    vv_launch(VV_PICK(precision, vv_kernel_tether), grid_for(t.nwaves, block_threads), dim3(block_threads), 0, s, ev0, ev1, t.slots, t.nwaves, block_threads / 64, t);
    return hipGetLastError();
}
hipError_t launch_mass_table(int precision, const void* velm, const int2* slots, int nwaves, double* slot_m, double* slot_f, hipStream_t s) {
    if (nwaves <= 0) return hipSuccess;
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_mass_table), dim3((unsigned) ((nwaves + 3) / 4)), dim3(256), 0, s, velm, slots, nwaves, slot_m, slot_f);
    return hipGetLastError();
}
hipError_t launch_fill_normals(float4* out, uint32_t count, uint64_t seed, unsigned long long* epoch, hipStream_t s) {
    if (count == 0) return hipSuccess;
    const unsigned blocks = (count + 255) / 256 > 1024 ? 1024 : (count + 255) / 256;
    hipLaunchKernelGGL(vv_kernel_fill_normals, dim3(blocks), dim3(256), 0, s, out, count, seed, (const unsigned long long*) epoch);
    hipLaunchKernelGGL(vv_kernel_bump_epoch, dim3(1), dim3(1), 0, s, epoch);
    return hipGetLastError();
}
hipError_t launch_image_pairs(int precision, void* posq, void* corr, const int2* pairs, int npairs, double mirror, hipStream_t s) {
    if (npairs <= 0) return hipSuccess;
    const int blocks = (npairs + 255) / 256;
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_images), dim3(blocks), dim3(256), 0, s, posq, corr, pairs, npairs, mirror);
    return hipGetLastError();
}
hipError_t launch_report(int precision, const ReportArgs& a, int block_threads, int grid_cap, hipStream_t s) {
    const int wpb = block_threads / 64;
    const int g1 = std::max(1, std::min((a.nwaves + wpb - 1) / wpb, grid_cap));
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_report_lanes), dim3((unsigned) g1), dim3(block_threads), 0, s, a);
    const hipError_t e = hipGetLastError();
    const int items = a.nmol + a.ncross;
    if (e != hipSuccess || items == 0) return e;
    const int g2 = std::max(1, std::min((items + block_threads - 1) / block_threads, grid_cap));
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_report_molecules), dim3((unsigned) g2), dim3(block_threads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_series_append(const SeriesArgs& a, int grid_cap, hipStream_t s) {
    const long long g = a.rep_out ? std::min<long long>((a.rep_mol_words + 255) / 256, grid_cap) : 1;
    hipLaunchKernelGGL(vv_kernel_series_append, dim3((unsigned) std::max<long long>(1, g)), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cm_motion(int precision, const CmmArgs& a, int block_threads, int grid_cap, hipStream_t s) {
    const int wpb = block_threads / 64;
    const int g = std::max(1, std::min((a.rep.nwaves + wpb - 1) / wpb, grid_cap));
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_cmm_sum), dim3((unsigned) g), dim3(block_threads), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_cmm_subtract), dim3((unsigned) g), dim3(block_threads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_barostat(int precision, const BarostatArgs& a, int block_threads, int grid_cap, hipStream_t s) {
    const int wpb = block_threads / 64;
    const int g = std::max(1, std::min(std::max((a.nwaves + wpb - 1) / wpb, (a.nlaneless + block_threads - 1) / block_threads), grid_cap));
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_barostat_sum), dim3((unsigned) g), dim3(block_threads), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_barostat_shift), dim3((unsigned) g), dim3(block_threads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_thermalize(int precision, const ThermalizeArgs& a, int grid_cap, hipStream_t s) {
    const int g = std::max(1, std::min(std::max((a.nwaves + 7) / 8, (a.nlaneless + 511) / 512), grid_cap));
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_thermalize), dim3((unsigned) g), dim3(512), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_digest(const DigestArgs& a, int block_threads, int grid_cap, hipStream_t s) {
    if (a.nwords == 0) return hipSuccess;
    if (block_threads < 64 || block_threads > 512 || block_threads % 64) return hipErrorInvalidValue;
    const unsigned long long want = (a.nwords / 4 + block_threads - 1) / block_threads;      // one 16-byte group per thread and pass
    const unsigned g = (unsigned) std::max<unsigned long long>(1, std::min<unsigned long long>(want, (unsigned long long) std::max(1, grid_cap)));
    hipLaunchKernelGGL(vv_kernel_digest, dim3(g), dim3((unsigned) block_threads), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_frame(int precision, const FrameArgs& a, bool float64, int grid_cap, hipStream_t s) {
    const dim3 g((unsigned) std::max(1, std::min((a.n + 511) / 512, std::max(1, grid_cap))));
    const auto k = a.subset ? (float64 ? VV_PICK(precision, vv_kernel_frame, double, true) : VV_PICK(precision, vv_kernel_frame, float, true))
                            : (float64 ? VV_PICK(precision, vv_kernel_frame, double, false) : VV_PICK(precision, vv_kernel_frame, float, false));
    hipLaunchKernelGGL(k, g, dim3(512), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vv_kernel_frame_advance, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_profile(int precision, const ProfileArgs& a, int grid_cap, hipStream_t s) {
    const dim3 g((unsigned) std::max(1, std::min((a.n + 511) / 512, std::max(1, grid_cap))));
    const size_t table_bytes = (size_t) a.table_words * sizeof(long long);
    const bool lds = table_bytes <= PROFILE_LDS_BYTES;
    const auto k = a.group ? (lds ? VV_PICK(precision, vv_kernel_profile, true, true) : VV_PICK(precision, vv_kernel_profile, true, false))
                           : (lds ? VV_PICK(precision, vv_kernel_profile, false, true) : VV_PICK(precision, vv_kernel_profile, false, false));
    hipLaunchKernelGGL(k, g, dim3(512), lds ? (unsigned) table_bytes : 0u, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vv_kernel_profile_advance, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
template <bool MOLECULES, bool GROUPED>
static auto pick_msd(int precision, bool lds) {
    return lds ? VV_PICK(precision, vv_kernel_msd, MOLECULES, GROUPED, true) : VV_PICK(precision, vv_kernel_msd, MOLECULES, GROUPED, false);
}
hipError_t launch_msd(int precision, const MsdArgs& a, int block_threads, int grid_cap, hipStream_t s) {
    if (block_threads < 64 || block_threads > 512 || block_threads % 64) return hipErrorInvalidValue;
    const dim3 g((unsigned) std::max(1, std::min((a.n + block_threads - 1) / block_threads, std::max(1, grid_cap))));
    const size_t table_bytes = (size_t) a.table_words * sizeof(long long);
    const bool lds = table_bytes <= PROFILE_LDS_BYTES;
    const auto k = a.first ? (a.group ? pick_msd<true, true>(precision, lds) : pick_msd<true, false>(precision, lds))
                           : (a.group ? pick_msd<false, true>(precision, lds) : pick_msd<false, false>(precision, lds));
    hipLaunchKernelGGL(k, g, dim3((unsigned) block_threads), lds ? (unsigned) table_bytes : 0u, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vv_kernel_msd_advance, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_msd_floor(long long* words, hipStream_t s) {
    hipLaunchKernelGGL(vv_kernel_msd_floor, dim3(1), dim3(64), 0, s, words);
    return hipGetLastError();
}
size_t rdf_lds_bytes(int nbins, int copies) { return (size_t) RDF_TILE * (3 * sizeof(double) + sizeof(int)) + (size_t) copies * (size_t) nbins * sizeof(unsigned int); }
hipError_t launch_rdf(int precision, const RdfArgs& a, int grid_cap, hipStream_t s) {
    // what the kernels rely on: a private word cannot wrap, the histograms fit the block's LDS, the planes hold the sites
    if (a.max_jsites < 1 || (long long) a.max_jsites * RDF_TILE >= (1ll << 32)) return hipErrorInvalidValue;
    if (a.nbins < 1 || a.copies < 1 || a.copies > RDF_TILE / 64 || rdf_lds_bytes(a.nbins, a.copies) > PROFILE_LDS_BYTES) return hipErrorInvalidValue;
    if (a.n < 0 || a.stride < a.n || a.num_items < 0) return hipErrorInvalidValue;
    const dim3 gg((unsigned) std::max(1, std::min((a.n + 255) / 256, std::max(1, grid_cap))));
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_rdf_gather), gg, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 gp((unsigned) std::max(1, a.num_items));
    const unsigned lds = (unsigned) rdf_lds_bytes(a.nbins, a.copies);
    if (a.mol) hipLaunchKernelGGL(vv_kernel_rdf_pairs<true>, gp, dim3(RDF_TILE), lds, s, a);
    else hipLaunchKernelGGL(vv_kernel_rdf_pairs<false>, gp, dim3(RDF_TILE), lds, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(vv_kernel_rdf_advance, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_current(int precision, const CurrentArgs& a, int block_threads, int grid_cap, hipStream_t s) {
    // what the kernels rely on: the block's LDS copy holds the groups, the row's words are the classes'
    if (block_threads < 64 || block_threads > 512 || block_threads % 64) return hipErrorInvalidValue;
    if (a.num_groups < 1 || a.num_groups > CUR_MAX_GROUPS || a.n < 0 || a.num_origins < 1 ||
        a.row_words != 1 + 3 * (a.num_groups * (a.num_groups + 1) / 2 + a.num_groups * a.num_groups))
        return hipErrorInvalidValue;
    const dim3 g((unsigned) std::max(1, std::min((a.n + block_threads - 1) / block_threads, std::max(1, grid_cap))));
    CurrentArgs b = a;
    b.num_slabs = (int32_t) g.x;
    if (b.slabs) hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_current_reduce, true), g, dim3((unsigned) block_threads), 0, s, b);
    else hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_current_reduce, false), g, dim3((unsigned) block_threads), 0, s, b);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long cells = (long long) (a.num_origins + 1) * (a.row_words - 1);
    const dim3 gc((unsigned) std::max<long long>(1, std::min<long long>((cells + 255) / 256, std::max(1, grid_cap))));
    hipLaunchKernelGGL(vv_kernel_current_correlate, gc, dim3(256), 0, s, b);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(vv_kernel_current_advance, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_current_floor(long long* words, hipStream_t s) {
    hipLaunchKernelGGL(vv_kernel_current_floor, dim3(1), dim3(64), 0, s, words);
    return hipGetLastError();
}
hipError_t launch_modes(int precision, const ModesArgs& a, int sites_per_thread, int block_threads, int grid_cap, hipStream_t s) {
    // what the kernels rely on: the planes hold the sites, an item's sites fit its block's registers (the host built the items for this shape)
    if (block_threads < 64 || block_threads > 512 || block_threads % 64) return hipErrorInvalidValue;
    if (a.num_groups < 1 || a.num_groups > MODES_MAX_GROUPS || a.num_modes < 1 || a.n < 0 || a.stride < a.n || a.num_items < 0 || a.num_origins < 0 ||
        (long long) a.row_words != 1 + (long long) a.num_groups * a.num_groups * a.num_modes)
        return hipErrorInvalidValue;
    const dim3 gg((unsigned) std::max(1, std::min((a.n + 255) / 256, std::max(1, grid_cap))));
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_modes_gather), gg, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 gm((unsigned) std::max(1, a.num_items)), bm((unsigned) block_threads);
    switch (sites_per_thread) {
        case 1: hipLaunchKernelGGL(vv_kernel_modes<1>, gm, bm, 0, s, a); break;
        case 2: hipLaunchKernelGGL(vv_kernel_modes<2>, gm, bm, 0, s, a); break;
        case 4: hipLaunchKernelGGL(vv_kernel_modes<4>, gm, bm, 0, s, a); break;
        case 8: hipLaunchKernelGGL(vv_kernel_modes<8>, gm, bm, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const long long cells = (long long) (a.num_origins + 1) * (a.row_words - 1);
    const dim3 gc((unsigned) std::max<long long>(1, std::min<long long>((cells + 255) / 256, std::max(1, grid_cap))));
    hipLaunchKernelGGL(vv_kernel_modes_correlate, gc, dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(vv_kernel_modes_advance, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_modes_floor(long long* words, hipStream_t s) {
    hipLaunchKernelGGL(vv_kernel_modes_floor, dim3(1), dim3(64), 0, s, words);
    return hipGetLastError();
}
hipError_t launch_contacts(int precision, const ContactsArgs& a, int grid_cap, hipStream_t s) {
    // what the kernels rely on: the staged rows fit the block's LDS, the planes hold the sites, the slots are a grid dimension
    if (a.rows_per_tile < 64 || a.rows_per_tile > CONTACTS_MAX_ROWS_PER_TILE || a.rows_per_tile % 64) return hipErrorInvalidValue;
    if (a.n < 0 || a.stride < a.n || a.num_mask_items < 0 || a.num_corr_items < 1 || a.num_origins < 1 || a.num_origins > 1024 ||
        a.num_classes < 1 || a.num_classes > CONTACTS_MAX_CLASSES || a.sample_words % 2)
        return hipErrorInvalidValue;
    const dim3 gg((unsigned) std::max(1, std::min((a.n + 255) / 256, std::max(1, grid_cap))));
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_contacts_gather), gg, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 gm((unsigned) std::max(1, a.num_mask_items));
    const unsigned lds = (unsigned) a.rows_per_tile * (3 * sizeof(double) + sizeof(int)) + sizeof(long long);
    if (a.mol) hipLaunchKernelGGL(vv_kernel_contacts_mask<true>, gm, dim3(256), lds, s, a);
    else hipLaunchKernelGGL(vv_kernel_contacts_mask<false>, gm, dim3(256), lds, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 gc((unsigned) a.num_corr_items, (unsigned) a.num_origins);
    if (a.cont) hipLaunchKernelGGL(vv_kernel_contacts_correlate<true>, gc, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(vv_kernel_contacts_correlate<false>, gc, dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(vv_kernel_contacts_advance, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
template <int MODE, bool GROUPED>
static auto pick_acf(int precision, bool lds) {
    return lds ? VV_PICK(precision, vv_kernel_acf, MODE, GROUPED, true) : VV_PICK(precision, vv_kernel_acf, MODE, GROUPED, false);
}
template <int MODE>
static auto pick_acf(int precision, bool grouped, bool lds) { return grouped ? pick_acf<MODE, true>(precision, lds) : pick_acf<MODE, false>(precision, lds); }
hipError_t launch_acf(int precision, const AcfArgs& a, int mode, int block_threads, int grid_cap, hipStream_t s) {
    if (block_threads < 64 || block_threads > 512 || block_threads % 64) return hipErrorInvalidValue;
    // what the kernel relies on: the ring's columns hold the units, the slots in flight fit its registers, the mode has its tables
    if (a.n < 0 || a.stride < a.n || a.num_origins < 1 || a.slots_in_flight < 1 || a.slots_in_flight > ACF_MAX_SLOTS_IN_FLIGHT) return hipErrorInvalidValue;
    if (mode != ACF_VELOCITY_PARTICLES && mode != ACF_VELOCITY_MOLECULES && mode != ACF_ORIENTATION) return hipErrorInvalidValue;
    if (a.n > 0 && (mode == ACF_VELOCITY_MOLECULES ? !(a.first && a.weight && a.total && a.index) : mode == ACF_ORIENTATION && !a.index)) return hipErrorInvalidValue;
    const dim3 g((unsigned) std::max(1, std::min((a.n + block_threads - 1) / block_threads, std::max(1, grid_cap))));
    const size_t table_bytes = (size_t) a.table_words * sizeof(long long);
    const bool lds = table_bytes <= PROFILE_LDS_BYTES;
    const bool grouped = a.group != nullptr;
    const auto k = mode == ACF_VELOCITY_MOLECULES ? pick_acf<ACF_VELOCITY_MOLECULES>(precision, grouped, lds)
                   : mode == ACF_ORIENTATION      ? pick_acf<ACF_ORIENTATION>(precision, grouped, lds)
                                                  : pick_acf<ACF_VELOCITY_PARTICLES>(precision, grouped, lds);
    hipLaunchKernelGGL(k, g, dim3((unsigned) block_threads), lds ? (unsigned) table_bytes : 0u, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vv_kernel_acf_advance, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_acf_floor(long long* words, hipStream_t s) {
    hipLaunchKernelGGL(vv_kernel_acf_floor, dim3(1), dim3(64), 0, s, words);
    return hipGetLastError();
}
template <bool MOLECULES, bool GROUPED>
static auto pick_vanhove(int precision, bool lds) {
    return lds ? VV_PICK(precision, vv_kernel_vanhove, MOLECULES, GROUPED, true) : VV_PICK(precision, vv_kernel_vanhove, MOLECULES, GROUPED, false);
}
hipError_t launch_vanhove(int precision, const VanHoveArgs& a, int block_threads, int grid_cap, hipStream_t s) {
    if (block_threads < 64 || block_threads > 512 || block_threads % 64) return hipErrorInvalidValue;
    // what the kernel relies on: the ring's columns hold the units, the edges fit its LDS copy, the groups it counts in LDS fit the histogram
    if (a.n < 0 || a.stride < a.n || a.num_origins < 1 || a.num_bins < 1 || a.num_bins > VANHOVE_MAX_BINS || !a.e2) return hipErrorInvalidValue;
    if (a.lds_groups < 0 || (long long) a.lds_groups * a.num_bins > VANHOVE_LDS_WORDS) return hipErrorInvalidValue;
    const dim3 g((unsigned) std::max(1, std::min((a.n + block_threads - 1) / block_threads, std::max(1, grid_cap))));
    const bool lds = a.lds_groups > 0;
    const auto k = a.first ? (a.group ? pick_vanhove<true, true>(precision, lds) : pick_vanhove<true, false>(precision, lds))
                           : (a.group ? pick_vanhove<false, true>(precision, lds) : pick_vanhove<false, false>(precision, lds));
    hipLaunchKernelGGL(k, g, dim3((unsigned) block_threads), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vv_kernel_vanhove_advance, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_vanhove_floor(long long* words, hipStream_t s) {
    hipLaunchKernelGGL(vv_kernel_vanhove_floor, dim3(1), dim3(64), 0, s, words);
    return hipGetLastError();
}
hipError_t launch_vhd(int precision, const VhdArgs& a, bool lds_hist, int grid_cap, hipStream_t s) {
    // what the kernels rely on: a private word cannot wrap, the histograms fit the block's LDS, the planes hold the sites, the grid's y
    // extent holds the ring's slots
    if (a.max_jsites < 1 || (long long) a.max_jsites * RDF_TILE >= (1ll << 32)) return hipErrorInvalidValue;
    if (a.nbins < 1 || a.copies < 1 || a.copies > RDF_TILE / 64 || rdf_lds_bytes(a.nbins, a.copies) > PROFILE_LDS_BYTES) return hipErrorInvalidValue;
    if (a.n < 0 || a.stride < a.n || a.num_items < 0 || !a.ring) return hipErrorInvalidValue;
    if (a.origin_every < 1 || a.num_lags < 1 || a.num_origins < 1 || a.num_origins > 1024 || (long long) a.num_origins * a.origin_every < a.num_lags) return hipErrorInvalidValue;
    const dim3 gg((unsigned) std::max(1, std::min((a.n + 255) / 256, std::max(1, grid_cap))));
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_vhd_gather), gg, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 gp((unsigned) std::max(1, a.num_items), (unsigned) (a.num_origins + 1));
    const unsigned lds = (unsigned) rdf_lds_bytes(lds_hist ? a.nbins : 0, a.copies);
    if (a.mol) {
        if (lds_hist) hipLaunchKernelGGL((vv_kernel_vhd_pairs<true, false>), gp, dim3(RDF_TILE), lds, s, a);
        else hipLaunchKernelGGL((vv_kernel_vhd_pairs<true, true>), gp, dim3(RDF_TILE), lds, s, a);
    } else {
        if (lds_hist) hipLaunchKernelGGL((vv_kernel_vhd_pairs<false, false>), gp, dim3(RDF_TILE), lds, s, a);
        else hipLaunchKernelGGL((vv_kernel_vhd_pairs<false, true>), gp, dim3(RDF_TILE), lds, s, a);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(vv_kernel_vhd_advance, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_vhd_floor(long long* words, hipStream_t s) {
    hipLaunchKernelGGL(vv_kernel_vhd_floor, dim3(1), dim3(64), 0, s, words);
    return hipGetLastError();
}
hipError_t launch_sdf(int precision, const SdfArgs& a, int grid_cap, hipStream_t s) {
    // what the kernels rely on: the planes hold the sites and the frames, a voxel index stays inside the table's class
    if (a.nbins < 1 || a.nbins > SDF_MAX_BINS || a.max_jsites < 1) return hipErrorInvalidValue;
    if (a.n < 0 || a.stride < a.n || a.nf < 0 || a.fstride < a.nf || a.num_items < 0 || !a.scratch) return hipErrorInvalidValue;
    const long long threads = (long long) a.n + a.nf;
    const dim3 gg((unsigned) std::max<long long>(1, std::min<long long>((threads + 255) / 256, std::max(1, grid_cap))));
    hipLaunchKernelGGL(VV_PICK(precision, vv_kernel_sdf_gather), gg, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 gp((unsigned) std::max(1, a.num_items));
    const unsigned lds = (unsigned) rdf_lds_bytes(0, 0);      // (the staged j-tile alone)
    if (a.mol) hipLaunchKernelGGL(vv_kernel_sdf_pairs<true>, gp, dim3(RDF_TILE), lds, s, a);
    else hipLaunchKernelGGL(vv_kernel_sdf_pairs<false>, gp, dim3(RDF_TILE), lds, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(vv_kernel_sdf_advance, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
#endif      // VV_KERNELS_PART != 2

}  // namespace vv
