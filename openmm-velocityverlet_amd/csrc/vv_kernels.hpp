// vv_kernels.hpp -- launch entry points of the HIP kernels (gfx950).
// Device code lives in vv_device.inc (compiled through vv_kernels.hip); the C ABI (vv_api.cpp) only sees this header.
#pragma once
#include <atomic>
#include "vv_args.hpp"
#include "vv_host.hpp"

namespace vv {

inline PeriodicArgs periodic_args(const PeriodicLayout& q) {
    PeriodicArgs r{};
    r.magic = q.magic; r.wpc = q.wpc; r.apc = q.apc; r.spc = q.spc;
    for (int k = 0; k < 4; k++) {
        const bool used = k < q.nreg;
        r.wave_start[k] = used ? q.reg_wave_start[k] : 0x7fffffff;
        auto inc = [&](const int32_t* v) { return !used ? 0 : (k == 0 ? v[0] : v[k] - v[k - 1]); };
        r.d_wave[k] = inc(q.reg_wave_start); r.d_atom_start[k] = inc(q.reg_atom_start); r.d_atom_end[k] = inc(q.reg_atom_end);
        r.d_seg[k] = inc(q.reg_seg_start); r.d_P[k] = inc(q.reg_P); r.d_spw[k] = inc(q.reg_spw);
    }
    return r;
}

// launchers (precision = VVHIP_SINGLE / MIXED / DOUBLE); return hipError_t of the launch
// block_threads = 64 x tile waves per block; grid_cap = most blocks to launch (the kernels stride over tiles beyond that)
// ev0 / ev1 (optional): events that receive the dispatch's own begin / end timestamps (timing runs; never inside a graph capture)
// route (optional): which kernel the launch took -- ROUTE_COMPILED (a specialisation of the library), ROUTE_RUNTIME (hipRTC),
// ROUTE_GENERIC (run-time stage bits) -- so that the caller can count per plan (several host threads may drive plans of their own)
enum LaunchRoute { ROUTE_COMPILED = 0, ROUTE_RUNTIME = 1, ROUTE_GENERIC = 2 };
hipError_t launch_a(int precision, const KArgs& a, int block_threads, int grid_cap, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, int* route = nullptr);
hipError_t launch_b(int precision, const KArgs& a, int block_threads, int grid_cap, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, int* route = nullptr);
// The fused step: kernel A's stage set a.flags_a and kernel B's a.flags in one launch of vv_kernel_b<.., SFA> over `rendezvous` (an uncached
// [NUM_ACC][ACC_SLOTS] array of 8-byte words); block_threads = 64 x tile waves per block, one pass.  blocks_per_cu != nullptr: only report the
// kernel's occupancy (blocks of this shape per CU).  hipErrorNotSupported: no kernel for the pair, or a shape the rendezvous cannot take.
hipError_t launch_fused(int precision, const KArgs& a, int block_threads, const unsigned long long* rendezvous, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr,
                        int* route = nullptr, int* blocks_per_cu = nullptr);
hipError_t launch_chain(const NHConst& c, NHDevState* st, unsigned long long* acc, hipStream_t s);
hipError_t launch_tether(int precision, const TetherArgs& t, int block_threads, hipStream_t s, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
// Fills the static per-lane mass tables from the inverse masses in velm.w (once per binding; see A_MTAB / B_MTAB).
hipError_t launch_mass_table(int precision, const void* velm, const int2* slots, int nwaves, double* slot_m, double* slot_f, hipStream_t s);
// whether the specialised kernels A (kernel = 0) / B (1) of this build were compiled with the mass tables (they then carry A_MTAB /
// B_MTAB in their stage sets)
bool sf_kernels_use_mass_table(int kernel);
// Device Gaussian generator (stand-alone hosts; inside OpenMM the random buffer is OpenMM's): Philox4x32-10 keyed by
// `seed`, counter = (*epoch, element index); a second 1-thread launch bumps *epoch so that graph replays draw fresh numbers.
hipError_t launch_fill_normals(float4* out, uint32_t count, uint64_t seed, unsigned long long* epoch, hipStream_t s);
hipError_t launch_image_pairs(int precision, void* posq, void* corr, const int2* pairs, int npairs, double mirror,
                              hipStream_t s);
// The Drude temperature report's two passes (vv_dev_report.inc) over a.nwaves waves and a.nmol + a.ncross items: blocks of block_threads,
// at most grid_cap of them per pass (the kernels stride beyond).  a.mol_p and a.out must be zero on entry.
hipError_t launch_report(int precision, const ReportArgs& a, int block_threads, int grid_cap, hipStream_t s);
// One series row (vv_dev_report.inc: vv_kernel_series_append) behind the report's passes (or alone: a.rep_out null).
hipError_t launch_series_append(const SeriesArgs& a, int grid_cap, hipStream_t s);
// Removal of the centre-of-mass velocity (vv_dev_cmm.inc): the sum kernel, then the subtract kernel, over a.rep.nwaves waves in blocks of
// block_threads, at most grid_cap of them (the kernels stride beyond).  a.words must be zero on entry and is zero again afterwards.
hipError_t launch_cm_motion(int precision, const CmmArgs& a, int block_threads, int grid_cap, hipStream_t s);
// Monte Carlo barostat (vv_dev_barostat.inc): the sum kernel, then the shift kernel, over a.nwaves waves and a.nlaneless listed particles in
// blocks of block_threads, at most grid_cap of them (the kernels stride beyond).  a.words must be zero on entry.
hipError_t launch_barostat(int precision, const BarostatArgs& a, int block_threads, int grid_cap, hipStream_t s);
// Maxwell-Boltzmann start velocities (vv_dev_thermalize.inc): one kernel over a.nwaves waves and a.nlaneless listed particles in blocks of
// 512 threads, at most grid_cap of them (the kernel strides beyond).
hipError_t launch_thermalize(int precision, const ThermalizeArgs& a, int grid_cap, hipStream_t s);
// State digest (vv_dev_digest.inc): one streaming reduction over a.nwords words in blocks of block_threads (a multiple of 64, at most 512),
// at most grid_cap of them (the kernel strides beyond), added to *a.out.
hipError_t launch_digest(const DigestArgs& a, int block_threads, int grid_cap, hipStream_t s);
// One trajectory frame (vv_dev_frames.inc): the streaming kernel over a.n recorded particles in blocks of 512 threads, at most grid_cap of
// them (the kernel strides beyond; one idle block where a.n = 0), then the one-thread kernel that writes the header and advances the
// cursor.  float64: components as double instead of float.
hipError_t launch_frame(int precision, const FrameArgs& a, bool float64, int grid_cap, hipStream_t s);
// One profile sample (vv_dev_profile.inc): the accumulating kernel over a.n recorded particles in blocks of 512 threads, at most grid_cap
// of them (the kernel strides beyond; one idle block where a.n = 0), then the one-thread kernel that counts the sample.  A table of at
// most PROFILE_LDS_BYTES is accumulated per block in LDS first, a larger one by global atomics directly; a.group selects the grouped kernels.
constexpr size_t PROFILE_LDS_BYTES = 64 * 1024;
hipError_t launch_profile(int precision, const ProfileArgs& a, int grid_cap, hipStream_t s);
// One MSD sample (vv_dev_msd.inc): the accumulating kernel over a.n units in blocks of block_threads threads (64 .. 512, a multiple of
// 64), at most grid_cap of them (the kernel strides beyond; one idle block where a.n = 0), then the one-thread kernel that counts the sample.  A table of at most PROFILE_LDS_BYTES is
// accumulated per block in LDS first, a larger one by global atomics directly; a.first selects the molecule kernels, a.group the grouped ones.
hipError_t launch_msd(int precision, const MsdArgs& a, int block_threads, int grid_cap, hipStream_t s);
// The origin floor becomes the current sample ordinal (one thread, in the stream): words as MsdArgs::words.
hipError_t launch_msd_floor(long long* words, hipStream_t s);
// One RDF sample (vv_dev_rdf.inc): the gather over a.n sites in blocks of 256 threads, at most grid_cap of them (the kernel strides
// beyond), the pair kernel with one block of RDF_TILE threads per work item (one idle block where there is none) and dynamic LDS of
// rdf_lds_bytes (the staged j-tile and a.copies private histograms, 1 .. RDF_TILE / 64, within PROFILE_LDS_BYTES), then the one-thread
// kernel that counts the sample.  a.mol selects the kernel that leaves out pairs of one molecule.  hipErrorInvalidValue where
// a.max_jsites * RDF_TILE >= 2^32: a block's private 32-bit words could wrap.
size_t rdf_lds_bytes(int nbins, int copies);
hipError_t launch_rdf(int precision, const RdfArgs& a, int grid_cap, hipStream_t s);
// One current sample (vv_dev_current.inc): the reduce over a.n recorded particles in blocks of block_threads threads (64 .. 512, a multiple
// of 64), at most grid_cap of them (the kernel strides beyond; one idle block where a.n = 0), the correlate kernel with one thread per
// (ring slot or zero lag, class, component) in blocks of 256, then the one-wave kernel that stores the origin and counts the sample.
// a.slabs selects the two-level form: it must hold (a.n + 63) / 64 + 1 slabs of a.num_groups * 6 + 1 words (no launch has more blocks).
hipError_t launch_current(int precision, const CurrentArgs& a, int block_threads, int grid_cap, hipStream_t s);
// The origin floor becomes the current sample ordinal (one thread, in the stream): words as CurrentArgs::words.
hipError_t launch_current_floor(long long* words, hipStream_t s);
// One density-mode sample (vv_dev_modes.inc): the gather over a.n sites in blocks of 256, at most grid_cap of them; the mode kernel with one
// block of block_threads threads (64 .. 512, a multiple of 64) and sites_per_thread (1, 2, 4, 8) sites per thread for each of a.num_items
// work items (one idle block where there is none) -- the items must have been built for this shape: no item has more than block_threads *
// sites_per_thread sites or MODES_MAX_K_TILE modes --; the correlate kernel with one thread per (ring slot or zero lag, g, h, k) in blocks
// of 256, at most grid_cap; then the one-wave kernel that stores the origin and counts the sample.
hipError_t launch_modes(int precision, const ModesArgs& a, int sites_per_thread, int block_threads, int grid_cap, hipStream_t s);
// The origin floor becomes the current sample ordinal (one thread, in the stream): words as ModesArgs::words.
hipError_t launch_modes_floor(long long* words, hipStream_t s);
// One contact sample (vv_dev_contacts.inc): the gather over a.n sites in blocks of 256, at most grid_cap of them; the mask kernel with one
// block of 256 threads per work item (one idle block where there is none) and dynamic LDS for a.rows_per_tile staged rows (a multiple of 64,
// at most CONTACTS_MAX_ROWS_PER_TILE) -- the items must have been built for that tile --; the correlate kernel with one block of 256 per
// (work item, slot of the ring); then the one-wave kernel that writes the slot's ordinal and counts the sample.  a.mol selects the mask
// kernel that clears pairs of one molecule, a.cont the correlate kernel that keeps the surviving contacts.
hipError_t launch_contacts(int precision, const ContactsArgs& a, int grid_cap, hipStream_t s);
// One autocorrelation sample (vv_dev_acf.inc): the accumulating kernel over a.n units in blocks of block_threads (64 .. 512, a multiple of
// 64), at most grid_cap of them, then the one-thread kernel that advances the sample ordinal.  mode (ACF_*) and a.group select the kernel;
// a table of at most PROFILE_LDS_BYTES is accumulated per block in LDS.
hipError_t launch_acf(int precision, const AcfArgs& a, int mode, int block_threads, int grid_cap, hipStream_t s);
// The origin floor becomes the current sample ordinal (one thread, in the stream): words as AcfArgs::words.
hipError_t launch_acf_floor(long long* words, hipStream_t s);
// One self van Hove sample (vv_dev_vanhove.inc): the accumulating kernel over a.n units in blocks of block_threads (64 .. 512, a multiple
// of 64), at most grid_cap of them, then the one-thread kernel that advances the sample ordinal.  a.first and a.group select the kernel;
// a.lds_groups > 0 the one that counts in a block-private LDS histogram (lds_groups * num_bins <= VANHOVE_LDS_WORDS), 0 the plain one.
hipError_t launch_vanhove(int precision, const VanHoveArgs& a, int block_threads, int grid_cap, hipStream_t s);
// The origin floor becomes the current sample ordinal (one thread, in the stream): words as VanHoveArgs::words.
hipError_t launch_vanhove_floor(long long* words, hipStream_t s);
// One distinct van Hove sample (vv_dev_vanhove_distinct.inc): the gather over a.n sites in blocks of 256 threads, at most grid_cap of them,
// into the plane set of "now"; the pair kernel with one block of RDF_TILE threads per (work item, ring slot), grid (items, num_origins + 1),
// and dynamic LDS of rdf_lds_bytes (lds_hist: the staged j-tile and a.copies private histograms; else the tile alone and every pair a global
// add); then the one-thread kernel that counts the visits and advances the ordinal.  hipErrorInvalidValue where a.max_jsites * RDF_TILE >=
// 2^32 or the ring has fewer slots than the lags need.
hipError_t launch_vhd(int precision, const VhdArgs& a, bool lds_hist, int grid_cap, hipStream_t s);
// The origin floor becomes the current sample ordinal (one thread, in the stream): words as VhdArgs::words.
hipError_t launch_vhd_floor(long long* words, hipStream_t s);
// One spatial distribution sample (vv_dev_sdf.inc): the gather over a.n sites and a.nf frames in blocks of 256 threads, at most grid_cap
// of them (the kernel strides beyond), the pair kernel with one block of RDF_TILE threads per work item (one idle block where there is
// none) and dynamic LDS for the staged j-tile, then the one-thread kernel that counts the sample.  Every in-range pair is an agent-scope
// add to the int64 table: no private histogram, nothing that could wrap.
hipError_t launch_sdf(int precision, const SdfArgs& a, int grid_cap, hipStream_t s);

}  // namespace vv
