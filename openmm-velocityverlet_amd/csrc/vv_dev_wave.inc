// vv_dev_wave.inc -- part of vv_device.inc: precision traits, DPP scans and reductions, fixed-point block sums, cos(kz)
template <class T> struct Vec;
template <> struct Vec<float> { using v4 = float4; using v3 = float3; };
template <> struct Vec<double> { using v4 = double4; using v3 = double3; };

// What OpenMM's context prepends to the reference kernels (assumption stated in oracle/ref_prelude.h):
// single-precision sqrt/recip literals unless the `real` type is double.
template <class real> struct Prec;
template <> struct Prec<float> {
    template <class T> static __device__ __forceinline__ float SQRT(T x) { return sqrtf((float) x); }
    static __device__ __forceinline__ float RECIP(float x) { return 1.0f / x; }
    static __device__ __forceinline__ double RECIP(double x) { return 1.0f / x; }
    // Reciprocal for quantities that only feed REDUCTIONS (kinetic-energy sums, molecular COM): hardware estimate (24 bits) + two Newton
    // steps, within 1 ulp of the IEEE quotient (equal to it in 2^20 random samples, tools/probes/rcp_probe.cpp).  Those sums already depend on the summation order at that level, so nothing that is compared
    // bit for bit with the oracle (kick, drift, hard wall, scaling arithmetic) goes through this; an IEEE fp64 division
    // costs 14 instructions, this 5, on a kernel that is issue-bound at the headline size.
    static __device__ __forceinline__ float RECIP_SUM(float x) { return __builtin_amdgcn_rcpf(x); }
    static __device__ __forceinline__ double RECIP_SUM(double x) { double r = __builtin_amdgcn_rcp(x); r = fma(fma(-x, r, 1.0), r, r); return fma(fma(-x, r, 1.0), r, r); }
};
template <> struct Prec<double> {
    static __device__ __forceinline__ double SQRT(double x) { return sqrt(x); }
    static __device__ __forceinline__ double RECIP(double x) { return 1.0 / x; }
    static __device__ __forceinline__ double RECIP_SUM(double x) { double r = __builtin_amdgcn_rcp(x); r = fma(fma(-x, r, 1.0), r, r); return fma(fma(-x, r, 1.0), r, r); }
};

// Reciprocal and reciprocal square root for the constraint solvers' own arithmetic (not the reference's): hardware estimate + two Newton steps in
// double (within 1 ulp; 5 and 9 instructions against the 14 of an IEEE fp64 division and the ~25 of one behind a correctly rounded square root);
// the IEEE operations in float, where they are cheap and the estimates have no Newton headroom.
__device__ __forceinline__ double recip_nr(double x) { double r = __builtin_amdgcn_rcp(x); r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r); return __builtin_fma(__builtin_fma(-x, r, 1.0), r, r); }
__device__ __forceinline__ float recip_nr(float x) { return 1.0f / x; }
__device__ __forceinline__ double rsqrt_nr(double x) {
    double r = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
    r = __builtin_fma(__builtin_fma(-h * r, r, 0.5), r, r);      // r (1.5 - h r^2)
    return __builtin_fma(__builtin_fma(-h * r, r, 0.5), r, r);
}
__device__ __forceinline__ float rsqrt_nr(float x) { return 1.0f / sqrtf(x); }
// square root by the same route (x * rsqrt; 0 for x <= 0, which an exactly degenerate triangle would produce): 10 instructions against ~18
__device__ __forceinline__ double sqrt_nr(double x) { return x > 0 ? x * rsqrt_nr(x) : 0.0; }
__device__ __forceinline__ float sqrt_nr(float x) { return sqrtf(x); }
template <class V>
__device__ __forceinline__ void store_vec(V* base, int index, const V& val) {
    base[index] = val;
}

__device__ __forceinline__ float shfl(float x, int src) { return __shfl(x, src, 64); }
__device__ __forceinline__ double shfl(double x, int src) { return __shfl(x, src, 64); }

// ---- wave-wide inclusive prefix sum on the DPP network (no LDS round trips): Hillis-Steele inside each 16-lane
// row (row_shr 1,2,4,8; lanes without a source add 0), then row 0 -> row 1 / row 2 -> row 3 (row_bcast:15) and
// rows 0+1 -> rows 2,3 (row_bcast:31).  Lane 63 ends up with the wave total.
// ROW_MASK 0xF with bound_ctrl writes EVERY lane (lanes without a source read 0), so the destination needs no initial value:
// __builtin_amdgcn_mov_dpp.  The two row_bcast steps write only some rows; there the unwritten lanes must read 0, which costs a
// zeroing move per 32-bit half (update_dpp with old = 0).  Using update_dpp everywhere, as round 1 did, put those moves into all
// 6 steps of every scan (24 instructions per 64-bit scan instead of 20).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_fetch32(int v) {
    if (ROW_MASK == 0xF) return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true);
    return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, true);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_fetch(double x) {
    const int lo = dpp_fetch32<CTRL, ROW_MASK>(__double2loint(x));
    const int hi = dpp_fetch32<CTRL, ROW_MASK>(__double2hiint(x));
    return __hiloint2double(hi, lo);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_fetch(float x) {
    return __int_as_float(dpp_fetch32<CTRL, ROW_MASK>(__float_as_int(x)));
}

// Arithmetic layout (vv_host.hpp: PeriodicLayout): everything a lane used to read from its slot words, from the wave index alone.
struct PeriodicWave {
    int atom0, count, region, seg0;
};
__device__ __forceinline__ PeriodicWave periodic_wave(const PeriodicArgs& q, int wave_uniform) {
    const int w = __builtin_amdgcn_readfirstlane(wave_uniform);
    const int cell = (int) __umulhi((unsigned) w, q.magic);                 // = w / wpc (checked for every wave by analyze()); 0 for one cell
    const int wl = w - cell * q.wpc;
    int ws = q.d_wave[0], as = q.d_atom_start[0], ae = q.d_atom_end[0], ss = q.d_seg[0], P = q.d_P[0], spw = q.d_spw[0], region = 0;
#pragma unroll
    for (int k = 1; k < 4; k++) {
        const bool in = wl >= q.wave_start[k];
        region += in ? 1 : 0;
        ws += in ? q.d_wave[k] : 0; as += in ? q.d_atom_start[k] : 0; ae += in ? q.d_atom_end[k] : 0;
        ss += in ? q.d_seg[k] : 0; P += in ? q.d_P[k] : 0; spw += in ? q.d_spw[k] : 0;
    }
    const int wr = wl - ws, a0 = as + wr * P;
    PeriodicWave r;
    r.atom0 = cell * q.apc + a0;
    r.count = min(P, ae - a0);
    r.region = region;
    r.seg0 = cell * q.spc + ss + wr * spw;
    return r;
}

// number of set bits of a 64-lane mask below the calling lane
__device__ __forceinline__ unsigned lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned) (mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) mask, 0u));
}

template <class T>
__device__ __forceinline__ T wave_scan(T x) {
    x += dpp_fetch<0x111, 0xF>(x);   // row_shr:1
    x += dpp_fetch<0x112, 0xF>(x);   // row_shr:2
    x += dpp_fetch<0x114, 0xF>(x);   // row_shr:4
    x += dpp_fetch<0x118, 0xF>(x);   // row_shr:8
    x += dpp_fetch<0x142, 0xA>(x);   // row_bcast:15 into rows 1 and 3
    x += dpp_fetch<0x143, 0xC>(x);   // row_bcast:31 into rows 2 and 3
    return x;
}
// Three independent scans, step by step side by side: the compiler keeps the order of the source, and a DPP read needs two wait
// states after the VALU write of its source -- alone, every step of a scan is followed by an s_nop and a dependent add; three
// interleaved scans fill each other's gaps.
template <class T>
__device__ __forceinline__ void wave_scan3(T& x, T& y, T& z) {
#define VV_SCAN_STEP(CTRL, MASK) { const T dx_ = dpp_fetch<CTRL, MASK>(x), dy_ = dpp_fetch<CTRL, MASK>(y), dz_ = dpp_fetch<CTRL, MASK>(z); x += dx_; y += dy_; z += dz_; }
    VV_SCAN_STEP(0x111, 0xF) VV_SCAN_STEP(0x112, 0xF) VV_SCAN_STEP(0x114, 0xF) VV_SCAN_STEP(0x118, 0xF) VV_SCAN_STEP(0x142, 0xA) VV_SCAN_STEP(0x143, 0xC)
#undef VV_SCAN_STEP
}
// total of a wave in lane 63
__device__ __forceinline__ double wave_sum(double x) { return wave_scan(x); }

// FOUR wave totals for the price of one.  v_permlane32_swap / v_permlane16_swap (new in gfx950) exchange half-waves / neighbouring
// rows BETWEEN two registers: after a swap, x' + y' holds, in one half (row), the pairwise sums of x and in the other those of y.  Two
// such steps fold four 64-lane quantities into one register whose row r carries quantity r, and four DPP shifts inside the rows finish:
// 6 swaps + 8 DPP moves + 7 additions for four quantities, against (12 DPP moves + 6 additions) for EACH with the scan above
// (tools/probes/permswap_probe.cpp shows the lane mapping).  Result: lane 15 holds the total of a, lane 31 of b, 47 of c, 63 of d.
__device__ __forceinline__ void lane_swap32(double& x, double& y) {
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned) __double2loint(x), (unsigned) __double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned) __double2hiint(x), (unsigned) __double2hiint(y), false, false);
    x = __hiloint2double((int) hi[0], (int) lo[0]); y = __hiloint2double((int) hi[1], (int) lo[1]);
}
__device__ __forceinline__ void lane_swap16(double& x, double& y) {
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned) __double2loint(x), (unsigned) __double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned) __double2hiint(x), (unsigned) __double2hiint(y), false, false);
    x = __hiloint2double((int) hi[0], (int) lo[0]); y = __hiloint2double((int) hi[1], (int) lo[1]);
}
__device__ __forceinline__ void lane_swap32(long long& x, long long& y) {
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned) x, (unsigned) y, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned) ((unsigned long long) x >> 32), (unsigned) ((unsigned long long) y >> 32), false, false);
    x = (long long) (((unsigned long long) hi[0] << 32) | lo[0]); y = (long long) (((unsigned long long) hi[1] << 32) | lo[1]);
}
__device__ __forceinline__ void lane_swap16(long long& x, long long& y) {
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned) x, (unsigned) y, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned) ((unsigned long long) x >> 32), (unsigned) ((unsigned long long) y >> 32), false, false);
    x = (long long) (((unsigned long long) hi[0] << 32) | lo[0]); y = (long long) (((unsigned long long) hi[1] << 32) | lo[1]);
}
template <class T>
__device__ __forceinline__ T wave_reduce4_rows(T a, T b, T c, T d) {
    lane_swap32(a, c); T ac = a + c;        // lanes 0-31: a over the half-wave pairs, lanes 32-63: c
    lane_swap32(b, d); T bd = b + d;        // ... b, d
    lane_swap16(ac, bd);
    return ac + bd;                         // row 0: a, row 1: b, row 2: c, row 3: d -- 16 partial sums each
}
__device__ __forceinline__ double wave_reduce4(double a, double b, double c, double d) {
    double t = wave_reduce4_rows(a, b, c, d);
    t += dpp_fetch<0x111, 0xF>(t);   // row_shr:1, 2, 4, 8: the row's total in its last lane
    t += dpp_fetch<0x112, 0xF>(t);
    t += dpp_fetch<0x114, 0xF>(t);
    t += dpp_fetch<0x118, 0xF>(t);
    return t;
}

// Up to three such reductions side by side (the cos perturbation has ten quantities to sum: 4 + 4 + 2).  One after the other, every step
// of a reduction waits for the one before it -- lane swaps and DPP moves are dependent chains with wait states, ~0.2 us per round at
// the end of kernel A, where the whole block then waits at a barrier (round 4, in-kernel stamps: C4's kernel A spent 1.1 us between
// its last tile and that barrier against 0.67 us for C3's single round).  Written step by step across the groups, the rounds fill
// each other's gaps, as the three momentum scans do (wave_scan3).  `on[g]` false: group g is skipped (compile-time in the
// specialised kernels).  Result as wave_reduce4: lane 16 r + 15 of t[g] holds the total of quantity r of group g.
template <int G>
__device__ __forceinline__ void wave_reduce4_groups(const double (&v)[G][4], const bool (&on)[G], double (&t)[G]) {
    double a[G], b[G], c[G], d[G], ac[G], bd[G];
#pragma unroll
    for (int g = 0; g < G; g++) { a[g] = v[g][0]; b[g] = v[g][1]; c[g] = v[g][2]; d[g] = v[g][3]; ac[g] = bd[g] = t[g] = 0; }
#pragma unroll
    for (int g = 0; g < G; g++) if (on[g]) { lane_swap32(a[g], c[g]); lane_swap32(b[g], d[g]); }
#pragma unroll
    for (int g = 0; g < G; g++) if (on[g]) { ac[g] = a[g] + c[g]; bd[g] = b[g] + d[g]; }
#pragma unroll
    for (int g = 0; g < G; g++) if (on[g]) lane_swap16(ac[g], bd[g]);
#pragma unroll
    for (int g = 0; g < G; g++) if (on[g]) t[g] = ac[g] + bd[g];
#define VV_RED_STEP(CTRL) { double f_[G]; _Pragma("unroll") for (int g = 0; g < G; g++) f_[g] = on[g] ? dpp_fetch<CTRL, 0xF>(t[g]) : 0.0; _Pragma("unroll") for (int g = 0; g < G; g++) if (on[g]) t[g] += f_[g]; }
    VV_RED_STEP(0x111) VV_RED_STEP(0x112) VV_RED_STEP(0x114) VV_RED_STEP(0x118)
#undef VV_RED_STEP
}

// Total of the contiguous lane segment [first, last] for every lane of it: P[last] - P[first-1] on the wave prefix sum.
// (The prefix runs over at most 64 particles, so the subtraction costs < 3 bits; the reference itself sums serially.)
template <class T>
__device__ __forceinline__ T segment_total(T x, int lane, int first, int last) {
    const T P = wave_scan(x);
    const T hi = shfl(P, last);
    const T lo = shfl(P, first > 0 ? first - 1 : 0);
    return first > 0 ? hi - lo : hi;
}

// Block partials -> fixed-point atomics.  vals[k] is the calling thread's contribution.
// First half: the wave's totals of the enabled quantities into row `w` of the block's LDS table (the caller meets the block at a barrier).
template <int NV>
__device__ __forceinline__ void wave_partials_to_lds(const double (&vals)[NV], const bool (&enabled)[NV], double (*red)[NV], int w, int lane) {
    // four quantities per wave reduction, the (up to three) groups of four side by side (wave_reduce4_groups): the kinetic-energy sums and
    // the bias moment, then the cos moments
    constexpr int G = (NV + 3) / 4;
    double v[G][4], t[G];
    bool on[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        on[g] = false;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = 4 * g + i;
            v[g][i] = k < NV ? vals[k < NV ? k : 0] : 0.0;
            on[g] = on[g] || (k < NV && enabled[k < NV ? k : 0]);      // compile-time in the specialised kernels
        }
    }
    wave_reduce4_groups<G>(v, on, t);
#pragma unroll
    for (int g = 0; g < G; g++)
        if (on[g] && (lane & 15) == 15 && 4 * g + (lane >> 4) < NV) red[w][4 * g + (lane >> 4)] = t[g];
}
// Second half, behind the barrier: thread k (k < NV, quantity enabled) adds the nw waves' partials of quantity k in wave order, scales
// and rounds to fixed point.  Nothing here may index `enabled` or `scale` by the thread id: both live in constant / kernel
// argument memory, and a lane-indexed read of those turns into a global load in front of the atomic -- two dependent memory
// round trips at the very end of every block (seen in the ISA; ~0.5 us of kernel A's tail).  Bit mask and select chain instead.
// `blocks`: one block may contribute 2^62 / blocks (the int64 total over all blocks -- and ranks <= 16 with 1024x headroom in the
// scale -- cannot wrap unnoticed); a block beyond that (or a NaN) raises the sticky flag in host memory instead of feeding the
// thermostat garbage (vvhip_synchronize / the run loops return VVHIP_ERR_OVERFLOW).
template <int NV>
__device__ __forceinline__ bool block_quantity_enabled(const bool (&enabled)[NV], int k) {
    unsigned mask = 0;
#pragma unroll
    for (int i = 0; i < NV; i++) mask |= enabled[i] ? (1u << i) : 0u;
    return k < NV && ((mask >> k) & 1u);
}
template <int NV>
__device__ __forceinline__ double block_quantity_scale(const bool (&enabled)[NV], const double* scale, int k) {
    double sc = 0;
#pragma unroll
    for (int i = 0; i < NV; i++)
        if (enabled[i] && k == i) sc = scale[i];
    return sc;
}
template <int NV>
__device__ __forceinline__ long long block_fixed_point_sum(const double (*red)[NV], int nw, int k, double sc, unsigned int* status, double blocks) {
    // (all waves' partials requested at once: a loop with a run-time trip count reads them one LDS round trip after the other,
    // at the very end of the kernel; blocks have at most 8 waves, launch_bounds(512))
    double part[8];
#pragma unroll
    for (int i = 0; i < 8; i++) part[i] = red[i < nw ? i : 0][k];
    double s = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) s += i < nw ? part[i] : 0.0;
    const double scaled = s * sc;
    if (__builtin_expect(!(fabs(scaled) * blocks < 4611686018427387904.0), 0) && status)
        __hip_atomic_store(&status[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return __double2ll_rn(scaled);
}
// ... where the caller has zeroed the rows of the waves the block does not have (the one-launch step's thermostat wave does, at the kernel's head):
// eight unconditional reads and additions -- x + 0.0 is what the select above adds for a missing wave, so the sum has the same bits -- without the
// sixteen selects and eight scalar comparisons in front of the publish, on the critical path of every block.
template <int NV>
__device__ __forceinline__ long long block_fixed_point_sum_padded(const double (*red)[NV], int k, double sc, unsigned int* status, double blocks) {
    double part[8];
#pragma unroll
    for (int i = 0; i < 8; i++) part[i] = red[i][k];
    double s = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) s += part[i];
    double scaled = s * sc;
    if (__builtin_expect(!(fabs(scaled) * blocks < 4611686018427387904.0), 0)) {
        if (status) __hip_atomic_store(&status[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        scaled = 0;          // (the run is void -- the flag says so --, and a sum beyond the payload's 58 bits would run into the word's tag: the rendezvous must still complete)
    }
    return __double2ll_rn(scaled);
}
template <int NV>
__device__ __forceinline__ void block_accumulate(const double (&vals)[NV], const bool (&enabled)[NV],
                                                 unsigned long long* acc, const double* scale, unsigned int* status, bool exclusive, unsigned long long acc_old) {
    __shared__ double red[16][NV];

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    wave_partials_to_lds<NV>(vals, enabled, red, w, lane);
    __syncthreads();
    if (block_quantity_enabled<NV>(enabled, (int) threadIdx.x)) {
        const long long q = block_fixed_point_sum<NV>(red, nw, (int) threadIdx.x, block_quantity_scale<NV>(enabled, scale, (int) threadIdx.x), status, (double) gridDim.x);
        // `exclusive`: the launch has at most ACC_SLOTS blocks, so this block is the only one that touches its slot: the slot's old
        // content (requested at the kernel's top) plus q goes back as a plain store.  An agent-scope atomic of this multi-XCD part is
        // executed at the memory side, and the kernel cannot end before it has come back.
        if (exclusive) { if (q != 0) acc[threadIdx.x * ACC_SLOTS + (blockIdx.x & (ACC_SLOTS - 1))] = acc_old + (unsigned long long) q; }
        else if (q != 0) atomicAdd(&acc[threadIdx.x * ACC_SLOTS + (blockIdx.x & (ACC_SLOTS - 1))], (unsigned long long) q);
    }
}

// Sum of the ACC_SLOTS slots of quantity k (exact integer sum), computed cooperatively by one wave (DPP prefix sum,
// total taken from lane 63).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ long long dpp_fetch_i64(long long x) {
    const int lo = dpp_fetch32<CTRL, ROW_MASK>((int) (x & 0xFFFFFFFFll));
    const int hi = dpp_fetch32<CTRL, ROW_MASK>((int) (x >> 32));
    return ((long long) hi << 32) | (unsigned int) lo;
}
__device__ __forceinline__ long long acc_reduce_lane_sum(long long s);
// ... of values the caller has already loaded (kernel B's thermostat wave issues all its loads first)
__device__ __forceinline__ long long acc_reduce(const long long (&raw)[ACC_SLOTS / 64]) {
    long long s = 0;
#pragma unroll
    for (int j = 0; j < ACC_SLOTS / 64; j++) s += raw[j];
    return acc_reduce_lane_sum(s);
}
__device__ __forceinline__ long long acc_total(const unsigned long long* acc, int k, int lane) {
    long long s = 0;
#pragma unroll
    for (int j = 0; j < ACC_SLOTS / 64; j++) s += (long long) acc[k * ACC_SLOTS + lane + 64 * j];
    return acc_reduce_lane_sum(s);
}
__device__ __forceinline__ long long acc_reduce_lane_sum(long long s) {
    s += dpp_fetch_i64<0x111, 0xF>(s);
    s += dpp_fetch_i64<0x112, 0xF>(s);
    s += dpp_fetch_i64<0x114, 0xF>(s);
    s += dpp_fetch_i64<0x118, 0xF>(s);
    s += dpp_fetch_i64<0x142, 0xA>(s);
    s += dpp_fetch_i64<0x143, 0xC>(s);
    return __shfl(s, 63, 64);
}

template <class real>
__device__ __forceinline__ double cos_kz(real z, real inv_box_z) {
    const double x = 2 * 3.1415926 * z * inv_box_z;   // literal pi and double cosine in every mode (quirk Q2)
    bool ok;
    double c = cos_short_range(x, ok);                 // vv_layout.h: <= 0.79 ulp, a third of the library's instructions
    if (__builtin_expect(__any(!ok), 0)) c = ok ? c : cos(x);      // wave-uniform, practically never taken
    return c;
}

// A 16- or 32-byte element per lane for the lanes that WANT one, nothing for the others: a raw buffer load whose offset lies beyond the
// buffer in the lanes that do not want data returns zeros there without touching memory (the hardware's range check), so the load stays
// one unconditional instruction in the tile's load batch -- no divergent block, no dependent wait -- and moves only the wanted bytes.
// (`if (want) x = p[i]` puts the load into a block of its own behind a branch; an unconditional load from a clamped index fetches 32 bytes
// per lane for nothing: with in-kernel constraints 54 % of kernel A's lanes at C3 are in no cluster, profiles/pmc_latest_hbonds.json.)
template <class T4>
__device__ __forceinline__ T4 load_wanted(const void* base, uint32_t bytes, int index, bool want) {
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    static_assert(sizeof(T4) == 16 || sizeof(T4) == 32, "float4 or double4");
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int) bytes, 0x00020000);
    const unsigned off = want ? (unsigned) index * (unsigned) sizeof(T4) : 0xFFFFFFE0u;
    union { v4u u[sizeof(T4) / 16]; T4 t; } r;
    r.u[0] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int) off, 0, 0);
    if (sizeof(T4) == 32) r.u[sizeof(T4) / 16 - 1] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int) (off + 16u), 0, 0);
    return r.t;
}

// positions are posq (+ posqCorrection in mixed mode): K/middle.cu:81-96
template <class real, class mixed>
struct PosIO {
    using real4 = typename Vec<real>::v4;
    static constexpr bool kMixed = sizeof(real) != sizeof(mixed);
    // K/middle.cu:81-96: positions are posq (+ posqCorrection in mixed mode)
    static __device__ __forceinline__ void load(const void* posq, const void* corr, int i, mixed& x, mixed& y, mixed& z, mixed& w, real& zraw) {
        const real4 p1 = ((const real4*) posq)[i];
        zraw = p1.z;
        if (kMixed) {
            const real4 p2 = ((const real4*) corr)[i];
            x = p1.x + (mixed) p2.x; y = p1.y + (mixed) p2.y; z = p1.z + (mixed) p2.z; w = p1.w;
        } else {
            x = p1.x; y = p1.y; z = p1.z; w = p1.w;
        }
    }
    // x, y, z only: posq.w (the charge) and the correction's w stay as they are in memory (a virtual site stored by its parent's lane)
    static __device__ __forceinline__ void store_xyz(void* posq, void* corr, int i, mixed x, mixed y, mixed z) {
        struct alignas(sizeof(real) == 4 ? 16 : 32) R3 { real x, y, z; };      // (one 12- / 24-byte store at the element's alignment)
        *(R3*) ((real4*) posq + i) = R3{(real) x, (real) y, (real) z};
        if (kMixed) *(R3*) ((real4*) corr + i) = R3{(real) (x - (real) x), (real) (y - (real) y), (real) (z - (real) z)};
    }
    static __device__ __forceinline__ void store(void* posq, void* corr, int i, mixed x, mixed y, mixed z, mixed w) {
        real4 p = {(real) x, (real) y, (real) z, (real) w};
        store_vec((real4*) posq, i, p);
        if (kMixed) {
            real4 c = {(real) (x - (real) x), (real) (y - (real) y), (real) (z - (real) z), 0};
            store_vec((real4*) corr, i, c);
        }
    }
};

// A solver that reaches its iteration cap with a constraint still outside its tolerance says so: sticky word [3] of the plan's status (pinned host
// memory, system-scope store; the host reports VVHIP_ERR_CONSTRAINT from vvhip_synchronize and the run loops -- like an accumulator overflow or
// a rendezvous that ran out, never silently).  Seen in the wild: near-collinear rigid triangles (an angle of 1-2 degrees), which Gauss-Seidel
// sweeps do not converge in 150 rounds -- OpenMM's own sweeps stop at their cap likewise, but there the host is told nothing.
__device__ __forceinline__ void constraint_cap_reached(unsigned int* status) {
    if (status) __hip_atomic_store(&status[3], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

