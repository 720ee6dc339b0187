// vv_dev_barostat.inc -- part of vv_device.inc: the device half of a Monte Carlo barostat attempt (vvhip_barostat_scale): every molecule is
// moved rigidly so that its geometric centre scales with the box.  Two stand-alone kernels over the plan's wave layout (and the list of the
// shard's particles without a lane: image particles, virtual sites placed from a parent's lane) that touch posq.xyz, the correction's xyz and
// their own scratch (BarostatArgs::words), and nothing else: no posq.w, no corr.w, no velocity, no velm.w, no force, no forceExtra, no
// thermostat copy, no accumulator, no rendezvous or status word.  The geometric centre is OpenMM's choice for its barostat as remembered,
// stated in float64 and NOT pinned against OpenMM (DESIGN.md section 2).  include/vvhip.h states the arithmetic; in short, with X the stored
// position in double (posq + correction in mixed precision) and F = BarostatArgs::frac_bits
//   sum:    Q = llrint(X 2^F) (to nearest even) per component, valid for finite |X| < 2^22 nm -- anything else raises the bad word and adds
//           nothing --, added into the molecule's three words as integers: exact, the same bits in any order.  In front of the atomics a
//           segmented wave reduction over runs of neighbouring lanes of one molecule: with the COM temperature group every molecule sits
//           inside one wave and gets one atomic per component; interleaved or split molecules get one per run.  (Wrapping uint64 arithmetic:
//           a run's total is exact whenever the molecule's is, |S| < 2^62 by construction.)
//   shift:  c = ((double) S 2^-F) / n_m, d = c e (one multiply, contraction off), X' = X + d (one add); stored as posq' = (real) X',
//           corr' = (real) (X' - (double) posq') -- the split of kernel B's position store (PosIO::store_xyz) --; an axis with e = 0 keeps
//           its stored bits, posq and correction alike; with the bad word raised nothing is stored at all.
// Nothing between the two but the kernel boundary.  The scratch is cleared by the host's asynchronous memset in front (never captured).

__device__ __forceinline__ unsigned long long baro_scan(unsigned long long x) {
    x += (unsigned long long) dpp_fetch_i64<0x111, 0xF>((long long) x);
    x += (unsigned long long) dpp_fetch_i64<0x112, 0xF>((long long) x);
    x += (unsigned long long) dpp_fetch_i64<0x114, 0xF>((long long) x);
    x += (unsigned long long) dpp_fetch_i64<0x118, 0xF>((long long) x);
    x += (unsigned long long) dpp_fetch_i64<0x142, 0xA>((long long) x);
    x += (unsigned long long) dpp_fetch_i64<0x143, 0xC>((long long) x);
    return x;
}
__device__ __forceinline__ unsigned long long baro_shfl(unsigned long long x, int src) {
    const unsigned lo = (unsigned) __shfl((int) (unsigned) x, src, 64), hi = (unsigned) __shfl((int) (unsigned) (x >> 32), src, 64);
    return ((unsigned long long) hi << 32) | lo;
}
// the stored position in double, and its fixed-point image (false: out of range or not finite)
template <class real4>
__device__ __forceinline__ void baro_position(const real4& p, const real4& c, bool mixed_mode, double (&x)[3]) {
    x[0] = (double) p.x; x[1] = (double) p.y; x[2] = (double) p.z;
    if (mixed_mode) { x[0] += (double) c.x; x[1] += (double) c.y; x[2] += (double) c.z; }
}
__device__ __forceinline__ bool baro_fixed(const double (&x)[3], double scale, unsigned long long (&q)[3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const bool in = fabs(x[k]) < 4194304.0;      // (false for NaN)
        q[k] = in ? (unsigned long long) __double2ll_rn(x[k] * scale) : 0ull;
        ok = ok && in;
    }
    return ok;
}

template <class real, class mixed>
__global__ void __launch_bounds__(512) vv_kernel_barostat_sum(const BarostatArgs a) {
    using real4 = typename Vec<real>::v4;
    constexpr bool kMixed = sizeof(real) != sizeof(mixed);
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    bool bad = false;
    for (int wave = blockIdx.x * wpb + (threadIdx.x >> 6); wave < a.nwaves; wave += gridDim.x * wpb) {      // (uniform in the wave)
        const size_t k = (size_t) wave * 64 + lane;
        const int2 slot = a.slots[k];
        const int mol = slot.x >= 0 ? a.lane_mol[k] : -1;
        unsigned long long q[3] = {0, 0, 0};
        if (mol >= 0) {
            const real4 p = ((const real4*) a.posq)[slot.x];
            real4 c = {0, 0, 0, 0};
            if (kMixed) c = ((const real4*) a.corr)[slot.x];
            double x[3];
            baro_position(p, c, kMixed, x);
            if (!baro_fixed(x, a.scale, q)) { bad = true; q[0] = q[1] = q[2] = 0; }
        }
        // runs of neighbouring lanes of one molecule: the run's total in its last lane, from the wave's prefix sums (every lane takes part)
        const int prev = __shfl(mol, lane > 0 ? lane - 1 : 0, 64);
        const unsigned long long heads = __ballot(lane == 0 || prev != mol);
        const unsigned long long upto = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
        const int head = 63 - __clzll((long long) upto);      // (bit 0 is always set)
        const bool last = lane == 63 || ((heads >> (lane + 1)) & 1ull);
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const unsigned long long P = baro_scan(q[d]);
            const unsigned long long below = baro_shfl(P, head > 0 ? head - 1 : 0);
            const unsigned long long t = head > 0 ? P - below : P;
            if (last && mol >= 0 && t != 0) atomicAdd(&a.words[BARO_HEAD + 3 * (size_t) mol + d], t);
        }
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.nlaneless; i += gridDim.x * blockDim.x) {
        const int2 w = a.laneless[i];
        const real4 p = ((const real4*) a.posq)[w.x];
        real4 c = {0, 0, 0, 0};
        if (kMixed) c = ((const real4*) a.corr)[w.x];
        double x[3];
        unsigned long long q[3];
        baro_position(p, c, kMixed, x);
        if (!baro_fixed(x, a.scale, q)) { bad = true; continue; }
#pragma unroll
        for (int d = 0; d < 3; d++)
            if (q[d] != 0) atomicAdd(&a.words[BARO_HEAD + 3 * (size_t) w.y + d], q[d]);
    }
    if (bad) atomicOr(&a.words[BARO_BAD], 1ull);
}

template <class real, class mixed>
__device__ __forceinline__ void baro_shift(const BarostatArgs& a, int atom, int mol) {
    using real4 = typename Vec<real>::v4;
    constexpr bool kMixed = sizeof(real) != sizeof(mixed);
    real4 p = ((const real4*) a.posq)[atom];
    real4 c = {0, 0, 0, 0};
    if (kMixed) c = ((const real4*) a.corr)[atom];
    double x[3];
    baro_position(p, c, kMixed, x);
    const double n = a.mol_count[mol];
    real np[3] = {p.x, p.y, p.z}, nc[3] = {c.x, c.y, c.z};
#pragma unroll
    for (int d = 0; d < 3; d++) {
        if (a.e[d] == 0.0) continue;      // (uniform: a kernel argument) the stored bits stay, posq and correction alike
        const double centre = ((double) (long long) a.words[BARO_HEAD + 3 * (size_t) mol + d] * a.inv_scale) / n;
        const double shift = centre * a.e[d];
        const double xn = x[d] + shift;
        np[d] = (real) xn;
        nc[d] = kMixed ? (real) (xn - (double) np[d]) : (real) 0;
    }
    p.x = np[0]; p.y = np[1]; p.z = np[2];
    ((real4*) a.posq)[atom] = p;
    if (kMixed) {
        c.x = nc[0]; c.y = nc[1]; c.z = nc[2];
        ((real4*) a.corr)[atom] = c;
    }
}

template <class real, class mixed>
__global__ void __launch_bounds__(512) vv_kernel_barostat_shift(const BarostatArgs a) {
    if (a.words[BARO_BAD] != 0) return;      // (every thread reads the same word: nothing is stored at all)
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int wave = blockIdx.x * wpb + (threadIdx.x >> 6); wave < a.nwaves; wave += gridDim.x * wpb) {
        const size_t k = (size_t) wave * 64 + lane;
        const int2 slot = a.slots[k];
        if (slot.x < 0) continue;
        const int mol = a.lane_mol[k];
        if (mol >= 0) baro_shift<real, mixed>(a, slot.x, mol);
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.nlaneless; i += gridDim.x * blockDim.x) {
        const int2 w = a.laneless[i];
        baro_shift<real, mixed>(a, w.x, w.y);
    }
}
