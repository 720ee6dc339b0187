// vv_dev_acf.inc -- part of vv_device.inc: autocorrelations of a per-unit vector (vvhip_acf_*; include/vvhip.h states the units and their
// vector, the bad vectors, the schedule of origins and lags, the terms and the fixed point).  Stand-alone kernels that read velm (the
// velocity modes) or posq and posqCorrection (orientation mode) and write the recorder's own words, and nothing else: no force, no
// accumulator, no thermostat copy, no rendezvous or status word.
//   acf:      one thread per unit (a particle's velocity, a molecule's centre-of-mass velocity, or the unit vector from a pair's tail to its
//             head), striding over a capped grid of blocks of 64 .. 512 threads.  The thread forms its unit's vector in float64 -- a
//             molecule's as the sequential sum over its members in ascending particle index, a pair's through acf_inverse_norm
//             (vv_layout.h): order and sequence are part of the definition --, NaN in all three components where the vector is bad, reads the
//             sample ordinal j and the origin floor from the device-side words (nothing writes them while this kernel runs), adds the self
//             term to row 0 from its registers where j is an origin, and walks the ring's slots: slot s holds origin k E with k the
//             largest k = s (mod num_origins) and k E < j.  Of a live origin it reads ring[slot][a][u] for its own u only and adds the pair
//             to row j - k E of its group.  If j is a multiple of E it stores its vector into slot (j / E) mod num_origins.
//             STORE AND READ NEED NO ORDERING: the slot a new origin overwrites held origin j - num_origins E <= j - num_lags, which no
//             row can use, so this sample never reads the slot it writes; and the ring is planar, double[num_origins][3][stride], every
//             thread touching only its own column u.  No barrier, within a block or across blocks.
//             The slot loop issues a.slots_in_flight slots' ring loads (three each) before it uses the first: one slot at a time the walk
//             is a chain of dependent round trips.  Which slots are live, and their rows, are wave-uniform.
//             All lanes of a wave add to the same lag row for a given origin; where the wave's units share a group (always without
//             groups; nearly always with them, the units being ordered by group) and a.wave_reduce is set, the 4 or 5 int64 words are
//             summed across the wave and added once, otherwise every lane adds its own.  Integer adds commute: both give the same bits, as
//             does any grid, block size, unit order or number of slots in flight.  LDS_TABLE (a table of at most 64 KiB): the adds go to
//             the block's private copy in LDS with workgroup-scope 64-bit atomics, zeroed at block start and flushed with agent-scope adds
//             that skip the zero words, as the MSD kernel does.
//   advance:  one thread behind it (the kernel boundary orders it behind every block's read of the ordinal): counts the sample, or counts
//             it as dropped past max_samples -- no memset node, no host work.
//   floor:    one thread: the origin floor becomes the current ordinal (vvhip_set_velocities_to_temperature rewrote the velocities: the
//             origins stored so far are dead, the table is kept).
// The tails need no special case: lanes past the last unit take part in the wave's sums with zeros, and a shard without recorded units
// runs one idle block and the advance.

// a word every lane has loaded from the same address, as the scalar it is: what is derived from it branches without a lane mask
__device__ __forceinline__ long long acf_uniform(unsigned long long x) {
    const unsigned lo = (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) x), hi = (unsigned) __builtin_amdgcn_readfirstlane((int) (unsigned) (x >> 32));
    return (long long) (((unsigned long long) hi << 32) | lo);
}

template <class real, class mixed, int MODE, bool GROUPED, bool LDS_TABLE>
__global__ void __launch_bounds__(512) vv_kernel_acf(const AcfArgs a) {
    using real4 = typename Vec<real>::v4;
    using mixed4 = typename Vec<mixed>::v4;
    constexpr bool CORR = sizeof(real) != sizeof(mixed);      // mixed precision: the position is posq + posqCorrection, summed in double
    constexpr int W = MODE == ACF_ORIENTATION ? 5 : 4;        // words per row
    constexpr int Q = ACF_MAX_SLOTS_IN_FLIGHT;
    const long long j = acf_uniform(__hip_atomic_load((const unsigned long long*) &a.words[ACF_SAMPLES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (j >= a.max_samples) return;
    const long long floor_j = acf_uniform(__hip_atomic_load((const unsigned long long*) &a.words[ACF_FLOOR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    long long* const table = a.words + ACF_HEAD;
    long long* acc = table;
    if (LDS_TABLE) {
        extern __shared__ double vv_dyn_lds[];
        acc = (long long*) vv_dyn_lds;
        for (int w = threadIdx.x; w < a.table_words; w += blockDim.x) acc[w] = 0;
        __syncthreads();
    }
    auto add = [&](long long* at, long long v) {
        if (LDS_TABLE) __hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else __hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto position = [&](int k, double x[3]) {
        const real4 p = ((const real4*) a.posq)[k];
        x[0] = (double) p.x; x[1] = (double) p.y; x[2] = (double) p.z;
        if (CORR) {
            const real4 q = ((const real4*) a.corr)[k];
            x[0] = x[0] + (double) q.x; x[1] = x[1] + (double) q.y; x[2] = x[2] + (double) q.z;
        }
    };
    auto velocity = [&](int k, double x[3]) {
        const mixed4 v = ((const mixed4*) a.velm)[k];
        x[0] = (double) v.x; x[1] = (double) v.y; x[2] = (double) v.z;
    };
    const int R = a.num_origins, E = a.origin_every;
    const int sif = a.slots_in_flight;
    const long long kmax = j > 0 ? (j - 1) / E : -1;         // the newest origin in front of this sample
    const bool store = j % E == 0;                           // this sample is an origin: the self term, then the store
    const int store_slot = (int) ((j / E) % R);
    const int kmax_slot = kmax >= 0 ? (int) (kmax % R) : 0;  // where the newest origin lies: the slots behind it hold the ones before
    const size_t plane = (size_t) a.stride;
    const int lane = threadIdx.x & 63;
    const long long stride = (long long) gridDim.x * blockDim.x;
    const double nan = __builtin_nan("");
    // (the loop's bound is the wave's first unit: every lane of a wave makes the same trips and takes part in the wave's sums)
    for (long long u = (long long) blockIdx.x * blockDim.x + threadIdx.x; u - lane < a.n; u += stride) {
        const bool live = u < a.n;
        double c[3] = {0, 0, 0};
        int g = 0;
        if (live) {
            if (GROUPED) g = a.group[u];
            bool good;
            if (MODE == ACF_VELOCITY_MOLECULES) {
                double s[3] = {0, 0, 0};
                const int end = a.first[u + 1];
                // (four members' loads in flight at a time -- a member past the end repeats the chunk's first -- and the sum in the members' order)
                for (int m = a.first[u]; m < end; m += 4) {
                    int k[4];
                    double w[4], x[4][3];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int at = m + q < end ? m + q : m;
                        k[q] = a.index[at]; w[q] = a.weight[at];
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) velocity(k[q], x[q]);
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (m + q < end) { s[0] = s[0] + w[q] * x[q][0]; s[1] = s[1] + w[q] * x[q][1]; s[2] = s[2] + w[q] * x[q][2]; }
                }
                const double M = a.total[u];
                c[0] = s[0] / M; c[1] = s[1] / M; c[2] = s[2] / M;
            } else if (MODE == ACF_VELOCITY_PARTICLES) {
                velocity(a.index ? a.index[u] : (int) u, c);
            } else {
                double h[3], t[3];
                const int2 pr = ((const int2*) a.index)[u];
                position(pr.x, h); position(pr.y, t);
                c[0] = h[0] - t[0]; c[1] = h[1] - t[1]; c[2] = h[2] - t[2];
            }
            if (MODE == ACF_ORIENTATION) {
                const double n2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
                good = n2 >= 0x1p-40 && n2 < 0x1p40;                                          // (false for a NaN)
                if (good) {
                    const double y = acf_inverse_norm(n2);
                    c[0] = c[0] * y; c[1] = c[1] * y; c[2] = c[2] * y;
                }
            } else
                good = fabs(c[0]) < a.limit && fabs(c[1]) < a.limit && fabs(c[2]) < a.limit;   // (false for a NaN)
            if (!good) { c[0] = nan; c[1] = nan; c[2] = nan; }
        }
        bool uniform = false;
        if (a.wave_reduce) uniform = !GROUPED || __all(!live || g == __shfl(g, 0, 64));      // (lane 0 is live: the loop's bound)
        const int g0 = GROUPED ? __shfl(g, 0, 64) : 0;
        long long bad = 0;
        // one (origin, now) pair of this unit into row `row`; the origin's vector is o
        auto pair = [&](int row, double ox, double oy, double oz) {
            long long w[W];
#pragma unroll
            for (int q = 0; q < W; q++) w[q] = 0;
            if (live) {
                const double px = ox * c[0], py = oy * c[1], pz = oz * c[2];
                if (ox == ox && c[0] == c[0]) {                                               // (a bad vector is NaN in every component)
                    w[0] = 1; w[1] = llrint(px * a.scale); w[2] = llrint(py * a.scale); w[3] = llrint(pz * a.scale);
                    if (W == 5) {
                        const double cs = (px + py) + pz;
                        w[W - 1] = llrint(cs * cs * a.scale);
                    }
                } else
                    bad++;
            }
            if (uniform) {
                long long* at = acc + ((size_t) g0 * (size_t) a.num_lags + (size_t) row) * W;
#pragma unroll
                for (int q = 0; q < W; q++) {
                    const long long t = rep_wave_sum(w[q]);
                    if (lane == 0 && t != 0) add(at + q, t);
                }
            } else if (w[0]) {
                long long* at = acc + ((size_t) g * (size_t) a.num_lags + (size_t) row) * W;
#pragma unroll
                for (int q = 0; q < W; q++) add(at + q, w[q]);
            }
        };
        if (store) pair(0, c[0], c[1], c[2]);
        for (int s0 = 0; s0 < R && kmax >= 0; s0 += sif) {
            double o[Q][3];
            int row[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) {
                row[q] = -1;
                const int slot = s0 + q;
                if (q >= sif || slot >= R) continue;
                const long long k = kmax - (kmax_slot - slot + (kmax_slot < slot ? R : 0));  // wave-uniform, as the row below
                if (k < 0 || k * E < floor_j || j - k * E >= a.num_lags) continue;
                row[q] = (int) (j - k * E);
                if (live) {
                    const double* at = a.ring + (size_t) slot * 3 * plane + (size_t) u;
                    o[q][0] = at[0]; o[q][1] = at[plane]; o[q][2] = at[2 * plane];
                }
            }
#pragma unroll
            for (int q = 0; q < Q; q++)
                if (row[q] >= 0) pair(row[q], o[q][0], o[q][1], o[q][2]);
        }
        if (bad) __hip_atomic_fetch_add(&a.words[ACF_OUT_OF_RANGE], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (store && live) {
            double* at = a.ring + (size_t) store_slot * 3 * plane + (size_t) u;
            at[0] = c[0]; at[plane] = c[1]; at[2 * plane] = c[2];
        }
    }
    if (LDS_TABLE) {
        __syncthreads();
        for (int w = threadIdx.x; w < a.table_words; w += blockDim.x) {
            const long long v = acc[w];
            if (v != 0) __hip_atomic_fetch_add(table + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

#ifndef VV_DEVICE_NO_PLAIN_KERNELS
__global__ void __launch_bounds__(64) vv_kernel_acf_advance(const AcfArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (a.words[ACF_SAMPLES] < a.max_samples) a.words[ACF_SAMPLES] = a.words[ACF_SAMPLES] + 1;
    else a.words[ACF_DROPPED] = a.words[ACF_DROPPED] + 1;
}
__global__ void __launch_bounds__(64) vv_kernel_acf_floor(long long* words) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    words[ACF_FLOOR] = words[ACF_SAMPLES];
}
#endif
