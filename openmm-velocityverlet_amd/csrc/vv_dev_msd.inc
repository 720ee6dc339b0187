// vv_dev_msd.inc -- part of vv_device.inc: mean-squared displacements (vvhip_msd_*; include/vvhip.h states the units, the schedule of
// origins and lags, the terms and the fixed point).  Stand-alone kernels that read posq and posqCorrection and write the recorder's own words,
// and nothing else: no velocity, no force, no accumulator, no thermostat copy, no rendezvous or status word.
//   msd:      one thread per unit (a particle, or a molecule's centre of mass), striding over a capped grid of blocks of 64 .. 512
//             threads.  The thread forms its unit's position in float64 -- a molecule's as the sequential sum over its members in ascending particle index: the order is part of
//             the definition --, reads the sample ordinal j and the origin floor from the device-side words (nothing writes them while this
//             kernel runs), and walks the ring's slots: slot s holds origin k E with k the largest k = s (mod num_origins) and k E < j, an
//             older holder of the slot is further back than num_lags.  Of a live origin it reads ring[slot][a][u] for its own u only and
//             adds the pair, 1 and three squares, to row j - k E - 1 of its group.  If j is a multiple of E it then stores its position
//             into slot (j / E) mod num_origins.  The ring is planar, double[num_origins][3][stride]: EVERY THREAD TOUCHES ONLY ITS OWN
//             COLUMN u, so reading a slot and overwriting it in one kernel (num_origins E == num_lags) is free of races, within a block
//             and across blocks, without a barrier.
//             All lanes of a wave add to the same lag row for a given origin; where the wave's units share a group (always without
//             groups; nearly always with them, the units being ordered by group) and a.wave_reduce is set, the four int64 words are summed
//             across the wave and added once, otherwise every lane adds its own.  Integer adds commute: both give the same bits, as does
//             any grid, block size or unit order.  LDS_TABLE (a table of at most 64 KiB): the adds go to the block's private copy in LDS,
//             zeroed at block start and flushed with agent-scope adds that skip the zero words, as the profile kernel does.
//   advance:  one thread behind it (the kernel boundary orders it behind every block's read of the ordinal): counts the sample, or counts
//             it as dropped past max_samples -- no memset node, no host work.
//   floor:    one thread: the origin floor becomes the current ordinal (vvhip_barostat_scale / _restore rewrote the positions: the origins
//             stored so far are dead, the table is kept).
// The tails need no special case: lanes past the last unit take part in the wave's sums with zeros, and a shard without recorded units
// runs one idle block and the advance.

template <class real, class mixed, bool MOLECULES, bool GROUPED, bool LDS_TABLE>
__global__ void __launch_bounds__(512) vv_kernel_msd(const MsdArgs a) {
    using real4 = typename Vec<real>::v4;
    constexpr bool CORR = sizeof(real) != sizeof(mixed);      // mixed precision: the position is posq + posqCorrection, summed in double
    const long long j = (long long) __hip_atomic_load((const unsigned long long*) &a.words[MSD_SAMPLES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (j >= a.max_samples) return;
    const long long floor_j = (long long) __hip_atomic_load((const unsigned long long*) &a.words[MSD_FLOOR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    long long* const table = a.words + MSD_HEAD;
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
    const int R = a.num_origins, E = a.origin_every;
    const long long kmax = j > 0 ? (j - 1) / E : -1;         // the newest origin in front of this sample
    const bool store = j % E == 0;
    const int store_slot = (int) ((j / E) % R);
    const size_t plane = (size_t) a.stride;
    const int lane = threadIdx.x & 63;
    const long long stride = (long long) gridDim.x * blockDim.x;
    // (the loop's bound is the wave's first unit: every lane of a wave makes the same trips and takes part in the wave's sums)
    for (long long u = (long long) blockIdx.x * blockDim.x + threadIdx.x; u - lane < a.n; u += stride) {
        const bool live = u < a.n;
        double c[3] = {0, 0, 0};
        int g = 0;
        if (live) {
            if (GROUPED) g = a.group[u];
            if (MOLECULES) {
                double s[3] = {0, 0, 0};
                const int end = a.first[u + 1];
                // (four members' loads in flight at a time -- a member past the end repeats the chunk's first -- and the sum in the members'
                // order: one member at a time the loop is two dependent memory round trips per member and nothing else)
                for (int m = a.first[u]; m < end; m += 4) {
                    int k[4];
                    double w[4], x[4][3];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int at = m + q < end ? m + q : m;
                        k[q] = a.index[at]; w[q] = a.weight[at];
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) position(k[q], x[q]);
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        if (m + q < end) { s[0] = s[0] + w[q] * x[q][0]; s[1] = s[1] + w[q] * x[q][1]; s[2] = s[2] + w[q] * x[q][2]; }
                }
                const double M = a.total[u];
                c[0] = s[0] / M; c[1] = s[1] / M; c[2] = s[2] / M;
            } else
                position(a.index ? a.index[u] : (int) u, c);
        }
        bool uniform = false;
        if (a.wave_reduce) uniform = !GROUPED || __all(!live || g == __shfl(g, 0, 64));      // (lane 0 is live: the loop's bound)
        long long bad = 0;
        for (int slot = 0; slot < R && kmax >= 0; slot++) {
            const long long k = kmax - ((kmax - slot) % R + R) % R;                          // wave-uniform, as the row below
            if (k < 0 || k * E < floor_j || j - k * E > a.num_lags) continue;
            const int row = (int) (j - k * E - 1);
            long long w[4] = {0, 0, 0, 0};
            if (live) {
                const double* o = a.ring + (size_t) slot * 3 * plane + (size_t) u;
                const double dx = c[0] - o[0], dy = c[1] - o[plane], dz = c[2] - o[2 * plane];
                if (fabs(dx) < a.limit && fabs(dy) < a.limit && fabs(dz) < a.limit) {         // (false for a NaN)
                    w[0] = 1; w[1] = llrint(dx * dx * a.scale); w[2] = llrint(dy * dy * a.scale); w[3] = llrint(dz * dz * a.scale);
                } else
                    bad++;
            }
            if (uniform) {
                const int g0 = GROUPED ? __shfl(g, 0, 64) : 0;
                long long* at = acc + ((size_t) g0 * (size_t) a.num_lags + (size_t) row) * 4;
                for (int q = 0; q < 4; q++) {
                    const long long t = rep_wave_sum(w[q]);
                    if (lane == 0 && t != 0) add(at + q, t);
                }
            } else if (w[0]) {
                long long* at = acc + ((size_t) g * (size_t) a.num_lags + (size_t) row) * 4;
                for (int q = 0; q < 4; q++) add(at + q, w[q]);
            }
        }
        if (bad) __hip_atomic_fetch_add(&a.words[MSD_OUT_OF_RANGE], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (store && live) {
            double* o = a.ring + (size_t) store_slot * 3 * plane + (size_t) u;
            o[0] = c[0]; o[plane] = c[1]; o[2 * plane] = c[2];
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
__global__ void __launch_bounds__(64) vv_kernel_msd_advance(const MsdArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (a.words[MSD_SAMPLES] < a.max_samples) a.words[MSD_SAMPLES] = a.words[MSD_SAMPLES] + 1;
    else a.words[MSD_DROPPED] = a.words[MSD_DROPPED] + 1;
}
__global__ void __launch_bounds__(64) vv_kernel_msd_floor(long long* words) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    words[MSD_FLOOR] = words[MSD_SAMPLES];
}
#endif
