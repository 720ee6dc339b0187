// vv_dev_vanhove.inc -- part of vv_device.inc: the self part of the van Hove function (vvhip_vanhove_*; include/vvhip.h states the units,
// the schedule of origins and lags, the bins, the moments and the fixed point).  Stand-alone kernels that read posq and posqCorrection and
// write the recorder's own words, and nothing else.
//   vanhove:  one thread per unit, a block a contiguous chunk of blockDim units per trip over a capped grid, the unit's float64 position
//             (the MSD kernel's, word for word) held in registers while the block walks the ring's slots in the OUTER loop.  A slot's
//             origin ordinal and lag row are the same for every thread of the grid, so per slot the block's increments go to one row
//             [group][row][0 .. num_bins) of hist for each group its chunk holds -- the units are ordered by group, a chunk holds the groups
//             gmin .. gmax of its first and last unit.  Every thread touches only its own ring column u: accumulate first, store second,
//             free of races when num_origins E == num_lags, as for the MSD.
//             The design problem is the adds: U x (live origins) increments per sample into a table of MBs.
//               plain path (LDS_HIST = false, "vanhove_lds" = 0): every increment is one agent-scope int64 add on its bin.
//               privatised path (the default): the block counts a slot into a private LDS histogram of 32-bit words,
//               [lds_groups][num_bins] with lds_groups = min(num_groups, VANHOVE_LDS_WORDS / num_bins) >= 4, by ds_add_u32 (no return: a
//               bank conflict or lanes on one bin serialise inside the CU, nothing leaves it); a unit of a group past gmin + lds_groups
//               - 1 (more than four groups of 1024 bins in one chunk) adds globally as in the plain path.  Behind one barrier the block
//               flushes the words of the groups present: a thread reads its words, and where one is non-zero zeroes it and sends ONE
//               int64 add: at most min(blockDim, num_bins) adds per slot and group instead of blockDim, and displacements at one lag
//               crowd into few bins.  Two histograms alternate by slot, so the flush of slot s runs beside the count of slot s + 1 and
//               one barrier per live slot orders both: a thread counts into a histogram again only behind the next barrier, which every
//               thread reaches after its flush.  Per-wave sub-histograms were not chosen: with up to 1024 bins eight of them leave no room
//               for a second group, and they multiply the flush's adds by eight; a ballot / match on equal bins costs a loop of up to
//               64 trips per slot where the LDS add costs one instruction.
//               LDS: 2 x 16 KiB histograms + 8 200 B of squared edges = 40 968 B, four blocks of 512 threads per CU still fit (160 KiB).
//               Barriers: one behind the zeroing and the edges' load, then one per live slot and trip; none in the plain path.
//             The bin is decided by comparisons of r2 against the squared edges alone (a bisection over e2 in LDS; no square root).
//             The six head words: pairs, below and beyond travel packed in one word (21 bits each, a wave adds at most 64), so a wave
//             whose units share a group sums four words across its lanes and lane 0 adds the six; otherwise every lane adds its own.
//             Integer adds commute: every path, grid, block size and unit order gives the same bits.
//   advance:  one thread behind it: counts the sample, or counts it as dropped past max_samples.
//   floor:    one thread: the origin floor becomes the current ordinal (the barostat rewrote the positions).
// The tails need no special case: lanes past the last unit count nothing and take part in the wave's sums with zeros and in the block's
// barriers, a wave that straddles two groups adds per lane, and a shard without recorded units runs one idle block and the advance.

template <class real, class mixed, bool MOLECULES, bool GROUPED, bool LDS_HIST>
__global__ void __launch_bounds__(512) vv_kernel_vanhove(const VanHoveArgs a) {
    using real4 = typename Vec<real>::v4;
    constexpr bool CORR = sizeof(real) != sizeof(mixed);      // mixed precision: the position is posq + posqCorrection, summed in double
    __shared__ double e2[VANHOVE_MAX_BINS + 1];
    __shared__ unsigned int lds_hist[LDS_HIST ? 2 * VANHOVE_LDS_WORDS : 1];      // two histograms, alternating by slot
    const long long j = (long long) __hip_atomic_load((const unsigned long long*) &a.words[VANHOVE_SAMPLES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (j >= a.max_samples) return;
    const long long floor_j = (long long) __hip_atomic_load((const unsigned long long*) &a.words[VANHOVE_FLOOR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    long long* const head = a.words + VANHOVE_HEAD;
    long long* const hist = head + a.head_words;
    const int B = a.num_bins;
    for (int w = threadIdx.x; w <= B; w += blockDim.x) e2[w] = a.e2[w];
    if (LDS_HIST)
        for (int w = threadIdx.x; w < 2 * VANHOVE_LDS_WORDS; w += blockDim.x) lds_hist[w] = 0;
    __syncthreads();
    auto add = [](long long* at, long long v) { __hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
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
    const double e2_first = e2[0], e2_last = e2[B];
    int phase = 0;
    long long bad = 0;
    // (the loop's bound is the block's first unit: every thread of a block makes the same trips and reaches the same barriers)
    for (long long base = (long long) blockIdx.x * blockDim.x; base < a.n; base += stride) {
        const long long u = base + threadIdx.x;
        const bool live = u < a.n;
        double c[3] = {0, 0, 0};
        int g = 0, gmin = 0, gspan = 1;
        if (GROUPED) {      // (the groups of the chunk: block-uniform)
            const long long last = base + blockDim.x - 1 < a.n ? base + blockDim.x - 1 : (long long) a.n - 1;
            gmin = a.group[base];
            gspan = a.group[last] - gmin + 1;
            if (gspan > a.lds_groups) gspan = a.lds_groups;
        }
        if (live) {
            if (GROUPED) g = a.group[u];
            if (MOLECULES) {
                double s[3] = {0, 0, 0};
                const int end = a.first[u + 1];
                // (four members' loads in flight at a time and the sum in the members' order, as the MSD kernel's)
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
        if (a.wave_reduce) uniform = !GROUPED || __all(!live || g == __shfl(g, 0, 64));      // (a wave without a live lane adds zeros)
        for (int slot = 0; slot < R && kmax >= 0; slot++) {
            const long long k = kmax - ((kmax - slot) % R + R) % R;                          // grid-uniform, as the row below
            if (k < 0 || k * E < floor_j || j - k * E > a.num_lags) continue;
            const int row = (int) (j - k * E - 1);
            long long counts = 0, w2 = 0, whi = 0, wlo = 0;                                  // counts: pairs | below << 21 | beyond << 42
            if (live) {
                const double* o = a.ring + (size_t) slot * 3 * plane + (size_t) u;
                const double dx = c[0] - o[0], dy = c[1] - o[plane], dz = c[2] - o[2 * plane];
                if (fabs(dx) < a.limit && fabs(dy) < a.limit && fabs(dz) < a.limit) {         // (false for a NaN)
                    const double r2 = (dx * dx + dy * dy) + dz * dz;
                    const double x = (r2 * r2) * a.scale_hi;
                    const double hi = floor(x);
                    w2 = llrint(r2 * a.scale2); whi = (long long) hi; wlo = llrint((x - hi) * a.scale_lo);
                    if (r2 < e2_first) counts = 1ll | (1ll << 21);
                    else if (r2 >= e2_last) counts = 1ll | (1ll << 42);
                    else {
                        counts = 1;
                        int lo = 0, up = B;                                                  // e2[lo] <= r2 < e2[up]
                        while (up - lo > 1) {
                            const int mid = (lo + up) >> 1;
                            if (r2 >= e2[mid]) lo = mid; else up = mid;
                        }
                        if (LDS_HIST && g - gmin < a.lds_groups) atomicAdd(&lds_hist[phase * VANHOVE_LDS_WORDS + (g - gmin) * B + lo], 1u);
                        else add(hist + ((size_t) g * (size_t) a.num_lags + (size_t) row) * (size_t) B + (size_t) lo, 1);
                    }
                } else
                    bad++;
            }
            if (uniform) {
                const int g0 = GROUPED ? __shfl(g, 0, 64) : 0;
                long long* at = head + ((size_t) g0 * (size_t) a.num_lags + (size_t) row) * VANHOVE_ROW;
                const long long tc = rep_wave_sum(counts), t2 = rep_wave_sum(w2), thi = rep_wave_sum(whi), tlo = rep_wave_sum(wlo);
                if (lane == 0 && tc != 0) {
                    add(at + VANHOVE_PAIRS, tc & 0x1FFFFF);
                    if ((tc >> 21) & 0x1FFFFF) add(at + VANHOVE_BELOW, (tc >> 21) & 0x1FFFFF);
                    if (tc >> 42) add(at + VANHOVE_BEYOND, tc >> 42);
                    if (t2) add(at + VANHOVE_R2, t2);
                    if (thi) add(at + VANHOVE_R4_HI, thi);
                    if (tlo) add(at + VANHOVE_R4_LO, tlo);
                }
            } else if (counts) {
                long long* at = head + ((size_t) g * (size_t) a.num_lags + (size_t) row) * VANHOVE_ROW;
                add(at + VANHOVE_PAIRS, 1);
                if ((counts >> 21) & 1) add(at + VANHOVE_BELOW, 1);
                if (counts >> 42) add(at + VANHOVE_BEYOND, 1);
                if (w2) add(at + VANHOVE_R2, w2);
                if (whi) add(at + VANHOVE_R4_HI, whi);
                if (wlo) add(at + VANHOVE_R4_LO, wlo);
            }
            if (LDS_HIST) {
                __syncthreads();
                for (int w = threadIdx.x; w < gspan * B; w += blockDim.x) {
                    const unsigned int v = lds_hist[phase * VANHOVE_LDS_WORDS + w];
                    if (v != 0) {
                        lds_hist[phase * VANHOVE_LDS_WORDS + w] = 0;
                        add(hist + ((size_t) (gmin + w / B) * (size_t) a.num_lags + (size_t) row) * (size_t) B + (size_t) (w % B), (long long) v);
                    }
                }
                phase ^= 1;
            }
        }
        if (store && live) {
            double* o = a.ring + (size_t) store_slot * 3 * plane + (size_t) u;
            o[0] = c[0]; o[plane] = c[1]; o[2 * plane] = c[2];
        }
    }
    if (bad) add(&a.words[VANHOVE_OUT_OF_RANGE], bad);
}

#ifndef VV_DEVICE_NO_PLAIN_KERNELS
__global__ void __launch_bounds__(64) vv_kernel_vanhove_advance(const VanHoveArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (a.words[VANHOVE_SAMPLES] < a.max_samples) a.words[VANHOVE_SAMPLES] = a.words[VANHOVE_SAMPLES] + 1;
    else a.words[VANHOVE_DROPPED] = a.words[VANHOVE_DROPPED] + 1;
}
__global__ void __launch_bounds__(64) vv_kernel_vanhove_floor(long long* words) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    words[VANHOVE_FLOOR] = words[VANHOVE_SAMPLES];
}
#endif
