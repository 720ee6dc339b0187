// vv_dev_modes.inc -- part of vv_device.inc: density modes for the structure factors S(k) and F(k, t) (vvhip_modes_*; include/vvhip.h states the
// turns, the phase, the phasor, the fixed-point sums, the schedule of origins and lags, the table and the order of its float64 adds).
// Stand-alone kernels that read posq and posqCorrection and write the recorder's own words and scratch, and nothing else: no velocity, no
// force, no accumulator, no thermostat copy, no rendezvous or status word.
//   gather:     one thread per recorded site over the compact list (ordered by group), striding over a capped grid: X in float64, then per
//               axis t = X inv_L, u = t - floor(t), T = (uint64) floor(u 2^32) mod 2^32 into the planar scratch uint32[3][stride].  A site
//               that is NaN or at / beyond the limit adds 1 to the sample's bad word and stores zeros.  The only kernel that touches posq.
//   modes:      the hot kernel, one block per work item (ModesItem: a group, a run of its sites, a run of modes).  A thread keeps P sites in
//               registers (T_x, T_y, T_z, w) and loops over the item's modes; the mode triple is wave-uniform and comes through scalar
//               registers.  Per mode and site: phi = n_x T_x + n_y T_y + n_z T_z in 32-bit arithmetic, the phasor (vv_layout.h), two
//               multiplies by w and two by 2^F, two round-to-nearest conversions to int32, in-lane int64 adds over the P sites; then one
//               64-bit wave sum per word, and lane 0 adds what is not zero to the block's [modes of the item][2] copy in LDS.  Behind one
//               barrier the block adds its non-zero words to the sample's sums with agent-scope adds.  Integer adds commute: the sums are
//               the same bits for any work list, P, block size or site order.  A sample the gather found invalid is skipped.
//   correlate:  one thread per (slot of the ring or the zero lag, g, h, k).  A usable slot -- it holds a sample (hold >= 0) at or above the
//               floor, 1 <= j - o <= num_lags -- gives row l = j - o; the thread adds ONE term a_g(o) a_h(j) + b_g(o) b_h(j) to its own
//               cell with a plain float64 add, so a cell is the sequential sum over the samples in ascending order whatever the grid.
//   advance:    one wave behind it: stores the sums as the origin of slot (j / E) mod num_origins where j is a multiple of E -- or marks
//               the slot dead if the sample is invalid --, zeroes the sums and the bad word, counts the sample as taken (and invalid, or
//               adds the box) or as dropped.  It strides over the G K 2 words; j and the bad word are read before any lane writes.
//   floor:      one thread: the origin floor becomes the current ordinal (vvhip_barostat_scale / _restore rewrote the positions).
// The tails need no special case: a thread's sites past its item's last repeat the item's first site's loads with w = 0 and take part in
// the wave's sums with zeros, a group without sites gives no item, and a sample without items runs one idle block.

template <class real, class mixed>
__global__ void __launch_bounds__(256) vv_kernel_modes_gather(const ModesArgs a) {
    using real4 = typename Vec<real>::v4;
    constexpr bool CORR = sizeof(real) != sizeof(mixed);      // mixed precision: the position is posq + posqCorrection, summed in double
    const unsigned long long j = __hip_atomic_load((const unsigned long long*) &a.words[MODES_SAMPLES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (j >= (unsigned long long) a.max_samples) return;
    const long long stride = (long long) gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    // (the loop's bound is the wave's first site: every lane of a wave makes the same trips and takes part in the ballot)
    for (long long s = (long long) blockIdx.x * blockDim.x + threadIdx.x; s - lane < a.n; s += stride) {
        const bool live = s < a.n;
        const int k = a.index[live ? s : s - lane];
        const real4 p = ((const real4*) a.posq)[k];
        double x[3] = {(double) p.x, (double) p.y, (double) p.z};
        if (CORR) {
            const real4 q = ((const real4*) a.corr)[k];
            x[0] = x[0] + (double) q.x; x[1] = x[1] + (double) q.y; x[2] = x[2] + (double) q.z;
        }
        const bool ok = fabs(x[0]) < a.limit && fabs(x[1]) < a.limit && fabs(x[2]) < a.limit;      // (false for a NaN)
        unsigned int T[3] = {0u, 0u, 0u};
        if (ok)
            for (int c = 0; c < 3; c++) {
                const double t = x[c] * a.inv_L[c];
                const double u = t - floor(t);                // in [0, 1]; 1.0 (from t = -1e-20) becomes 2^32 and wraps to 0: the right phase
                T[c] = (unsigned int) ((unsigned long long) floor(u * 4294967296.0) & 0xFFFFFFFFull);
            }
        if (live)
            for (int c = 0; c < 3; c++) a.turns[(size_t) c * (size_t) a.stride + (size_t) s] = T[c];
        const long long nbad = (long long) __popcll(__ballot(live && !ok));
        if (lane == 0 && nbad != 0) __hip_atomic_fetch_add(&a.words[MODES_BAD], nbad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int P>
__global__ void __launch_bounds__(512) vv_kernel_modes(const ModesArgs a) {
    __shared__ long long acc[MODES_MAX_K_TILE * 2];           // the block's sums (A, B) of its item's modes
    const unsigned long long j = __hip_atomic_load((const unsigned long long*) &a.words[MODES_SAMPLES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (j >= (unsigned long long) a.max_samples || (int) blockIdx.x >= a.num_items) return;
    if (__hip_atomic_load(&a.words[MODES_BAD], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;      // (the gather is complete: a kernel boundary)
    const ModesItem it = a.items[blockIdx.x];
    const int nk = min(it.k1 - it.k0, MODES_MAX_K_TILE);      // (the host lists no longer run: `acc` holds it)
    for (int w = threadIdx.x; w < 2 * nk; w += blockDim.x) acc[w] = 0;
    __syncthreads();
    const unsigned int* const tx = a.turns;
    const unsigned int* const ty = tx + a.stride;
    const unsigned int* const tz = ty + a.stride;
    unsigned int Tx[P], Ty[P], Tz[P];
    double ws[P];
#pragma unroll
    for (int p = 0; p < P; p++) {
        const int s = it.s0 + p * (int) blockDim.x + (int) threadIdx.x;
        const bool live = s < it.s1;
        const int at = live ? s : it.s0;                      // (it.s0 < it.s1: the host lists no empty item)
        Tx[p] = tx[at]; Ty[p] = ty[at]; Tz[p] = tz[at];
        const double w = a.weight[at];
        ws[p] = live ? w : 0.0;
    }
    const int lane = threadIdx.x & 63;
    const double scale = a.scale;
    // the mode triples are read-only for the recorder's whole life (uploaded at the start) and the index is wave-uniform: through the
    // constant address space they are scalar loads into scalar registers, whatever the block's LDS atomics and barriers do in between
    typedef const __attribute__((address_space(4))) int32_t* ConstModes;
    const ConstModes modes = (ConstModes) (a.modes + 3 * (size_t) it.k0);
    for (int k = 0; k < nk; k++) {
        const unsigned int nx = (unsigned int) modes[3 * k], ny = (unsigned int) modes[3 * k + 1], nz = (unsigned int) modes[3 * k + 2];
        long long A = 0, B = 0;
#pragma unroll
        for (int p = 0; p < P; p++) {
            const unsigned int phi = nx * Tx[p] + ny * Ty[p] + nz * Tz[p];      // (mod 2^32: the multiple of a turn drops out)
            double c, s;
            phasor_turns(phi, c, s);
            A += (long long) (int) __builtin_rint((ws[p] * c) * scale);
            B += (long long) (int) __builtin_rint((ws[p] * s) * scale);
        }
        A = rep_wave_sum(A);
        B = rep_wave_sum(B);
        if (lane == 0) {
            if (A != 0) __hip_atomic_fetch_add(&acc[2 * k], A, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (B != 0) __hip_atomic_fetch_add(&acc[2 * k + 1], B, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    long long* const sums = a.words + MODES_HEAD + ((size_t) it.group * (size_t) a.num_modes + (size_t) it.k0) * 2;
    for (int w = threadIdx.x; w < 2 * nk; w += blockDim.x) {
        const long long v = acc[w];
        if (v != 0) __hip_atomic_fetch_add(sums + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

#ifndef VV_DEVICE_NO_PLAIN_KERNELS
__global__ void __launch_bounds__(256) vv_kernel_modes_correlate(const ModesArgs a) {
    const long long j = a.words[MODES_SAMPLES];
    if (j >= a.max_samples || a.words[MODES_BAD] != 0) return;
    const int G = a.num_groups, K = a.num_modes, R = a.num_origins;
    const long long* const sums = a.words + MODES_HEAD;
    const long long floor_j = a.words[MODES_FLOOR];
    const long long cells = (long long) G * G * K;
    const long long total = (long long) (R + 1) * cells;
    const size_t slot_words = (size_t) G * (size_t) K * 2;
    const long long stride = (long long) gridDim.x * blockDim.x;
    for (long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int s = (int) (t / cells);                      // s == R: the zero lag
        const long long c = t % cells;
        long long l = 0;
        const long long* org = sums;
        if (s < R) {
            const long long o = a.hold[s];
            if (o < 0 || o < floor_j) continue;
            l = j - o;
            if (l < 1 || l > a.num_lags) continue;
            org = a.ring + (size_t) s * slot_words;
        }
        long long* const row = a.table + (size_t) l * (size_t) a.row_words;
        if (c == 0) row[0] = row[0] + 1;
        const int k = (int) (c % K), gh = (int) (c / K);
        const int g = gh / G, h = gh % G;
        const size_t og = ((size_t) g * (size_t) K + (size_t) k) * 2, jh = ((size_t) h * (size_t) K + (size_t) k) * 2;
        const double ao = (double) org[og] * a.inv_scale, bo = (double) org[og + 1] * a.inv_scale;      // the origin is the first index
        const double aj = (double) sums[jh] * a.inv_scale, bj = (double) sums[jh + 1] * a.inv_scale;
        const double term = ao * aj + bo * bj;
        long long* const cell = row + 1 + c;
        *cell = __double_as_longlong(__longlong_as_double(*cell) + term);
    }
}
__global__ void __launch_bounds__(64) vv_kernel_modes_advance(const ModesArgs a) {
    if (blockIdx.x != 0) return;
    const int lane = threadIdx.x;
    const long long nw = (long long) a.num_groups * a.num_modes * 2;
    const long long j = a.words[MODES_SAMPLES], bad = a.words[MODES_BAD];
    const bool taken = j < a.max_samples;
    const bool origin = taken && a.num_origins > 0 && j % a.origin_every == 0;
    const int slot = origin ? (int) ((j / a.origin_every) % a.num_origins) : 0;
    long long* const sums = a.words + MODES_HEAD;
    for (long long w = lane; w < nw; w += 64) {
        if (origin && bad == 0) a.ring[(size_t) slot * (size_t) nw + (size_t) w] = sums[w];
        sums[w] = 0;
    }
    if (lane != 0) return;
    if (origin) a.hold[slot] = bad == 0 ? j : -1;
    a.words[MODES_BAD] = 0;
    if (!taken) { a.words[MODES_DROPPED] = a.words[MODES_DROPPED] + 1; return; }
    a.words[MODES_SAMPLES] = j + 1;
    a.words[MODES_OUT_OF_RANGE] = a.words[MODES_OUT_OF_RANGE] + bad;
    if (bad != 0) a.words[MODES_INVALID] = a.words[MODES_INVALID] + 1;
    else
        for (int c = 0; c < 3; c++)
            a.words[MODES_BOX_SUM + c] = __double_as_longlong(__longlong_as_double(a.words[MODES_BOX_SUM + c]) + a.box[c]);
}
__global__ void __launch_bounds__(64) vv_kernel_modes_floor(long long* words) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    words[MODES_FLOOR] = words[MODES_SAMPLES];
}
#endif
