// vv_dev_current.inc -- part of vv_device.inc: collective current correlations (vvhip_current_*; include/vvhip.h states the weighted sums, the
// schedule of origins and lags, the table and the order of its float64 adds).  Stand-alone kernels that read posq, posqCorrection and velm and
// write the recorder's own words, and nothing else: no force, no accumulator, no thermostat copy, no rendezvous or status word.
//   reduce:     one thread per recorded particle over the compact list (index, weight, group: ordered by group), striding over a capped grid.
//               All of a thread's loads -- list entry, weight, group byte, posq, the correction in mixed precision, velm -- are issued before
//               the first use.  Six int64 terms per lane, llrint((w X_a) 2^Fp) and llrint((w v_a) 2^Fv); a wave whose lanes share a group
//               (nearly always: the list is ordered by group) sums them across the lanes and adds once, otherwise every lane adds its own.
//               The adds go to the block's [G][6] copy in LDS and from there, skipping the zero words, to the sample's sums with
//               agent-scope adds.  A particle out of range adds nothing but 1 to the sample's bad word.  Integer adds commute: the sums are
//               the same bits for any grid, block size or particle order.  At or past max_samples nothing is added.
//               SLABS (the two-level form): the block stores its copy, zeros included, to its own slab with plain stores instead, and the
//               correlate kernel's blocks each sum the slabs in LDS first (block 0 also writes the totals to the sample's words for the
//               advance kernel).  Exact integer sums either way: the same bits.
//   correlate:  one thread per (slot of the ring or the zero lag, class, component).  A slot whose origin o is usable -- it holds a sample
//               (hold >= 0) at or above the floor, 1 <= j - o <= num_lags -- gives row l = j - o; a thread adds ONE term to its own cell of
//               that row with a plain float64 add, so a cell's value is the sequential sum over the samples in ascending order whatever the
//               grid.  An invalid sample (bad word != 0) adds nothing.
//   advance:    one wave behind it (the kernel boundaries order it behind every read of the ordinal, the sums and the ring): stores the sums
//               as the origin of slot (j / E) mod num_origins where j is a multiple of E -- or marks the slot dead if the sample is invalid
//               --, zeroes the sums and the bad word, counts the sample as taken (and invalid, or adds 1 / V) or as dropped.  Every lane
//               reads what it needs before any lane writes.  No memset node, no host work.
//   floor:      one thread: the origin floor becomes the current ordinal (vvhip_barostat_scale / _restore rewrote the positions).
// The tails need no special case: lanes past the last particle repeat their wave's first particle's loads and take part in the wave's sums
// with zeros, and a plan without recorded particles runs one idle block.

template <class real, class mixed, bool SLABS>
__global__ void __launch_bounds__(512) vv_kernel_current_reduce(const CurrentArgs a) {
    using real4 = typename Vec<real>::v4;
    using mixed4 = typename Vec<mixed>::v4;
    constexpr bool CORR = sizeof(real) != sizeof(mixed);      // mixed precision: the position is posq + posqCorrection, summed in double
    __shared__ long long acc[CUR_MAX_GROUPS * 6 + 1];         // the block's sums, then its bad count
    const unsigned long long j = __hip_atomic_load((const unsigned long long*) &a.words[CUR_SAMPLES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (j >= (unsigned long long) a.max_samples) return;
    const int nw = a.num_groups * 6;
    for (int w = threadIdx.x; w <= nw; w += blockDim.x) acc[w] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long stride = (long long) gridDim.x * blockDim.x;
    // (the loop's bound is the wave's first particle: every lane of a wave makes the same trips and takes part in the wave's sums)
    for (long long u = (long long) blockIdx.x * blockDim.x + threadIdx.x; u - lane < a.n; u += stride) {
        const bool live = u < a.n;
        const long long at = live ? u : u - lane;
        const int k = a.index[at];
        const double w = a.weight[at];
        const int g = a.group[at];
        const real4 p = ((const real4*) a.posq)[k];
        real4 q = p;
        if (CORR) q = ((const real4*) a.corr)[k];
        const mixed4 vm = ((const mixed4*) a.velm)[k];
        double x[3] = {(double) p.x, (double) p.y, (double) p.z};
        if (CORR) { x[0] = x[0] + (double) q.x; x[1] = x[1] + (double) q.y; x[2] = x[2] + (double) q.z; }
        const double v[3] = {(double) vm.x, (double) vm.y, (double) vm.z};
        const bool ok = fabs(x[0]) < a.limit_p && fabs(x[1]) < a.limit_p && fabs(x[2]) < a.limit_p &&
                        fabs(v[0]) < a.limit_v && fabs(v[1]) < a.limit_v && fabs(v[2]) < a.limit_v;      // (false for a NaN)
        long long t[6] = {0, 0, 0, 0, 0, 0};
        if (live && ok)
            for (int c = 0; c < 3; c++) { t[c] = llrint((w * x[c]) * a.scale_p); t[3 + c] = llrint((w * v[c]) * a.scale_v); }
        const int g0 = __shfl(g, 0, 64);                      // (lane 0 is live: the loop's bound)
        if (__all(g == g0)) {
            for (int c = 0; c < 6; c++) {
                const long long s = rep_wave_sum(t[c]);
                if (lane == 0 && s != 0) __hip_atomic_fetch_add(&acc[g0 * 6 + c], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        } else if (live && ok) {
            for (int c = 0; c < 6; c++)
                if (t[c] != 0) __hip_atomic_fetch_add(&acc[g * 6 + c], t[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        const long long nbad = (long long) __popcll(__ballot(live && !ok));
        if (lane == 0 && nbad != 0) __hip_atomic_fetch_add(&acc[nw], nbad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    for (int w = threadIdx.x; w <= nw; w += blockDim.x) {
        const long long s = acc[w];
        if (SLABS) a.slabs[(size_t) blockIdx.x * (size_t) (nw + 1) + w] = s;
        else if (s != 0) __hip_atomic_fetch_add(w < nw ? &a.words[CUR_HEAD + w] : &a.words[CUR_BAD], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

#ifndef VV_DEVICE_NO_PLAIN_KERNELS
__global__ void __launch_bounds__(256) vv_kernel_current_correlate(const CurrentArgs a) {
    const long long j = a.words[CUR_SAMPLES];
    if (j >= a.max_samples) return;
    const int G = a.num_groups, ND = G * (G + 1) / 2, NC = G * G, R = a.num_origins;
    const long long* sums = a.words + CUR_HEAD;
    if (a.slabs) {                                            // two-level: every block sums the reduce's slabs; block 0 publishes the totals
        __shared__ long long tot[CUR_MAX_GROUPS * 6 + 1];
        const int nw1 = G * 6 + 1;
        for (int w = threadIdx.x; w < nw1; w += blockDim.x) tot[w] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < a.num_slabs * nw1; i += blockDim.x) {
            const long long s = a.slabs[i];
            if (s != 0) __hip_atomic_fetch_add(&tot[i % nw1], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __syncthreads();
        if (blockIdx.x == 0)
            for (int w = threadIdx.x; w < nw1; w += blockDim.x) a.words[w < nw1 - 1 ? CUR_HEAD + w : (int) CUR_BAD] = tot[w];
        sums = tot;
        if (tot[nw1 - 1] != 0) return;
    } else if (a.words[CUR_BAD] != 0)
        return;
    const long long floor_j = a.words[CUR_FLOOR];
    const int cells = 3 * (ND + NC);
    const long long total = (long long) (R + 1) * cells;
    const long long stride = (long long) gridDim.x * blockDim.x;
    for (long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int s = (int) (t / cells), c = (int) (t % cells);      // s == R: the zero lag
        const int cls = c / 3, comp = c % 3;
        long long l = 0;
        const long long* org = sums;
        if (s < R) {
            const long long o = a.hold[s];
            if (o < 0 || o < floor_j) continue;
            l = j - o;
            if (l < 1 || l > a.num_lags) continue;
            org = a.ring + (size_t) s * (size_t) (G * 6);
        }
        long long* const row = a.table + (size_t) l * (size_t) a.row_words;
        if (c == 0) row[0] = row[0] + 1;
        double term;
        if (cls < ND) {
            if (l == 0) continue;
            int g = 0, rest = cls;
            while (rest >= G - g) { rest -= G - g; g++; }            // class (g, h), g <= h, in the order (0,0) (0,1) .. (0,G-1) (1,1) ..
            const int h = g + rest;
            const double dg = (double) (sums[g * 6 + comp] - org[g * 6 + comp]) * a.inv_scale_p;
            const double dh = (double) (sums[h * 6 + comp] - org[h * 6 + comp]) * a.inv_scale_p;
            term = dg * dh;
        } else {
            const int g = (cls - ND) / G, h = (cls - ND) % G;
            const double jg = (double) org[g * 6 + 3 + comp] * a.inv_scale_v;      // the origin is the first index
            const double jh = (double) sums[h * 6 + 3 + comp] * a.inv_scale_v;
            term = jg * jh;
        }
        long long* const cell = row + 1 + c;
        *cell = __double_as_longlong(__longlong_as_double(*cell) + term);
    }
}
__global__ void __launch_bounds__(64) vv_kernel_current_advance(const CurrentArgs a) {
    if (blockIdx.x != 0) return;
    const int lane = threadIdx.x, nw = a.num_groups * 6;
    const long long j = a.words[CUR_SAMPLES], bad = a.words[CUR_BAD];
    const long long s = lane < nw ? a.words[CUR_HEAD + lane] : 0;
    const bool taken = j < a.max_samples;
    if (taken && j % a.origin_every == 0) {
        const int slot = (int) ((j / a.origin_every) % a.num_origins);
        if (bad == 0 && lane < nw) a.ring[(size_t) slot * (size_t) nw + lane] = s;
        if (lane == 0) a.hold[slot] = bad == 0 ? j : -1;
    }
    if (lane < nw) a.words[CUR_HEAD + lane] = 0;
    if (lane != 0) return;
    a.words[CUR_BAD] = 0;
    if (!taken) { a.words[CUR_DROPPED] = a.words[CUR_DROPPED] + 1; return; }
    a.words[CUR_SAMPLES] = j + 1;
    a.words[CUR_OUT_OF_RANGE] = a.words[CUR_OUT_OF_RANGE] + bad;
    if (bad != 0) a.words[CUR_INVALID] = a.words[CUR_INVALID] + 1;
    else a.words[CUR_INV_VOLUME] = __double_as_longlong(__longlong_as_double(a.words[CUR_INV_VOLUME]) + a.inv_volume);
}
__global__ void __launch_bounds__(64) vv_kernel_current_floor(long long* words) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    words[CUR_FLOOR] = words[CUR_SAMPLES];
}
#endif
