// vv_dev_cmm.inc -- part of vv_device.inc: removal of the centre-of-mass velocity (vvhip_cm_motion_*, vvhip_remove_cm_motion).  Two
// stand-alone kernels over the plan's wave layout that touch velm.xyz of the massive lanes, their own scratch (CmmArgs::words) and
// their own record, and nothing else: no position, no velm.w, no force, no accumulator, no thermostat state, no status word.
//   sum:      m v of every massive lane per component, each term to the report's two-word fixed point on its own (rep_split), wave and
//             block reduction, one integer atomic per word and block.  A term out of range (NaN included) raises the bad word.
//   subtract: wave 0 of every block fetches the seven words for its block, every thread forms V = P / M from them (the same words and
//             the same arithmetic in every thread: the same bits) and subtracts it from its lanes' velocities in `mixed`; massless and
//             idle lanes store nothing; with the bad word raised nothing is subtracted at all.  Thread 0 of block 0 keeps the record.
//             The block that is the last to have fetched the words (a ticket per block) zeroes them: the scratch is zero again when the
//             kernel ends, without a memset in the stream (and so inside a captured graph without a memset node).
// Nothing between the two but the kernel boundary: no host synchronisation, no copy.

__device__ __forceinline__ void cmm_block_add(long long s[6], long long* words) {
    __shared__ long long part[8][6];
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    for (int q = 0; q < 6; q++) {
        const long long t = rep_wave_sum(s[q]);
        if (lane == 0) part[wib][q] = t;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        long long t = 0;
        for (int w = 0; w < wpb; w++) t += part[w][threadIdx.x];
        if (t) atomicAdd((unsigned long long*) &words[threadIdx.x], (unsigned long long) t);
    }
}

template <class real, class mixed>
__global__ void __launch_bounds__(512) vv_kernel_cmm_sum(const CmmArgs a) {
    using mixed4 = typename Vec<mixed>::v4;
    const ReportArgs& r = a.rep;
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    long long s[6] = {0, 0, 0, 0, 0, 0};      // (hi, lo) of sum m vx, m vy, m vz
    bool bad = false;
    for (int wave = blockIdx.x * wpb + (threadIdx.x >> 6); wave < r.nwaves; wave += gridDim.x * wpb) {      // (uniform in the wave)
        const size_t k = (size_t) wave * 64 + lane;
        const int2 slot = r.slots[k];
        const double m = r.lane_mass[k];
        if (slot.x < 0 || !(m > 0)) continue;
        const mixed4 v = ((const mixed4*) r.velm)[slot.x];
        long long hi, lo;
        rep_split(m * (double) v.x, r, hi, lo, bad); s[0] += hi; s[1] += lo;
        rep_split(m * (double) v.y, r, hi, lo, bad); s[2] += hi; s[3] += lo;
        rep_split(m * (double) v.z, r, hi, lo, bad); s[4] += hi; s[5] += lo;
    }
    if (bad) atomicOr((unsigned long long*) &a.words[CMM_BAD], 1ull);
    cmm_block_add(s, a.words);
}

template <class real, class mixed>
__global__ void __launch_bounds__(512) vv_kernel_cmm_subtract(const CmmArgs a) {
    using mixed4 = typename Vec<mixed>::v4;
    const ReportArgs& r = a.rep;
    __shared__ long long w[CMM_WORDS];
    // (one wave fetches for the block: its loads have returned before it writes them to LDS, hence before thread 0 takes the ticket below)
    if (threadIdx.x < CMM_TICKET) w[threadIdx.x] = __hip_atomic_load(&a.words[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const bool bad = w[CMM_BAD] != 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double Vx = bad ? nan : rep_join(w[0], w[1], r) * a.inv_total_mass;
    const double Vy = bad ? nan : rep_join(w[2], w[3], r) * a.inv_total_mass;
    const double Vz = bad ? nan : rep_join(w[4], w[5], r) * a.inv_total_mass;
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned long long t = atomicAdd((unsigned long long*) &a.words[CMM_TICKET], 1ull);
        if (t + 1 == (unsigned long long) gridDim.x)          // every block has fetched the words: clean scratch for the next removal
            for (int q = 0; q < CMM_WORDS; q++) (void) atomicExch((unsigned long long*) &a.words[q], 0ull);
        if (blockIdx.x == 0) {
            if (bad) a.rec->skipped = a.rec->skipped + 1;
            else a.rec->removals = a.rec->removals + 1;
            a.rec->last_v[0] = Vx; a.rec->last_v[1] = Vy; a.rec->last_v[2] = Vz;
        }
    }
    if (bad) return;
    const mixed ux = (mixed) Vx, uy = (mixed) Vy, uz = (mixed) Vz;
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    for (int wave = blockIdx.x * wpb + (threadIdx.x >> 6); wave < r.nwaves; wave += gridDim.x * wpb) {
        const size_t k = (size_t) wave * 64 + lane;
        const int2 slot = r.slots[k];
        if (slot.x < 0 || !(r.lane_mass[k] > 0)) continue;
        mixed4 v = ((const mixed4*) r.velm)[slot.x];
        v.x -= ux; v.y -= uy; v.z -= uz;
        ((mixed4*) r.velm)[slot.x] = v;
    }
}
