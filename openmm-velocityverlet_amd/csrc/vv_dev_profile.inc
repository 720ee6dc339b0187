// vv_dev_profile.inc -- part of vv_device.inc: density and velocity profiles (vvhip_profile_*; include/vvhip.h states the arithmetic, the
// table's layout and the fixed point).  Two stand-alone kernels that read posq, posqCorrection and velm and write the recorder's own words,
// and nothing else: no force, no accumulator, no thermostat copy, no rendezvous or status word.
//   profile:  one thread per recorded particle, striding over a capped grid.  Per particle one 16- or 32-byte load of posq (and of the
//             correction in mixed precision), one of velm only with a velocity quantity on, a 4-byte index load only with a subset (without
//             one the index is the thread's own), the group byte (GROUPED) and the mass (a mass-weighted quantity on), and one 64-bit
//             integer add per row.  LDS_TABLE (a table of at most 64 KiB): the adds go to the block's private copy in LDS, zeroed at block
//             start; the block then adds its copy to the table, lane i of a wave element i of a run of the table (contiguous 8-byte-per-lane
//             wave instructions), skipping the words that are zero.  Otherwise the adds go to the table directly.  Integer adds commute:
//             the table is the same bits for any grid, block size or arrival order.  Every thread reads the sample count from the
//             device-side words; nothing writes that word while this kernel runs.  At or past max_samples nothing is added.
//   advance:  one thread behind it (the kernel boundary orders it behind every block's read of the count): counts the sample, or counts it
//             as dropped past max_samples -- no memset node, no host work.
// The tails need no special case: the loop bound is the particle count, and a shard without recorded particles runs one idle block and the
// advance.

template <class real, class mixed, bool GROUPED, bool LDS_TABLE>
__global__ void __launch_bounds__(512) vv_kernel_profile(const ProfileArgs a) {
    using real4 = typename Vec<real>::v4;
    using mixed4 = typename Vec<mixed>::v4;
    constexpr bool CORR = sizeof(real) != sizeof(mixed);      // mixed precision: the position is posq + posqCorrection, summed in double
    const unsigned long long taken = __hip_atomic_load((const unsigned long long*) &a.words[PROFILE_SAMPLES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (taken >= (unsigned long long) a.max_samples) return;
    long long* const table = a.words + PROFILE_HEAD;
    long long* acc = table;
    if (LDS_TABLE) {
        extern __shared__ double vv_dyn_lds[];
        acc = (long long*) vv_dyn_lds;
        for (int j = threadIdx.x; j < a.table_words; j += blockDim.x) acc[j] = 0;
        __syncthreads();
    }
    const bool charge = (a.mask & VVHIP_PROFILE_CHARGE) != 0, mass = (a.mask & VVHIP_PROFILE_MASS) != 0;
    const bool momentum = (a.mask & VVHIP_PROFILE_MOMENTUM) != 0, kinetic = (a.mask & VVHIP_PROFILE_KINETIC) != 0;
    const long long stride = (long long) gridDim.x * blockDim.x;
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        int g = 0;
        if (GROUPED) {
            g = a.group[i];
            if (g == 255) continue;
        }
        const int k = a.index ? a.index[i] : (int) i;
        const real4 p = ((const real4*) a.posq)[k];
        double c = (double) (a.axis == 0 ? p.x : a.axis == 1 ? p.y : p.z);
        if (CORR) {
            const real4 q = ((const real4*) a.corr)[k];
            c = c + (double) (a.axis == 0 ? q.x : a.axis == 1 ? q.y : q.z);
        }
        const double t = c * a.inv_L;
        const double u = t - floor(t);
        int b = (int) (u * (double) a.nbins);
        b = max(0, min(b, a.nbins - 1));                      // (0: only a coordinate that is NaN or infinite gets there)
        // every enabled term first: one that is NaN or out of range leaves the particle out of every row
        long long wq = 0, wm = 0, wpx = 0, wpy = 0, wpz = 0, wk = 0;
        bool bad = false;
        auto fixed = [&](double x, int q) {
            bad = bad || !(fabs(x) < a.limit[q]);
            return llrint(x * a.scale[q]);
        };
        if (charge) wq = fixed((double) p.w, 0);
        if (mass || momentum || kinetic) {
            const double m = a.mass[i];
            if (mass) wm = fixed(m, 1);
            if (momentum || kinetic) {
                const mixed4 vm = ((const mixed4*) a.velm)[k];
                const double vx = (double) vm.x, vy = (double) vm.y, vz = (double) vm.z;
                if (momentum) { wpx = fixed(m * vx, 2); wpy = fixed(m * vy, 2); wpz = fixed(m * vz, 2); }
                if (kinetic) wk = fixed(m * ((vx * vx + vy * vy) + vz * vz), 3);
            }
        }
        if (bad) {
            __hip_atomic_fetch_add(&a.words[PROFILE_OUT_OF_RANGE], 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        // ... then the rows in the table's order
        long long* at = acc + (size_t) g * (size_t) a.rows * (size_t) a.nbins + b;
        auto add = [&](long long v) {
            if (LDS_TABLE) __hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else __hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            at += a.nbins;
        };
        add(1);
        if (charge) add(wq);
        if (mass) add(wm);
        if (momentum) { add(wpx); add(wpy); add(wpz); }
        if (kinetic) add(wk);
    }
    if (LDS_TABLE) {
        __syncthreads();
        for (int j = threadIdx.x; j < a.table_words; j += blockDim.x) {
            const long long v = acc[j];
            if (v != 0) __hip_atomic_fetch_add(table + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

#ifndef VV_DEVICE_NO_PLAIN_KERNELS
__global__ void __launch_bounds__(64) vv_kernel_profile_advance(const ProfileArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (a.words[PROFILE_SAMPLES] < a.max_samples) a.words[PROFILE_SAMPLES] = a.words[PROFILE_SAMPLES] + 1;
    else a.words[PROFILE_DROPPED] = a.words[PROFILE_DROPPED] + 1;
}
#endif
