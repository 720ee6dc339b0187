// vv_dev_report.inc -- part of vv_device.inc: the Drude temperature report (vvhip_drude_temperatures).  Two stand-alone kernels that
// read velm and the plan's slot table and write nothing but their own scratch (ReportArgs::mol_p / out): no accumulator, no thermostat
// state, no status word of the step.
//   pass 1, one wave per 64 slots: m|v|^2 of every massive lane; mu|v_d - v_c|^2 on the Drude lane of a pair inside one molecule (the
//           parent's velocity comes from its lane: a pair always shares a wave, META_PARTNER_SHIFT); the momentum of every molecule,
//           summed over the lanes of the wave that belong to it (a molecule may be spread over several waves) and added to its words.
//   pass 2, one thread per molecule: |P|^2 / M; then the pairs whose two particles lie in different molecules, mu|u_d - u_c|^2 with
//           u = v - P/M of the particle's own molecule.
// Every term goes to fixed point on its own (vv_args.hpp: ReportArgs) before anything is added, so the sums are the same bits whatever
// the launch shape, the wave layout or the split of the particles over shards.

__device__ __forceinline__ void rep_split(double x, const ReportArgs& a, long long& hi, long long& lo, bool& bad) {
    if (!(fabs(x) < a.limit)) { bad = true; hi = 0; lo = 0; return; }      // (NaN included)
    const double y = x * a.unit, f = floor(y);                            // (exact: a power of two)
    hi = (long long) f;
    lo = (long long) rint((y - f) * a.frac_scale);                        // y - floor(y) is exact; lo in [0, 2^frac_bits]
}
__device__ __forceinline__ double rep_join(long long hi, long long lo, const ReportArgs& a) {
    return (double) (hi + (lo >> a.frac_bits)) * a.inv_unit + (double) (lo & ((1ll << a.frac_bits) - 1)) * a.inv_full;
}
__device__ __forceinline__ long long rep_wave_sum(long long x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
// block total of four words -> four atomics into out[w0], out[w0 + 1], out[w1], out[w1 + 1]
__device__ __forceinline__ void rep_block_add(long long s[4], long long* out, int w0, int w1) {
    __shared__ long long part[8][4];
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    for (int q = 0; q < 4; q++) {
        const long long t = rep_wave_sum(s[q]);
        if (lane == 0) part[wib][q] = t;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        long long t = 0;
        for (int w = 0; w < wpb; w++) t += part[w][threadIdx.x];
        const int word = threadIdx.x < 2 ? w0 + threadIdx.x : w1 + threadIdx.x - 2;
        if (t) atomicAdd((unsigned long long*) &out[word], (unsigned long long) t);
    }
}

template <class real, class mixed>
__global__ void __launch_bounds__(512) vv_kernel_report_lanes(const ReportArgs a) {
    using mixed4 = typename Vec<mixed>::v4;
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    long long s[4] = {0, 0, 0, 0};          // m|v|^2 (hi, lo), mu|v_d - v_c|^2 (hi, lo)
    bool bad = false;
    for (int wave = blockIdx.x * wpb + (threadIdx.x >> 6); wave < a.nwaves; wave += gridDim.x * wpb) {      // (uniform in the wave)
        const size_t k = (size_t) wave * 64 + lane;
        const int2 slot = a.slots[k];
        const int mol = a.lane_mol[k];
        const double m = a.lane_mass[k], mu = a.lane_mu[k];
        double vx = 0, vy = 0, vz = 0;
        if (slot.x >= 0) { const mixed4 v = ((const mixed4*) a.velm)[slot.x]; vx = (double) v.x; vy = (double) v.y; vz = (double) v.z; }
        const int partner = ((unsigned) slot.y >> META_PARTNER_SHIFT) & 63;
        const double px = shfl(vx, partner), py = shfl(vy, partner), pz = shfl(vz, partner);
        long long hi, lo;
        if (m > 0) { rep_split(m * (vx * vx + vy * vy + vz * vz), a, hi, lo, bad); s[0] += hi; s[1] += lo; }
        if (mu > 0) {
            const double dx = vx - px, dy = vy - py, dz = vz - pz;
            rep_split(mu * (dx * dx + dy * dy + dz * dz), a, hi, lo, bad); s[2] += hi; s[3] += lo;
        }
        long long w[6] = {0, 0, 0, 0, 0, 0};
        if (mol >= 0) { rep_split(m * vx, a, w[0], w[1], bad); rep_split(m * vy, a, w[2], w[3], bad); rep_split(m * vz, a, w[4], w[5], bad); }
        // one round per molecule present in the wave: its lanes' words summed over the wave, one atomic per word
        unsigned long long todo = __ballot(mol >= 0);
        while (todo) {
            const int leader = __builtin_ctzll(todo);
            const int lm = __shfl(mol, leader, 64);
            const bool in = mol == lm;
            todo &= ~(unsigned long long) __ballot(in);
            for (int q = 0; q < 6; q++) {
                const long long t = rep_wave_sum(in ? w[q] : 0);
                if (lane == leader && t) atomicAdd((unsigned long long*) &a.mol_p[(size_t) lm * 6 + q], (unsigned long long) t);
            }
        }
    }
    if (bad) atomicOr((unsigned long long*) &a.out[REP_FLAG], 1ull);
    rep_block_add(s, a.out, REP_TOTAL, REP_DRUDE);
}

template <class real, class mixed>
__global__ void __launch_bounds__(512) vv_kernel_report_molecules(const ReportArgs a) {
    using mixed4 = typename Vec<mixed>::v4;
    long long s[4] = {0, 0, 0, 0};          // |P|^2/M (hi, lo), mu|u_d - u_c|^2 of the pairs across molecules (hi, lo)
    bool bad = false;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.nmol + a.ncross; i += gridDim.x * blockDim.x) {
        long long hi, lo;
        if (i < a.nmol) {
            const long long* P = a.mol_p + (size_t) i * 6;
            const double px = rep_join(P[0], P[1], a), py = rep_join(P[2], P[3], a), pz = rep_join(P[4], P[5], a);
            rep_split((px * px + py * py + pz * pz) / a.mol_mass[i], a, hi, lo, bad);
            s[0] += hi; s[1] += lo;
        } else {
            const int4 c = a.cross[i - a.nmol];
            const mixed4 vd = ((const mixed4*) a.velm)[c.x], vc = ((const mixed4*) a.velm)[c.y];
            double V[2][3] = {{0, 0, 0}, {0, 0, 0}};
            for (int e = 0; e < 2; e++) {
                const int mol = e == 0 ? c.z : c.w;
                if (mol < 0) continue;
                const long long* P = a.mol_p + (size_t) mol * 6;
                const double M = a.mol_mass[mol];
                V[e][0] = rep_join(P[0], P[1], a) / M; V[e][1] = rep_join(P[2], P[3], a) / M; V[e][2] = rep_join(P[4], P[5], a) / M;
            }
            const double dx = ((double) vd.x - V[0][0]) - ((double) vc.x - V[1][0]);
            const double dy = ((double) vd.y - V[0][1]) - ((double) vc.y - V[1][1]);
            const double dz = ((double) vd.z - V[0][2]) - ((double) vc.z - V[1][2]);
            rep_split(a.cross_mu[i - a.nmol] * (dx * dx + dy * dy + dz * dz), a, hi, lo, bad);
            s[2] += hi; s[3] += lo;
        }
    }
    if (bad) atomicOr((unsigned long long*) &a.out[REP_FLAG], 1ull);
    rep_block_add(s, a.out, REP_COM, REP_DRUDE);
}

// Series row (vvhip_series_*): block 0 appends one row at the device-side cursor -- the report's result words (then zeroes them), the
// thermostat copy current after the step, the box and the cos acceleration -- or counts it as dropped past capacity; every block zeroes
// its share of the report's momentum words, so the next row's passes start from clean scratch without a memset in the stream.
// (Pass 2 cannot zero the momentum words itself: a pair across two molecules reads another molecule's words in the same pass.)
#ifndef VV_DEVICE_NO_PLAIN_KERNELS
__global__ void __launch_bounds__(256) vv_kernel_series_append(const SeriesArgs a) {
    constexpr int W = (int) (sizeof(vvhip_series_row) / 8), NHW = (int) (sizeof(vvhip_nh_state) / 8);
    constexpr int OFF_NH = (int) (__builtin_offsetof(vvhip_series_row, nh) / 8), OFF_BOX = (int) (__builtin_offsetof(vvhip_series_row, box) / 8);
    static_assert(__builtin_offsetof(vvhip_series_row, drude_raw) == 0 && __builtin_offsetof(vvhip_series_row, drude_overflow) == 8 * REP_FLAG, "row layout");
    static_assert(OFF_BOX == OFF_NH + NHW && W == OFF_BOX + 4, "row layout");
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {
        const unsigned long long c = a.cursor[0];
        long long w = 0;
        if (t < REP_WORDS) { if (a.rep_out) w = a.rep_out[t]; }
        else if (t >= OFF_NH && t < OFF_BOX) { if (a.nh) w = ((const long long*) a.nh)[t - OFF_NH]; }
        else if (t >= OFF_BOX && t < W) w = __double_as_longlong(t - OFF_BOX < 3 ? a.box[t - OFF_BOX] : a.cos_acceleration);
        if (c < (unsigned long long) a.capacity && t < W) ((long long*) (a.rows + c))[t] = w;
        if (a.rep_out && t < REP_WORDS) a.rep_out[t] = 0;
        __syncthreads();                                        // (every thread has read the cursor)
        if (t == 0) {
            a.cursor[0] = c + 1;
            if (c >= (unsigned long long) a.capacity) a.cursor[1] = a.cursor[1] + 1;
        }
    }
    if (a.rep_out)
        for (long long i = (long long) blockIdx.x * blockDim.x + t; i < a.rep_mol_words; i += (long long) gridDim.x * blockDim.x) a.rep_mol_p[i] = 0;
}
#endif
