// vv_dev_thermalize.inc -- part of vv_device.inc: Maxwell-Boltzmann start velocities (vvhip_set_velocities_to_temperature).  One stand-alone
// kernel over the plan's wave layout that writes velm.xyz of this plan's particles and nothing else: no velm.w, no position, no force, no
// accumulator, no thermostat state, no rendezvous or status word, no series / CM record.  All arithmetic in double; the store rounds to `mixed`.
//   n(g) = three standard normals of the particle with GLOBAL index g: Philox4x32-10 (vv_dev_misc.inc) on the counter {g, 0, 0, 0x5654}
//          (the tag keeps the stream apart from vv_kernel_fill_normals' 0x5656) under the key {seed low, seed high}, the four words to
//          uniforms u0 = (w0 + 1) 2^-32, u1 = w1 2^-32, u2 = (w2 + 1) 2^-32, u3 = w3 2^-32, then Box-Muller: r0 = sqrt(-2 ln u0),
//          r1 = sqrt(-2 ln u2), n = (r0 cos 2 pi u1, r0 sin 2 pi u1, r1 cos 2 pi u3); the fourth normal is not used.
//   plain:       v = sqrt(R T / m) n(g) for every particle with m > 0.
//   Drude-aware: a pair (d, p) with both masses > 0 gets V = sqrt(R T / M) n(p) and w = sqrt(R T_D / mu) n(d), M = m_d + m_p,
//                mu = m_d m_p / M, and v_d = V + (m_p / M) w, v_p = V - (m_d / M) w.  Each lane forms both normals itself: the generator is
//                counter based, so only the partner's index and mass come from the partner's lane.  Everybody else as in plain mode.
//   massless:    v = 0, in a lane or (image particles, virtual sites placed from a parent's lane) in the list of the particles without one.
// The result is a function of (seed, g, masses, T, T_D) alone: the same bits whatever the wave layout, the launch shape or the shard split.

__device__ __forceinline__ void therm_normals(uint32_t g, const uint32_t (&key)[2], double (&n)[3]) {
    uint32_t c[4] = {g, 0u, 0u, 0x5654u};
    uint32_t k[2] = {key[0], key[1]};
#pragma unroll
    for (int r = 0; r < 10; r++) {
        philox_round(c, k);
        k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
    }
    const double s = 2.3283064365386963e-10;      // 2^-32
    const double u0 = ((double) c[0] + 1.0) * s, u1 = (double) c[1] * s, u2 = ((double) c[2] + 1.0) * s, u3 = (double) c[3] * s;
    const double r0 = sqrt(-2.0 * log(u0)), r1 = sqrt(-2.0 * log(u2));
    double s0, c0;
    sincos(6.283185307179586 * u1, &s0, &c0);
    n[0] = r0 * c0; n[1] = r0 * s0; n[2] = r1 * cos(6.283185307179586 * u3);
}

template <class real, class mixed>
__global__ void __launch_bounds__(512) vv_kernel_thermalize(const ThermalizeArgs a) {
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    const uint32_t key[2] = {a.key[0], a.key[1]};
    for (int wave = blockIdx.x * wpb + (threadIdx.x >> 6); wave < a.nwaves; wave += gridDim.x * wpb) {      // (uniform in the wave)
        const size_t k = (size_t) wave * 64 + lane;
        const int2 slot = a.slots[k];
        const double m = a.lane_mass[k];
        const unsigned meta = (unsigned) slot.y;
        const int partner = (meta >> META_PARTNER_SHIFT) & 63;
        const double pm = shfl(m, partner);                    // (every lane of the wave takes part)
        const int patom = __shfl(slot.x, partner, 64);
        if (slot.x < 0) continue;                              // idle lane: nothing stored
        double v[3] = {0, 0, 0};
        if (m > 0) {
            const uint32_t g = (uint32_t) (a.shard_begin + slot.x);
            double n[3];
            therm_normals(g, key, n);
            if (a.drude_aware && (meta & META_PAIR) && partner != lane && patom >= 0 && pm > 0) {
                const bool isd = (meta & META_IS_DRUDE) != 0;
                double o[3];
                therm_normals((uint32_t) (a.shard_begin + patom), key, o);
                const double md = isd ? m : pm, mp = isd ? pm : m, M = md + mp, mu = md * mp / M;
                const double sV = sqrt(a.kt / M), sw = sqrt(a.kt_drude / mu), f = isd ? mp / M : -(md / M);
                for (int q = 0; q < 3; q++) {
                    const double V = sV * (isd ? o[q] : n[q]), w = sw * (isd ? n[q] : o[q]);
                    v[q] = V + f * w;
                }
            } else {
                const double sd = sqrt(a.kt / m);
                for (int q = 0; q < 3; q++) v[q] = sd * n[q];
            }
        }
        mixed* out = (mixed*) a.velm + 4 * (size_t) slot.x;
        out[0] = (mixed) v[0]; out[1] = (mixed) v[1]; out[2] = (mixed) v[2];
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.nlaneless; i += gridDim.x * blockDim.x) {
        mixed* out = (mixed*) a.velm + 4 * (size_t) a.laneless[i];
        out[0] = 0; out[1] = 0; out[2] = 0;
    }
}
