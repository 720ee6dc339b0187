// vv_dev_misc.inc -- part of vv_device.inc: mass tables, stand-alone image kernel, synthetic force provider, device Gaussian numbers
// ================================================================================ static mass tables
// One launch per binding: slot_m = RECIP(velm.w) and, for the two lanes of a Drude pair, slot_f = invTotalMass * own mass with
// invTotalMass = RECIP(mass1 + mass2) -- the operations of K/drudeNoseHoover.cu:173-180 / K/drudeLangevin.cu:16,36-44 in the mode's
// `mixed` type, so that the stages reading the tables get the very bits they used to recompute in every step.
template <class real, class mixed>
__global__ void __launch_bounds__(256) vv_kernel_mass_table(const void* velm_, const int2* slots, int nwaves, double* slot_m, double* slot_f) {
    using mixed4 = typename Vec<mixed>::v4;
    using P = Prec<real>;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (wave >= nwaves) return;
    const int2 slot = slots[(size_t) wave * 64 + lane];
    const unsigned meta = (unsigned) slot.y;
    const int partner = (meta >> META_PARTNER_SHIFT) & 63;
    mixed w = 0;
    if (slot.x >= 0) w = ((const mixed4*) velm_)[slot.x].w;
    const mixed m = w != 0 ? P::RECIP(w) : (mixed) 0;
    const mixed pm = shfl(m, partner);
    mixed f = 0;
    if (slot.x >= 0 && (meta & META_PAIR)) {
        const bool isd = (meta & META_IS_DRUDE) != 0;
        const mixed mass1 = isd ? m : pm, mass2 = isd ? pm : m;        // 1 = Drude, 2 = parent: the reference's operand order
        const mixed invTotalMass = P::RECIP(mass1 + mass2);
        f = invTotalMass * m;
    }
    slot_m[(size_t) wave * 64 + lane] = (double) m;
    slot_f[(size_t) wave * 64 + lane] = (double) f;
}

// ================================================================================ stand-alone image kernel
// vvhip_update_image_positions when called on its own (ModifyImageChargeKernel::updateImagePositions).
template <class real, class mixed>
__global__ void __launch_bounds__(256) vv_kernel_images(void* posq_, void* corr_, const int2* pairs, int npairs, double mirror) {
    using real4 = typename Vec<real>::v4;
    constexpr bool kMixed = sizeof(real) != sizeof(mixed);
    real4* posq = (real4*) posq_;
    real4* corr = (real4*) corr_;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += blockDim.x * gridDim.x) {
        const int2 pr = pairs[i];
        const real4 pp = posq[pr.y];
        real4 pi = posq[pr.x];
        pi.x = pp.x; pi.y = pp.y;
        if (kMixed) {
            const real4 cp = corr[pr.y];
            real4 ci = corr[pr.x];
            ci.x = cp.x; ci.y = cp.y;
            mixed z = (mixed) pp.z + (mixed) cp.z;
            z = (mixed) mirror * 2 - z;
            pi.z = (real) z;
            ci.z = (real) (z - (real) z);
            corr[pr.x] = ci;
        } else {
            pi.z = 2 * (mixed) mirror - pp.z;
        }
        posq[pr.x] = pi;
    }
}

// ================================================================================ synthetic force provider (bench/test support)
// Mirrors oracle vvo_tether_force bit for bit: tether on massive particles, Drude-parent spring, both
// converted to fixed point by truncation and then added as integers.
template <class real, class mixed>
__global__ void __launch_bounds__(512) vv_kernel_tether(const int2* __restrict__ pre_slots, const int pre_nwaves, const int pre_wpb, const TetherArgs t) {
    using real4 = typename Vec<real>::v4;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * pre_wpb + (threadIdx.x >> 6);
    if (wave >= pre_nwaves) return;
    [[maybe_unused]] const TetherArgs& a = t;           // (the span macros of the instrumented build read a.dbg_span)
    VV_SPAN_BEGIN;
    const int2 slot = pre_slots[(size_t) wave * 64 + lane];
    const int atom = slot.x;
    const unsigned meta = (unsigned) slot.y;
    const int partner = (meta >> META_PARTNER_SHIFT) & 63;
    const bool act = atom >= 0;
    real4 p = {0, 0, 0, 0}, s = {0, 0, 0, 0};
    const bool w = act && (meta & META_MASSIVE);       // == (velm.w != 0) without touching velm
    if (act) { p = ((const real4*) t.posq)[atom]; s = ((const real4*) t.site)[atom]; }
    const real kt = (real) t.k_tether, kd = (real) t.k_drude, scale = (real) 4294967296.0;
    real fx = 0, fy = 0, fz = 0;
    if (w) { fx = -kt * (p.x - s.x); fy = -kt * (p.y - s.y); fz = -kt * (p.z - s.z); }
    long long ix = (long long) (fx * scale), iy = (long long) (fy * scale), iz = (long long) (fz * scale);
    const real ox = shfl(p.x, partner), oy = shfl(p.y, partner), oz = shfl(p.z, partner);
    if (act && (meta & META_PAIR)) {
        const bool isd = (meta & META_IS_DRUDE) != 0;
        const real dxx = isd ? p.x - ox : ox - p.x, dyy = isd ? p.y - oy : oy - p.y, dzz = isd ? p.z - oz : oz - p.z;
        const long long sx = (long long) (-kd * dxx * scale), sy = (long long) (-kd * dyy * scale), sz = (long long) (-kd * dzz * scale);
        if (isd) { ix += sx; iy += sy; iz += sz; } else { ix -= sx; iy -= sy; iz -= sz; }
    }
    if (act) { t.force[atom] = ix; t.force[atom + t.padded] = iy; t.force[atom + 2 * t.padded] = iz; }
    VV_SPAN_END;
}

// ================================================================================ device Gaussian random numbers
// Philox4x32-10 (Salmon et al., SC'11) counter-based generator + Box-Muller; 4 normals per call = one float4 of the
// buffer the Langevin stage reads.  Not part of the reference (there the buffer is OpenMM's, CudaVVKernels.cpp:63,863).
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], const uint32_t (&k)[2]) {
    const uint64_t p0 = (uint64_t) 0xD2511F53u * c[0], p1 = (uint64_t) 0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t) (p1 >> 32) ^ c[1] ^ k[0], n1 = (uint32_t) p1, n2 = (uint32_t) (p0 >> 32) ^ c[3] ^ k[1], n3 = (uint32_t) p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
#ifndef VV_DEVICE_NO_PLAIN_KERNELS
__global__ void __launch_bounds__(256) vv_kernel_fill_normals(float4* out, uint32_t count, uint64_t seed, const unsigned long long* epoch) {
    const unsigned long long ep = *epoch;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += blockDim.x * gridDim.x) {
        uint32_t c[4] = {i, (uint32_t) ep, (uint32_t) (ep >> 32), 0x5656u};
        uint32_t key[2] = {(uint32_t) seed, (uint32_t) (seed >> 32)};
#pragma unroll
        for (int r = 0; r < 10; r++) {
            philox_round(c, key);
            key[0] += 0x9E3779B9u; key[1] += 0xBB67AE85u;
        }
        // (0,1] uniforms from the 32-bit words, then two Box-Muller pairs
        const float u0 = ((float) c[0] + 1.0f) * 2.3283064365386963e-10f, u1 = (float) c[1] * 2.3283064365386963e-10f;
        const float u2 = ((float) c[2] + 1.0f) * 2.3283064365386963e-10f, u3 = (float) c[3] * 2.3283064365386963e-10f;
        const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
        float s0, c0, s1, c1;
        sincosf(6.283185307179586f * u1, &s0, &c0);
        sincosf(6.283185307179586f * u3, &s1, &c1);
        out[i] = make_float4(r0 * c0, r0 * s0, r1 * c1, r1 * s1);
    }
}
#endif
#ifndef VV_DEVICE_NO_PLAIN_KERNELS
__global__ void vv_kernel_bump_epoch(unsigned long long* epoch) { *epoch += 1; }
#endif
