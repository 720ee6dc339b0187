// vv_dev_sdf.inc -- part of vv_device.inc: spatial distribution functions (vvhip_sdf_*; include/vvhip.h states the frames, the sites, the
// classes, the arithmetic and the voxels).  Stand-alone kernels that read posq and posqCorrection and write the recorder's own words and
// scratch, and nothing else: no velocity, no force, no accumulator, no thermostat copy, no rendezvous or status word.
//   gather:   one thread per site and per frame, striding over a capped grid.  A site: X_s in float64 into the planar scratch
//             double[3][stride], ordered by site group -- the RDF's gather.  A frame (ordered by frame group): X_o, X_a, X_b from posq, the
//             Gram-Schmidt steps of the definition through acf_inverse_norm, and 13 planes double[13][fstride] behind the sites': origin,
//             e1, e2, e3 and the frame's own cutoff for the pair kernel's cheap test (below).  A bad frame (n1 or n2 NaN or outside
//             [2^-40, 2^40)) is stored as 13 NaNs; a good frame's origin is finite (n1 is), so "origin x is NaN" IS the bad-frame flag.
//             Good frames add to frame_visits[g], bad ones to bad_frames: one add per wave where the wave's frames share a group.
//   pairs:    the RDF's tiling with frames for i-sites: one block of RDF_TILE threads per work item (RdfItem: class, i-tile of frames, a
//             range of j-sites of the class's site group).  A thread keeps its frame in registers (13 doubles); the j-sites are staged in
//             LDS RDF_TILE at a time as planar doubles and every lane reads the same j: a broadcast, free of bank conflicts.  Per pair
//             and axis d = X_s - X_o, n = rint(d inv_L), d = d - L n, then r2 = (dx dx + dy dy) + dz dz and ONE compare against the
//             frame's cutoff, which most pairs fail.  What passes it (or is NaN) is masked (the tile's tail, the frame's own molecule),
//             then takes the definition's path: xi_k = (dx e_kx + dy e_ky) + dz e_kz, u_k = (xi_k + h) inv_w, a NaN counts as invalid,
//             0 <= u_k < n on all three axes decides, (int) u_k is the voxel, and the int64 word gets an agent-scope relaxed add.  No
//             private histogram: a few percent of the pairs are in range and the table does not fit a block's LDS beyond n ~ 25.
//             The cheap test is conservative.  xi = E d with the rows e_k, so |xi|^2 >= lambda_min(E E^T) r2, and Gershgorin bounds
//             lambda_min from below by 1 - delta, delta = the largest row sum of |E E^T - 1|, which the gather forms from the e_k as
//             stored.  A pair in range has |xi_k| <= h (1 + a few 2^-53) on every axis, so r2 <= 3 h^2 / (1 - delta) up to rounding;
//             the frame's cutoff is 3 h^2 (1 + 2^-20) / (1 - delta), the factor covering the roundings of r2, xi, u and delta (each a
//             few 2^-53 relative), and +inf -- no cheap test -- where delta is not below 1/2.
//   advance:  one thread behind them (the kernel boundary orders it behind every block's read of the count): counts the sample and adds
//             its 1 / V to the sequential float64 sum, or counts it as dropped past max_samples or in a box that no longer holds the
//             cube -- no memset node, no host work.
// The tails need no special case: a thread past its tile's last frame, or with a bad frame, only helps staging; a j past the tile's count
// is masked by its index; a class with an empty group gives no work item, and a sample without work items runs one idle block and the
// advance.  Integer adds commute: the table is the same bits for any work list, tile shape or arrival order.

__device__ __forceinline__ bool sdf_sample_taken(const SdfArgs& a) {
    if (!a.live) return false;
    const unsigned long long taken = __hip_atomic_load((const unsigned long long*) &a.words[SDF_SAMPLES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return taken < (unsigned long long) a.max_samples;
}

template <class real, class mixed>
__global__ void __launch_bounds__(256) vv_kernel_sdf_gather(const SdfArgs a) {
    using real4 = typename Vec<real>::v4;
    constexpr bool CORR = sizeof(real) != sizeof(mixed);      // mixed precision: the position is posq + posqCorrection, summed in double
    if (!sdf_sample_taken(a)) return;
    auto position = [&](int k, double c[3]) {
        const real4 p = ((const real4*) a.posq)[k];
        c[0] = (double) p.x; c[1] = (double) p.y; c[2] = (double) p.z;
        if (CORR) {
            const real4 q = ((const real4*) a.corr)[k];
            c[0] = c[0] + (double) q.x; c[1] = c[1] + (double) q.y; c[2] = c[2] + (double) q.z;
        }
    };
    double* const x = a.scratch;
    double* const y = x + a.stride;
    double* const z = y + a.stride;
    double* const fr = a.scratch + 3 * (size_t) a.stride;      // the frames' planes
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const long long total = (long long) a.n + a.nf;
    const long long stride = (long long) gridDim.x * blockDim.x;
    for (long long s = (long long) blockIdx.x * blockDim.x + threadIdx.x; s < total; s += stride) {
        if (s < a.n) {
            double c[3];
            position(a.index[s], c);
            x[s] = c[0]; y[s] = c[1]; z[s] = c[2];
            continue;
        }
        const int f = (int) (s - a.n);
        double o[3], p[3], q[3];
        position(a.frames[3 * f], o); position(a.frames[3 * f + 1], p); position(a.frames[3 * f + 2], q);
        for (int k = 0; k < 3; k++) { p[k] = p[k] - o[k]; q[k] = q[k] - o[k]; }
        double e1[3], e2[3], e3[3], cut = nan;
        const double n1 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
        bool good = n1 >= 0x1p-40 && n1 < 0x1p40;                                                // (false for a NaN)
        if (good) {
            const double y1 = acf_inverse_norm(n1);
            for (int k = 0; k < 3; k++) e1[k] = p[k] * y1;
            const double t = (q[0] * e1[0] + q[1] * e1[1]) + q[2] * e1[2];
            double w[3];
            for (int k = 0; k < 3; k++) w[k] = q[k] - t * e1[k];
            const double n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
            good = n2 >= 0x1p-40 && n2 < 0x1p40;
            if (good) {
                const double y2 = acf_inverse_norm(n2);
                for (int k = 0; k < 3; k++) e2[k] = w[k] * y2;
                e3[0] = e1[1] * e2[2] - e1[2] * e2[1];
                e3[1] = e1[2] * e2[0] - e1[0] * e2[2];
                e3[2] = e1[0] * e2[1] - e1[1] * e2[0];
                // the cheap test's cutoff (the head of this file): Gershgorin's bound on E E^T as stored
                auto dot = [](const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; };
                const double g12 = fabs(dot(e1, e2)), g13 = fabs(dot(e1, e3)), g23 = fabs(dot(e2, e3));
                const double d1 = fabs(dot(e1, e1) - 1.0) + g12 + g13, d2 = fabs(dot(e2, e2) - 1.0) + g12 + g23, d3 = fabs(dot(e3, e3) - 1.0) + g13 + g23;
                const double delta = fmax(d1, fmax(d2, d3));
                cut = delta < 0.5 ? a.cut2 / (1.0 - delta) : __longlong_as_double(0x7FF0000000000000ll);
            }
        }
        if (!good)
            for (int k = 0; k < 3; k++) { o[k] = nan; e1[k] = nan; e2[k] = nan; e3[k] = nan; }
        double* const at = fr + f;
        for (int k = 0; k < 3; k++) {
            at[(size_t) k * a.fstride] = o[k]; at[(size_t) (3 + k) * a.fstride] = e1[k];
            at[(size_t) (6 + k) * a.fstride] = e2[k]; at[(size_t) (9 + k) * a.fstride] = e3[k];
        }
        at[(size_t) 12 * a.fstride] = cut;
        // the counts: the lanes that are here hold frames (a wave's lanes with sites took the other branch); one add per wave where they
        // share a group, which the order by group makes the rule
        const int g = a.fgroup[f];
        const int g0 = __builtin_amdgcn_readfirstlane(g);
        const unsigned long long here = __ballot(1), mixed_groups = __ballot(g != g0), ok = __ballot(good);
        if (mixed_groups == 0) {
            if ((int) __lane_id() == __ffsll((long long) here) - 1) {
                const long long n_good = __popcll(ok), n_bad = __popcll(here & ~ok);
                if (n_good) __hip_atomic_fetch_add(&a.words[SDF_VISITS + g0], n_good, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (n_bad) __hip_atomic_fetch_add(&a.words[SDF_BAD_FRAMES], n_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else
            __hip_atomic_fetch_add(&a.words[good ? SDF_VISITS + g : SDF_BAD_FRAMES], 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool EXCLUDE>
__global__ void __launch_bounds__(RDF_TILE) vv_kernel_sdf_pairs(const SdfArgs a) {
    if ((int) blockIdx.x >= a.num_items || !sdf_sample_taken(a)) return;
    extern __shared__ double vv_dyn_lds[];
    double* const tx = vv_dyn_lds;
    double* const ty = tx + RDF_TILE;
    double* const tz = ty + RDF_TILE;
    int* const tm = (int*) (tz + RDF_TILE);
    const int tid = threadIdx.x, nb = a.nbins;
    const RdfItem it = a.items[blockIdx.x];
    const double* const sx = a.scratch;
    const double* const sy = sx + a.stride;
    const double* const sz = sy + a.stride;
    const double* const fr = a.scratch + 3 * (size_t) a.stride + it.i0 + tid;
    bool live = tid < it.ni;
    double ox = 0, oy = 0, oz = 0, e1x = 0, e1y = 0, e1z = 0, e2x = 0, e2y = 0, e2z = 0, e3x = 0, e3y = 0, e3z = 0, cut2 = 0;
    int mi = -1;
    if (live) {
        const size_t fs = (size_t) a.fstride;
        ox = fr[0]; oy = fr[fs]; oz = fr[2 * fs];
        e1x = fr[3 * fs]; e1y = fr[4 * fs]; e1z = fr[5 * fs];
        e2x = fr[6 * fs]; e2y = fr[7 * fs]; e2z = fr[8 * fs];
        e3x = fr[9 * fs]; e3y = fr[10 * fs]; e3z = fr[11 * fs];
        cut2 = fr[12 * fs];
        if (EXCLUDE) mi = a.fmol[it.i0 + tid];
        live = ox == ox;                                          // (a bad frame: it takes part in no pair and reaches no count)
    }
    long long* const table = a.words + SDF_HEAD + (size_t) it.cls * (size_t) nb * (size_t) nb * (size_t) nb;
    const double Lx = a.L[0], Ly = a.L[1], Lz = a.L[2], ix = a.inv_L[0], iy = a.inv_L[1], iz = a.inv_L[2];
    const double h = a.h, inv_w = a.inv_w, top = (double) nb;
    long long invalid = 0;
    struct D { double x, y, z, r2; };
    auto delta = [&](int j) {
        D d;
        d.x = tx[j] - ox; d.y = ty[j] - oy; d.z = tz[j] - oz;
        d.x = d.x - Lx * rint(d.x * ix);
        d.y = d.y - Ly * rint(d.y * iy);
        d.z = d.z - Lz * rint(d.z * iz);
        d.r2 = (d.x * d.x + d.y * d.y) + d.z * d.z;
        return d;
    };
    // one pair that passed the cheap test: the masks, then the definition's three projections, comparisons and conversions
    auto count = [&](const D& d, int j, int cnt) {
        if (j >= cnt || (EXCLUDE && mi == tm[j])) return;
        const double u1 = (((d.x * e1x + d.y * e1y) + d.z * e1z) + h) * inv_w;
        const double u2 = (((d.x * e2x + d.y * e2y) + d.z * e2z) + h) * inv_w;
        const double u3 = (((d.x * e3x + d.y * e3y) + d.z * e3z) + h) * inv_w;
        if (u1 != u1 || u2 != u2 || u3 != u3) { invalid++; return; }
        if (!(u1 >= 0.0 && u1 < top && u2 >= 0.0 && u2 < top && u3 >= 0.0 && u3 < top)) return;
        const size_t v = ((size_t) (int) u1 * (size_t) nb + (size_t) (int) u2) * (size_t) nb + (size_t) (int) u3;
        __hip_atomic_fetch_add(table + v, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    for (int jb = it.j0; jb < it.j1; jb += RDF_TILE) {
        const int jbase = it.b0 + jb;
        const int cnt = min(RDF_TILE, it.j1 - jb);
        __syncthreads();                                          // (the tile before this one has been read by every wave)
        // (zeros behind the tile's last site: the loop below runs in fours and masks them by their index)
        tx[tid] = tid < cnt ? sx[jbase + tid] : 0.0; ty[tid] = tid < cnt ? sy[jbase + tid] : 0.0; tz[tid] = tid < cnt ? sz[jbase + tid] : 0.0;
        if (EXCLUDE) tm[tid] = tid < cnt ? a.mol[jbase + tid] : -2;
        __syncthreads();
        if (!live) continue;
        // four pairs' arithmetic in flight at a time (independent chains), then ONE compare each, which most pairs fail
        for (int j = 0; j < cnt; j += 4) {
            const D d0 = delta(j), d1 = delta(j + 1), d2 = delta(j + 2), d3 = delta(j + 3);
            if (!(d0.r2 >= cut2)) count(d0, j, cnt);
            if (!(d1.r2 >= cut2)) count(d1, j + 1, cnt);
            if (!(d2.r2 >= cut2)) count(d2, j + 2, cnt);
            if (!(d3.r2 >= cut2)) count(d3, j + 3, cnt);
        }
    }
    if (invalid) __hip_atomic_fetch_add(&a.words[SDF_INVALID], invalid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#ifndef VV_DEVICE_NO_PLAIN_KERNELS
__global__ void __launch_bounds__(64) vv_kernel_sdf_advance(const SdfArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (a.live && a.words[SDF_SAMPLES] < a.max_samples) {
        a.words[SDF_SAMPLES] = a.words[SDF_SAMPLES] + 1;
        double s = __longlong_as_double(a.words[SDF_INV_VOLUME]);
        s = s + a.inv_volume;
        a.words[SDF_INV_VOLUME] = __double_as_longlong(s);
    } else
        a.words[SDF_DROPPED] = a.words[SDF_DROPPED] + 1;
}
#endif
