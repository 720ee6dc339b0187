// vv_dev_rdf.inc -- part of vv_device.inc: radial distribution functions (vvhip_rdf_*; include/vvhip.h states the sites, the classes, the
// arithmetic and the bins).  Stand-alone kernels that read posq and posqCorrection and write the recorder's own words and scratch, and
// nothing else: no velocity, no force, no accumulator, no thermostat copy, no rendezvous or status word.
//   gather:   one thread per site, striding over a capped grid: X_s in float64 into the planar scratch double[3][stride], ordered by group
//             (the host built the index list at the start).  The pair kernel never touches posq.
//   pairs:    all pairs in tiles, one block of RDF_TILE threads per work item (RdfItem: class, i-tile, a range of j-sites; the host
//             lists, for a class of one group with itself, the j-sites from the i-tile's first on).  A thread keeps its i-site in
//             registers; the j-sites are staged in LDS RDF_TILE at a time as planar doubles and every lane reads the same j: a
//             broadcast, free of bank conflicts.  Per pair and axis d = X_i - X_j, n = rint(d inv_L), d = d - L n, then r2 = (dx dx + dy dy) + dz dz and ONE
//             compare against e(nbins), which most pairs fail; what passes it (in range, or NaN) is masked (the diagonal tile's i < j,
//             the same molecule), counted as invalid if NaN, else binned: the bin is guessed from a float square root and corrected
//             against e(k) = ((double) k dr)^2, so the comparisons of the definition decide it, not the root.  The adds go to the block's
//             private uint32 histogram in LDS (workgroup-scope atomics; a.copies > 1: one histogram per wave), zeroed at block start;
//             the block then adds its non-zero words to the int64 table with agent-scope adds, lane i of a wave word i of a run, as the
//             profile kernel does.  A block counts at most RDF_TILE max_jsites < 2^32 pairs (the launcher refuses otherwise), so no
//             private word wraps.  Integer adds commute: the table is the same bits for any work list, tile shape or arrival order.
//             Every thread reads the sample count from the device-side words; nothing writes that word while this kernel runs.
//   advance:  one thread behind them (the kernel boundary orders it behind every block's read of the count): counts the sample and adds
//             its 1 / V to the sequential float64 sum, or counts it as dropped past max_samples or in a box that no longer holds r_max --
//             no memset node, no host work.
// The tails need no special case: a thread past its tile's last i-site only helps staging, a j past the tile's count is masked by its index, a group
// without sites or a one-site group against itself gives no work item, and a sample without work items runs one idle block and the advance.

__device__ __forceinline__ bool rdf_sample_taken(const RdfArgs& a) {
    if (!a.live) return false;
    const unsigned long long taken = __hip_atomic_load((const unsigned long long*) &a.words[RDF_SAMPLES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return taken < (unsigned long long) a.max_samples;
}

template <class real, class mixed>
__global__ void __launch_bounds__(256) vv_kernel_rdf_gather(const RdfArgs a) {
    using real4 = typename Vec<real>::v4;
    constexpr bool CORR = sizeof(real) != sizeof(mixed);      // mixed precision: the position is posq + posqCorrection, summed in double
    if (!rdf_sample_taken(a)) return;
    double* const x = a.scratch;
    double* const y = x + a.stride;
    double* const z = y + a.stride;
    const long long stride = (long long) gridDim.x * blockDim.x;
    for (long long s = (long long) blockIdx.x * blockDim.x + threadIdx.x; s < a.n; s += stride) {
        const int k = a.index[s];
        const real4 p = ((const real4*) a.posq)[k];
        double c0 = (double) p.x, c1 = (double) p.y, c2 = (double) p.z;
        if (CORR) {
            const real4 q = ((const real4*) a.corr)[k];
            c0 = c0 + (double) q.x; c1 = c1 + (double) q.y; c2 = c2 + (double) q.z;
        }
        x[s] = c0; y[s] = c1; z[s] = c2;
    }
}

template <bool EXCLUDE>
__global__ void __launch_bounds__(RDF_TILE) vv_kernel_rdf_pairs(const RdfArgs a) {
    if ((int) blockIdx.x >= a.num_items || !rdf_sample_taken(a)) return;
    extern __shared__ double vv_dyn_lds[];
    double* const tx = vv_dyn_lds;
    double* const ty = tx + RDF_TILE;
    double* const tz = ty + RDF_TILE;
    int* const tm = (int*) (tz + RDF_TILE);
    unsigned int* const hist = (unsigned int*) (tm + RDF_TILE);
    const int tid = threadIdx.x, nb = a.nbins;
    for (int w = tid; w < a.copies * nb; w += RDF_TILE) hist[w] = 0;      // (the first tile's barrier below orders it in front of every add)
    const RdfItem it = a.items[blockIdx.x];
    const double* const sx = a.scratch;
    const double* const sy = sx + a.stride;
    const double* const sz = sy + a.stride;
    const bool live = tid < it.ni;
    double xi = 0, yi = 0, zi = 0;
    int mi = -1;
    if (live) {
        xi = sx[it.i0 + tid]; yi = sy[it.i0 + tid]; zi = sz[it.i0 + tid];
        if (EXCLUDE) mi = a.mol[it.i0 + tid];
    }
    unsigned int* const h = hist + (a.copies > 1 ? (tid >> 6) * nb : 0);
    const double Lx = a.L[0], Ly = a.L[1], Lz = a.L[2], ix = a.inv_L[0], iy = a.inv_L[1], iz = a.inv_L[2];
    const double dr = a.dr, cut2 = a.cut2;
    const float inv_dr = a.inv_dr;
    auto edge = [dr](int k) { const double t = (double) k * dr; return t * t; };
    long long invalid = 0;
    // one pair that passed the range compare: the masks, NaN, then the bin.  The guess from a float square root is within a bin of the
    // answer (its relative error of a few 2^-24 is 0.002 bins at 8192); one step either way is taken without a branch, and the edges
    // are asked again: should they ever disagree, the loops walk
    auto count = [&](double r2, int j, int jmin, int cnt) {
        if (j < jmin || j >= cnt || (EXCLUDE && mi == tm[j])) return;
        if (r2 != r2) { invalid++; return; }
        int b = min((int) (__builtin_amdgcn_sqrtf((float) r2) * inv_dr), nb - 1);
        b -= (b > 0 && r2 < edge(b)) ? 1 : 0;
        b += (b < nb - 1 && r2 >= edge(b + 1)) ? 1 : 0;
        if (!(edge(b) <= r2 && r2 < edge(b + 1))) {
            while (b > 0 && r2 < edge(b)) b--;
            while (b < nb - 1 && r2 >= edge(b + 1)) b++;
        }
        __hip_atomic_fetch_add(h + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto dist2 = [&](int j) {
        double dx = xi - tx[j], dy = yi - ty[j], dz = zi - tz[j];
        dx = dx - Lx * rint(dx * ix);
        dy = dy - Ly * rint(dy * iy);
        dz = dz - Lz * rint(dz * iz);
        return (dx * dx + dy * dy) + dz * dz;
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
        const int jmin = it.same ? it.i0 + tid + 1 - jbase : 0;      // a class of one group with itself: i < j, by the sites' indices
        // four pairs' arithmetic in flight at a time (independent chains: one wave per SIMD is what a small workload gets), then ONE
        // compare each against e(nbins), which most pairs fail
        for (int j = 0; j < cnt; j += 4) {
            const double r0 = dist2(j), r1 = dist2(j + 1), r2 = dist2(j + 2), r3 = dist2(j + 3);
            if (!(r0 >= cut2)) count(r0, j, jmin, cnt);
            if (!(r1 >= cut2)) count(r1, j + 1, jmin, cnt);
            if (!(r2 >= cut2)) count(r2, j + 2, jmin, cnt);
            if (!(r3 >= cut2)) count(r3, j + 3, jmin, cnt);
        }
    }
    if (invalid) __hip_atomic_fetch_add(&a.words[RDF_INVALID], invalid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    long long* const row = a.words + RDF_HEAD + (size_t) it.cls * (size_t) nb;
    for (int w = tid; w < nb; w += RDF_TILE) {
        long long v = 0;
        for (int c = 0; c < a.copies; c++) v += (long long) hist[c * nb + w];
        if (v != 0) __hip_atomic_fetch_add(row + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

#ifndef VV_DEVICE_NO_PLAIN_KERNELS
__global__ void __launch_bounds__(64) vv_kernel_rdf_advance(const RdfArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (a.live && a.words[RDF_SAMPLES] < a.max_samples) {
        a.words[RDF_SAMPLES] = a.words[RDF_SAMPLES] + 1;
        double s = __longlong_as_double(a.words[RDF_INV_VOLUME]);
        s = s + a.inv_volume;
        a.words[RDF_INV_VOLUME] = __double_as_longlong(s);
    } else
        a.words[RDF_DROPPED] = a.words[RDF_DROPPED] + 1;
}
#endif
