// vv_dev_vanhove_distinct.inc -- part of vv_device.inc: the distinct part of the van Hove function (vvhip_vanhove_distinct_*;
// include/vvhip.h states the sites, the classes, the schedule of origins and lags, the arithmetic and the bins).  Stand-alone kernels that
// read posq and posqCorrection and write the recorder's own words and planes, and nothing else.  Three launches per sample:
//   gather:   the RDF gather's work: one thread per site, striding over a capped grid, X_s in float64 into planes double[3][stride] for
//             "now".  The ring has R + 1 slots (R = num_origins) and one spare plane set behind them: a sample that is an origin (j mod E
//             == 0) is gathered straight into slot (j / E) mod (R + 1), any other into the spare set.  At sample j the origins that may
//             still be read are k E with j - num_lags <= k E < j, at most R of them, with k in (j / E - R - 1, j / E): R + 1 consecutive
//             k never share a slot, so the slot written now holds none of them -- also when R E == num_lags, where the oldest origin
//             contributes at lag num_lags while the newest is stored.  No copy kernel, and no word that one thread writes and another of
//             the same kernel reads.
//   pairs:    the RDF pair kernel with the i-sites taken from an origin's planes and the j-sites from now: one block of RDF_TILE threads
//             per (work item, slot), grid (items, R + 1).  A thread keeps its i-site in registers; the j-sites are staged in LDS RDF_TILE
//             at a time and every lane reads the same j (a broadcast).  Per pair and axis d = X_j(now) - X_i(origin), n = rint(d inv_L),
//             d = d - L n, r2 = (dx dx + dy dy) + dz dz and ONE compare against e(nbins), which most pairs fail; what passes is masked (a
//             site against its own earlier self where ga == gb, the same molecule), counted as invalid if NaN, else binned by the
//             comparisons against e(k) around a float guess, as for the RDF.  Which origin a slot holds, whether it is alive and which row
//             it feeds follow from the device-side ordinal and floor and are the same for every thread of the grid (vhd_slot); the blocks
//             of a dead slot return before they touch LDS.  Slot (ceil(j / E)) mod (R + 1) can hold no live origin: its blocks count now
//             against now into row 0.  The adds go to the block's private uint32 histogram in LDS (a.copies > 1: one per wave) and from
//             there, where non-zero, as one int64 add each to hist[cls][row]; PLAIN = true (test hook "vhd_lds" = 0) adds every pair to
//             the table directly.  A block counts at most RDF_TILE max_jsites < 2^32 pairs (the launcher refuses otherwise), so no
//             private word wraps.  Integer adds commute: the table is the same bits for any work list, tile shape, histogram layout or
//             arrival order.
//   advance:  one thread behind them (the kernel boundary orders it behind every block's read of ordinal and floor): a visit and 1 / V for
//             row 0 and for the row of every live origin, newest first, then the ordinal; or the sample counted as dropped -- past
//             max_samples nothing else, in a box that no longer holds r_max the floor becomes the ordinal too, which does not advance.
//   floor:    one thread: the origin floor becomes the current ordinal (the box or the positions were rewritten outside the steps).
// The tails need no special case: a thread past its tile's last i-site only helps staging, a j past the tile's count is masked by its
// index, a group without sites or a one-site group against itself gives no work item, and a sample without work items runs R + 1 idle
// blocks and the advance.

// Ordinal and floor as every thread of a sample's kernels reads them; nothing writes these words while the gather or the pair kernel runs.
struct VhdNow { long long j, floor; bool taken; };
__device__ __forceinline__ VhdNow vhd_now(const VhdArgs& a) {
    VhdNow w;
    w.j = (long long) __hip_atomic_load((const unsigned long long*) &a.words[VHD_SAMPLES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    w.floor = (long long) __hip_atomic_load((const unsigned long long*) &a.words[VHD_FLOOR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    w.taken = a.live && w.j < a.max_samples;
    return w;
}
// The plane set that holds the sample taken now: its ring slot where it is an origin, else the spare set behind the ring
__device__ __forceinline__ int vhd_now_set(const VhdArgs& a, long long j) {
    const int E = a.origin_every, R1 = a.num_origins + 1;
    return j % E == 0 ? (int) ((j / E) % R1) : R1;
}
// Grid slot `slot` (0 .. R) at sample j: false if it feeds nothing, else the row it feeds and the plane set of its i-sites
__device__ __forceinline__ bool vhd_slot(const VhdArgs& a, const VhdNow& w, int slot, int* row, int* set) {
    const int E = a.origin_every, R1 = a.num_origins + 1;
    const long long kmax = w.j > 0 ? (w.j - 1) / E : -1;         // the newest origin in front of this sample
    if (slot == (int) ((kmax + 1) % R1)) { *row = 0; *set = vhd_now_set(a, w.j); return true; }
    if (kmax < 0) return false;
    const long long k = kmax - ((kmax - slot) % R1 + R1) % R1;
    if (k < 0 || k * E < w.floor || w.j - k * E > a.num_lags) return false;
    *row = (int) (w.j - k * E); *set = slot;
    return true;
}

template <class real, class mixed>
__global__ void __launch_bounds__(256) vv_kernel_vhd_gather(const VhdArgs a) {
    using real4 = typename Vec<real>::v4;
    constexpr bool CORR = sizeof(real) != sizeof(mixed);      // mixed precision: the position is posq + posqCorrection, summed in double
    const VhdNow w = vhd_now(a);
    if (!w.taken) return;
    double* const x = a.ring + (size_t) vhd_now_set(a, w.j) * 3 * (size_t) a.stride;
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

template <bool EXCLUDE, bool PLAIN>
__global__ void __launch_bounds__(RDF_TILE) vv_kernel_vhd_pairs(const VhdArgs a) {
    if ((int) blockIdx.x >= a.num_items) return;
    const VhdNow w = vhd_now(a);
    int row = 0, set = 0;
    if (!w.taken || !vhd_slot(a, w, (int) blockIdx.y, &row, &set)) return;
    extern __shared__ double vv_dyn_lds[];
    double* const tx = vv_dyn_lds;
    double* const ty = tx + RDF_TILE;
    double* const tz = ty + RDF_TILE;
    int* const tm = (int*) (tz + RDF_TILE);
    unsigned int* const hist = (unsigned int*) (tm + RDF_TILE);
    const int tid = threadIdx.x, nb = a.nbins;
    if (!PLAIN)
        for (int q = tid; q < a.copies * nb; q += RDF_TILE) hist[q] = 0;      // (the first tile's barrier below orders it in front of every add)
    const RdfItem it = a.items[blockIdx.x];
    const size_t planes = 3 * (size_t) a.stride;
    const double* const ox = a.ring + (size_t) set * planes;                  // the i-sites: the origin
    const double* const oy = ox + a.stride;
    const double* const oz = oy + a.stride;
    const double* const sx = a.ring + (size_t) vhd_now_set(a, w.j) * planes;   // the j-sites: now
    const double* const sy = sx + a.stride;
    const double* const sz = sy + a.stride;
    const bool live = tid < it.ni;
    double xi = 0, yi = 0, zi = 0;
    int mi = -1;
    if (live) {
        xi = ox[it.i0 + tid]; yi = oy[it.i0 + tid]; zi = oz[it.i0 + tid];
        if (EXCLUDE) mi = a.mol[it.i0 + tid];
    }
    unsigned int* const h = hist + (a.copies > 1 ? (tid >> 6) * nb : 0);
    long long* const out = a.words + VHD_HEAD + a.head_words + ((size_t) it.cls * (size_t) (a.num_lags + 1) + (size_t) row) * (size_t) nb;
    const double Lx = a.L[0], Ly = a.L[1], Lz = a.L[2], ix = a.inv_L[0], iy = a.inv_L[1], iz = a.inv_L[2];
    const double dr = a.dr, cut2 = a.cut2;
    const float inv_dr = a.inv_dr;
    auto edge = [dr](int k) { const double t = (double) k * dr; return t * t; };
    long long invalid = 0;
    // one pair that passed the range compare: the masks, NaN, then the bin -- the guess from a float square root, one step either way
    // without a branch, and the edges asked again: should they ever disagree, the loops walk (as the RDF pair kernel)
    auto count = [&](double r2, int j, int jself, int cnt) {
        if (j == jself || j >= cnt || (EXCLUDE && mi == tm[j])) return;
        if (r2 != r2) { invalid++; return; }
        int b = min((int) (__builtin_amdgcn_sqrtf((float) r2) * inv_dr), nb - 1);
        b -= (b > 0 && r2 < edge(b)) ? 1 : 0;
        b += (b < nb - 1 && r2 >= edge(b + 1)) ? 1 : 0;
        if (!(edge(b) <= r2 && r2 < edge(b + 1))) {
            while (b > 0 && r2 < edge(b)) b--;
            while (b < nb - 1 && r2 >= edge(b + 1)) b++;
        }
        if (PLAIN) __hip_atomic_fetch_add(out + b, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else __hip_atomic_fetch_add(h + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto dist2 = [&](int j) {
        double dx = tx[j] - xi, dy = ty[j] - yi, dz = tz[j] - zi;
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
        const int jself = it.same ? it.i0 + tid - jbase : -1;      // a class of one group with itself: the site's own earlier self is G_s, not G_d
        for (int j = 0; j < cnt; j += 4) {
            const double r0 = dist2(j), r1 = dist2(j + 1), r2 = dist2(j + 2), r3 = dist2(j + 3);
            if (!(r0 >= cut2)) count(r0, j, jself, cnt);
            if (!(r1 >= cut2)) count(r1, j + 1, jself, cnt);
            if (!(r2 >= cut2)) count(r2, j + 2, jself, cnt);
            if (!(r3 >= cut2)) count(r3, j + 3, jself, cnt);
        }
    }
    if (invalid) __hip_atomic_fetch_add(&a.words[VHD_INVALID], invalid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (PLAIN) return;
    __syncthreads();
    for (int q = tid; q < nb; q += RDF_TILE) {
        long long v = 0;
        for (int c = 0; c < a.copies; c++) v += (long long) hist[c * nb + q];
        if (v != 0) __hip_atomic_fetch_add(out + q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

#ifndef VV_DEVICE_NO_PLAIN_KERNELS
__global__ void __launch_bounds__(64) vv_kernel_vhd_advance(const VhdArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long* const w = a.words;
    const long long j = w[VHD_SAMPLES];
    if (!a.live) { w[VHD_FLOOR] = j; w[VHD_DROPPED] = w[VHD_DROPPED] + 1; return; }
    if (j >= a.max_samples) { w[VHD_DROPPED] = w[VHD_DROPPED] + 1; return; }
    const long long floor_j = w[VHD_FLOOR];
    long long* const head = w + VHD_HEAD;
    auto visit = [&](long long row) {
        long long* const at = head + row * VHD_ROW;
        at[VHD_VISITS] = at[VHD_VISITS] + 1;
        double s = __longlong_as_double(at[VHD_INV_VOLUME]);
        s = s + a.inv_volume;
        at[VHD_INV_VOLUME] = __double_as_longlong(s);
    };
    visit(0);
    const int E = a.origin_every;
    for (long long k = j > 0 ? (j - 1) / E : -1; k >= 0 && k * E >= floor_j && j - k * E <= a.num_lags; k--) visit(j - k * E);
    w[VHD_SAMPLES] = j + 1;
}
__global__ void __launch_bounds__(64) vv_kernel_vhd_floor(long long* words) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    words[VHD_FLOOR] = words[VHD_SAMPLES];
}
#endif
