// vv_dev_contacts.inc -- part of vv_device.inc: contact lifetime correlations (vvhip_contacts_*; include/vvhip.h states the sites, the classes,
// the contact, the slots and the table; vv_layout.h: ContactsLayout states where every word lies).  Stand-alone kernels that read posq and
// posqCorrection and write the recorder's own words and scratch, and nothing else: no velocity, no force, no accumulator, no thermostat
// copy, no rendezvous or status word.  Everything the table holds is an integer: the same bits for any work list, tile shape or order.
//   gather:     the RDF's: one thread per site, striding over a capped grid: X_s in float64 into the planar scratch double[3][stride],
//               ordered by group.
//   mask:       one block of 256 threads per work item (ContactsMaskItem: class, a tile of rows, a run of column words).  The tile's rows
//               are staged in LDS as planar doubles (and their molecules); a wave takes the run's column words one at a time, a lane keeps
//               its column site in registers, and every lane reads the same row: a broadcast, free of bank conflicts.  Per pair and axis
//               d = X_i - X_j, n = rint(d inv_L), d = d - L n, then r2 = (dx dx + dy dy) + dz dz and the strict compare r2 < cut2: the wave's
//               compare mask IS the 64-bit word of row i (__ballot: no shuffle), and lane (i mod 64) keeps it.  After 64 rows every lane
//               stores one word: word-major, so the stores are contiguous.  Rows and columns past the last site, the diagonal of a class of
//               one group with itself and, with the exclusion on, pairs of one molecule give 0 bits; what is left and has a NaN r2 is
//               counted, with one agent-scope add per block at the most.  Where the sample is an origin (j mod E = 0) the same lanes store
//               the word into the slot's origin and surviving-contact copies too.
//   correlate:  one block of 256 threads per (slot, ContactsCorrItem: a run of pairs of words of one class), a thread per pair and trip:
//               128-bit loads of origin, surviving contacts and the sample's matrix, popcounts, the surviving contacts stored back only where
//               they change.  With skip_zero a zero origin pair costs no further load (cont is a subset of origin).  The three sums go
//               through the wave (wave_reduce4_rows), the block's waves through LDS, and to the table with one agent-scope add per
//               non-zero word; the class's designated block counts the visit.  A slot's lag l = j - ord[s]; the slot this sample itself
//               fills has l = 0 (its ord word is written behind this kernel, by the advance).
//   advance:    one wave behind them: writes ord[s] where the sample is an origin, counts the sample or the drop; no memset, no host work.
// The tails need no special case: a class without rows or columns has no mask item and one correlate item without pairs.
#ifndef VV_DEVICE_NO_PLAIN_KERNELS

__device__ __forceinline__ long long contacts_ordinal(const ContactsArgs& a) {
    return (long long) __hip_atomic_load((const unsigned long long*) &a.words[CONTACTS_SAMPLES], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool contacts_taken(const ContactsArgs& a, long long j) { return a.live && j < a.max_samples; }

template <class real, class mixed>
__global__ void __launch_bounds__(256) vv_kernel_contacts_gather(const ContactsArgs a) {
    using real4 = typename Vec<real>::v4;
    constexpr bool CORR = sizeof(real) != sizeof(mixed);      // mixed precision: the position is posq + posqCorrection, summed in double
    if (!contacts_taken(a, contacts_ordinal(a))) return;
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
__global__ void __launch_bounds__(256) vv_kernel_contacts_mask(const ContactsArgs a) {
    const long long j = contacts_ordinal(a);
    if ((int) blockIdx.x >= a.num_mask_items || !contacts_taken(a, j)) return;
    extern __shared__ double vv_dyn_lds[];
    const int T = a.rows_per_tile;
    double* const tx = vv_dyn_lds;
    double* const ty = tx + T;
    double* const tz = ty + T;
    int* const tm = (int*) (tz + T);
    long long* const bad = (long long*) (tm + T);                 // the block's NaN pairs (T is a multiple of 64: aligned)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ContactsMaskItem it = a.mask_items[blockIdx.x];
    const int c = it.cls, na = a.rows[c], nb = a.cols[c], fa = a.first_row[c], fb = a.first_col[c];
    const double* const sx = a.scratch;
    const double* const sy = sx + a.stride;
    const double* const sz = sy + a.stride;
    if (tid == 0) *bad = 0;
    // the tile's rows; past the class's last row zeros (their bits are masked by the row's index below)
    for (int r = tid; r < it.i1 - it.i0; r += 256) {
        const int i = it.i0 + r;
        const bool in = i < na;
        tx[r] = in ? sx[fa + i] : 0.0; ty[r] = in ? sy[fa + i] : 0.0; tz[r] = in ? sz[fa + i] : 0.0;
        if (EXCLUDE) tm[r] = in ? a.mol[fa + i] : -2;
    }
    __syncthreads();
    const double Lx = a.L[0], Ly = a.L[1], Lz = a.L[2], ix = a.inv_L[0], iy = a.inv_L[1], iz = a.inv_L[2];
    const double cut2 = a.cut2[c];
    const bool diagonal = fa == fb;                               // a class of one group with itself: no site with itself
    const bool is_origin = j % a.origin_every == 0;
    const long long slot_at = (long long) ((j / a.origin_every) % a.num_origins) * a.sample_words;
    long long invalid = 0;                                        // (wave-uniform)
    for (int jw = it.jw0 + wave; jw < it.jw1; jw += 4) {
        const int col = jw * 64 + lane;
        const bool col_in = col < nb;
        double xj = 0, yj = 0, zj = 0;
        int mj = -1;
        if (col_in) {
            xj = sx[fb + col]; yj = sy[fb + col]; zj = sz[fb + col];
            if (EXCLUDE) mj = a.mol[fb + col];
        }
        for (int r0 = 0; r0 < it.i1 - it.i0; r0 += 64) {
            unsigned long long keep = 0;
            const int rows_in = min(64, na - (it.i0 + r0));       // (<= 0: a chunk of padding rows, all words 0)
            for (int r = 0; r < rows_in; r++) {
                const int i = it.i0 + r0 + r;
                double dx = tx[r0 + r] - xj, dy = ty[r0 + r] - yj, dz = tz[r0 + r] - zj;
                dx = dx - Lx * rint(dx * ix);
                dy = dy - Ly * rint(dy * iy);
                dz = dz - Lz * rint(dz * iz);
                const double r2 = (dx * dx + dy * dy) + dz * dz;
                bool pair = col_in && !(diagonal && i == col);
                if (EXCLUDE) pair = pair && tm[r0 + r] != mj;
                const unsigned long long word = __ballot(pair && r2 < cut2);
                invalid += __popcll(__ballot(pair && r2 != r2));
                if (lane == r) keep = word;
            }
            const long long at = a.class_offset[c] + (long long) jw * a.rows_padded[c] + it.i0 + r0 + lane;
            a.mask[at] = keep;
            if (is_origin) {
                a.origin[slot_at + at] = keep;
                if (a.cont) a.cont[slot_at + at] = keep;
            }
        }
    }
    if (lane == 0 && invalid != 0) __hip_atomic_fetch_add(bad, invalid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (tid == 0 && *bad != 0) __hip_atomic_fetch_add(&a.words[CONTACTS_INVALID], *bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool CONT>
__global__ void __launch_bounds__(256) vv_kernel_contacts_correlate(const ContactsArgs a) {
    const long long j = contacts_ordinal(a);
    if ((int) blockIdx.x >= a.num_corr_items || !contacts_taken(a, j)) return;
    __shared__ long long part[4][3];
    const int s = blockIdx.y;
    // the slot this sample fills holds it already (the mask kernel stored both copies); its ord word follows in the advance
    const bool fills = j % a.origin_every == 0 && s == (int) ((j / a.origin_every) % a.num_origins);
    const long long o = fills ? j : a.ord[s];
    const long long l = j - o;
    if (o < 0 || l >= a.num_lags) return;                         // (block-uniform)
    const ContactsCorrItem it = a.corr_items[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ulonglong2* const org = (const ulonglong2*) (a.origin + (long long) s * a.sample_words);
    ulonglong2* const cnt = CONT ? (ulonglong2*) (a.cont + (long long) s * a.sample_words) : nullptr;
    const ulonglong2* const now = (const ulonglong2*) a.mask;
    long long n1 = 0, n2 = 0, n3 = 0;
    for (int q = tid; q < it.np; q += 256) {
        const long long p = it.p0 + q;
        const ulonglong2 og = org[p];
        if (a.skip_zero && (og.x | og.y) == 0) continue;          // no contact at the origin: none now, none surviving
        const ulonglong2 h = now[p];
        n1 += __popcll(og.x) + __popcll(og.y);
        n2 += __popcll(og.x & h.x) + __popcll(og.y & h.y);
        if (CONT) {
            const ulonglong2 was = cnt[p];
            const ulonglong2 is = {was.x & h.x, was.y & h.y};
            if (is.x != was.x || is.y != was.y) cnt[p] = is;
            n3 += __popcll(is.x) + __popcll(is.y);
        }
    }
    // rows 0, 1, 2 of the wave hold 16 partial sums of n1, n2, n3; four shifts inside the rows leave the totals in lanes 15, 31, 47
    long long t = wave_reduce4_rows<long long>(n1, n2, n3, 0);
    t += dpp_fetch_i64<0x111, 0xF>(t);
    t += dpp_fetch_i64<0x112, 0xF>(t);
    t += dpp_fetch_i64<0x114, 0xF>(t);
    t += dpp_fetch_i64<0x118, 0xF>(t);
    if ((lane & 15) == 15 && lane < 48) part[wave][lane >> 4] = t;
    __syncthreads();
    if (tid < 4) {
        long long* const cell = a.table + ((long long) it.cls * a.num_lags + l) * 4 + tid;
        const long long v = tid == 0 ? (long long) (it.first != 0) : part[0][tid - 1] + part[1][tid - 1] + part[2][tid - 1] + part[3][tid - 1];
        if (v != 0) __hip_atomic_fetch_add(cell, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(64) vv_kernel_contacts_advance(const ContactsArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const long long j = a.words[CONTACTS_SAMPLES];
    if (!contacts_taken(a, j)) { a.words[CONTACTS_DROPPED] = a.words[CONTACTS_DROPPED] + 1; return; }
    if (j % a.origin_every == 0) a.ord[(j / a.origin_every) % a.num_origins] = j;
    a.words[CONTACTS_SAMPLES] = j + 1;
}
#endif
