// vv_layout.h -- the role word of a lane and the cluster word of the in-kernel constraints: what the host analysis (vv_host.cpp) writes
// into the slot tables and the kernels (vv_device.inc) read.  No includes: this header is also compiled at run time (vv_rtc.cpp).
#pragma once

namespace vv {

// ---- role word of one lane ("slot"): what this particle needs from the kernels -----------------
enum Role : uint32_t {
    ROLE_NONE = 0,       // no integration work (idle lane, or a massless particle kept only as image parent)
    ROLE_PLAIN = 1,      // massive, neither NH nor Langevin (a massive image particle): kick + drift only
    ROLE_NH_NORMAL = 2,  // NH thermostat, not in a Drude pair      (normalParticlesNH, HOST:529)
    ROLE_NH_DRUDE = 3,   // NH, Drude particle of a pair (pair.x)   (pairParticlesNH,   HOST:523)
    ROLE_NH_PARENT = 4,  // NH, parent atom of a pair (pair.y)
    ROLE_LD_NORMAL = 5,  // Langevin subset                          (normalParticlesLD, HOST:804)
    ROLE_LD_DRUDE = 6,   //                                          (pairParticlesLD,   HOST:791)
    ROLE_LD_PARENT = 7,
};
constexpr uint32_t META_ROLE_MASK = 0xF;
constexpr int META_PARTNER_SHIFT = 4;    // 6 bits: lane of the Drude partner (own lane if none)
constexpr int META_SEGFIRST_SHIFT = 10;  // 6 bits: first lane of this lane's COM segment (molecule)
constexpr int META_SEGLAST_SHIFT = 16;   // 6 bits: last lane of the segment
constexpr uint32_t META_EFIELD = 1u << 22;     // particle is in particlesElectrolyte
constexpr uint32_t META_HAS_IMAGE = 1u << 23;  // particle is the parent of an image particle
constexpr uint32_t META_COM_LEADER = 1u << 24; // lane that adds its molecule's M*V^2 to TG_COM
constexpr uint32_t META_PAIR = 1u << 25;       // member of a DrudeForce pair (hard wall applies)
constexpr uint32_t META_IS_DRUDE = 1u << 26;   // the Drude (pair.x) of that pair
constexpr uint32_t META_MASSIVE = 1u << 27;    // mass != 0 (velm.w != 0)
constexpr uint32_t META_BIGMOL = 1u << 28;     // lane belongs to a molecule too large for one wave: its COM comes from bigacc
// slot_shake word of a lane that belongs to a constraint cluster (0 otherwise); every member carries the whole cluster, so that each
// lane can gather its mates' data itself: bit 0 central (apex) lane, bit 1 peripheral lane, bits 2-3 number of peripherals np,
// bits 4-9 / 10-15 / 16-21 lanes of peripherals 0 / 1 / 2 (unused ones: the central lane), bits 22-27 lane of the central particle,
// bits 28-29 the lane's own index among the peripherals, bit 30 the cluster is a rigid triangle (SETTLE)
constexpr int SHAKE_WORD_CENTRAL_SHIFT = 22;
constexpr int SHAKE_WORD_OWN_SHIFT = 28;
constexpr uint32_t SHAKE_WORD_SETTLE = 1u << 30;
constexpr uint32_t META_SHAKE = 1u << 30;      // member of an in-kernel constraint cluster: the kernels fetch its cluster word, parameters and
                                               // position in the same round of loads as the velocity, not after reading the cluster word
// General constraint clusters (any topology inside one wave): slot_shake then holds the WAVE's constraint list, constraint l in lane l:
// bits 0-5 lane of particle a, 6-11 lane of particle b, 12-15 colour (constraints of one colour share no particle), bit 31 valid;
// slot_shake_param: d^2, 0.5 / (1/m_a + 1/m_b), 1/m_a, 1/m_b
constexpr uint32_t GC_WORD_VALID = 1u << 31;
// Relaxation factor of the general clusters' sweeps (successive over-relaxation of the Gauss-Seidel SHAKE update): every update is taken
// GC_OMEGA times.  Chains and rings converge fastest slightly above 1; clusters that contain TRIANGLES of constraints (HAngles: H-X-H as an
// H-H distance) are stiff and want more.  Full C3 box, steps/s against the factor (tools/probes/gc_omega_scan.py, round 4, every run
// ends with all constraints within tolerance): AllBonds 25.0 / 29.2 / 32.9 / 32.0 / 30.2 k at 1.0 / 1.1 / 1.2 / 1.25 / 1.3;
// HAngles 8.9 / 14.5 / 17.3 / 17.7 / 16.4 / 13.4 k at 1.0 / 1.3 / 1.4 / 1.45 / 1.5 / 1.6.
constexpr double GC_OMEGA_PLAIN = 1.2, GC_OMEGA_TRIANGLES = 1.4;
// virtual-site word of the lane that places a site: lanes of parents 1, 2, 3 in bits 0-5, 6-11, 12-17 | kind (VS_*, = VVHIP_VSITE_*) << 18 | bit 31 valid
constexpr uint32_t VS_WORD_VALID = 1u << 31;
constexpr uint32_t VS_WORD_HOSTED = 1u << 30;      // the lane belongs to one of the site's parents: the site itself has no lane and is stored by index
constexpr int VS_AVERAGE2 = 0, VS_AVERAGE3 = 1, VS_OUT_OF_PLANE = 2, VS_LOCAL_COORDS = 3;
constexpr uint32_t META_BIG_FIRST = 1u << 29;  // leader of the FIRST chunk of such a molecule (adds M*V^2 once, clears bigacc)

inline uint32_t meta_role(uint32_t m) { return m & META_ROLE_MASK; }

// ---- cos(x) for the cos-acceleration stages (K/cosineAccelerate.cu:8, 26, 70, 82: `cos(2*3.1415926*z*invBoxZ)`, double in every mode)
// The library cosine of the device (ocml) spends ~150 instructions per lane on an argument reduction that copes with |x| up to 1e308;
// the argument here is 2 pi z / Lz, a few turns at most.  One Cody-Waite step with the tail kept (k pi/2 subtracted as a double-double:
// product and rounding error of k * PIO2_1 by fma, the second part of pi/2 by another), then the two fdlibm kernels (k_sin.c / k_cos.c
// polynomials, the tail passed as their `y`) and a select on k mod 4: ~45 instructions.  Only +, *, fma and rint, all correctly
// rounded on gfx950 and on the host alike, so the host check (tests/cpp/cos_check.cpp: 2^22 arguments as the kernels form them, 2^22
// spread over |x| <= 1024 with half of them pushed next to multiples of pi/2, against quad precision) holds for the device bit for bit:
// worst error 0.79 ulp.  `ok` = false where the short reduction is not enough -- |x| > 1024, or the argument within 2^-36 of a multiple
// of pi/2, where the third part of pi/2 starts to matter -- the caller then takes the library cosine (wave-uniform branch, practically
// never taken: probability ~1e-11 per lane for positions that are not adversarial).
#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define VV_HOST_DEVICE __host__ __device__
#else
#define VV_HOST_DEVICE
#endif
VV_HOST_DEVICE inline double cos_short_range(double x, bool& ok) {
    const double INV_PIO2 = 6.36619772367581382433e-01;
    const double PIO2_1 = 1.57079632679489655800e+00;    // the double next to pi/2
    const double PIO2_1T = 6.12323399573676603587e-17;   // pi/2 - PIO2_1, rounded
    const double k = __builtin_rint(x * INV_PIO2);
    const double p = k * PIO2_1, pe = __builtin_fma(k, PIO2_1, -p);      // p + pe = k * PIO2_1 exactly
    const double r0 = x - p;                                              // exact (x / p in [1/2, 2], or p = 0)
    const double t = __builtin_fma(-k, PIO2_1T, -pe);
    const double rh = r0 + t;
    const double bb = rh - r0;
    const double rl = (r0 - (rh - bb)) + (t - bb);                        // rh + rl = r0 + t (two-sum)
    ok = __builtin_fabs(x) <= 1024.0 && __builtin_fabs(rh) >= 0x1p-36;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = rh * rh, w = z * z;
    const double rs = __builtin_fma(z, __builtin_fma(z, S4, S3), S2) + z * w * __builtin_fma(z, S6, S5);
    const double v = z * rh;
    const double sn = rh - ((z * (0.5 * rl - v * rs) - rl) - v * S1);
    const double rc = z * __builtin_fma(z, __builtin_fma(z, C3, C2), C1) + (w * w) * __builtin_fma(z, __builtin_fma(z, C6, C5), C4);
    const double hz = 0.5 * z;
    const double ww = 1.0 - hz;
    const double cs = ww + (((1.0 - ww) - hz) + (z * rc - rh * rl));
    const int n = (int) k & 3;                                            // cos(r + n pi/2): cos, -sin, -cos, sin
    const double res = (n & 1) ? sn : cs;
    return (n == 1 || n == 2) ? -res : res;
}

// ---- (cos, sin) of a phase given in 2^-32 turns, for the density modes (include/vvhip.h: vvhip_modes_* states it; vv_dev_modes.inc)
// The phase is an integer, so the multiple of a turn has dropped out exactly before this function sees it and there is no floating-point
// argument reduction at all: the quadrant is the top two bits of phi + 1/8 turn, the rest is an exact signed offset r from the quadrant's
// centre, |r| <= 2^29, and x = r * C (C the double next to pi 2^-31) has |x| <= pi/4 with ONE rounding.  Then the six-term fdlibm
// polynomials (k_sin.c / k_cos.c: the coefficients of cos_short_range above) by Horner from the highest coefficient, every * and + rounded
// on its own -- NO fma, unlike cos_short_range: NumPy states this function bit for bit (tests/modes_reference.py), and the host build is
// held to that by a digest (tests/cpp/phasor_check.cpp).  Worst absolute error against long double over 2^22 random phases and every
// quadrant and octant edge +- 1: below 2^-51 (tests/test_modes.py).
VV_HOST_DEVICE inline void phasor_turns(unsigned int phi, double& c, double& s) {
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double TURN = 0x1.921fb54442d18p-30;                            // the double next to pi 2^-31 (1.4629180792671596e-09)
    const unsigned int t = phi + 0x20000000u;                             // (mod 2^32)
    const unsigned int q = t >> 30;
    const int r = (int) (t & 0x3FFFFFFFu) - 0x20000000;
    const double x = (double) r * TURN;
    const double z = x * x;
    const double ps = S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6))));
    const double pc = C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6))));
    const double sn = x + (x * z) * ps;
    const double cs = (1.0 - 0.5 * z) + (z * z) * pc;
    c = (q & 1) ? sn : cs;                                                // (cs, sn), (-sn, cs), (-cs, -sn), (sn, -cs)
    s = (q & 1) ? cs : sn;
    if (q == 1 || q == 2) c = -c;
    if (q >= 2) s = -s;
}

// ---- y ~ n2^(-1/2) for the orientation autocorrelation's unit vectors (include/vvhip.h: vvhip_acf_* states it; vv_dev_acf.inc)
// One sequence of correctly rounded +, -, * and exact scalings by powers of two: no sqrt, no rsqrt, no division, no fma, so the device,
// the host and NumPy (tests/acf_reference.py) give the same bits; the host build is held to that by a digest
// (tests/cpp/acf_unit_check.cpp).  n2 is normal and positive (the caller has refused what lies outside [2^-40, 2^40)).  With e the
// exponent of n2 made even (e = exponent - (exponent & 1)), m = n2 2^-e lies in [1, 4) and is formed by rewriting the exponent field;
// the seed is the chord of m^(-1/2) over [1, 2) or over [2, 4) (at most 4.6 % high), four Newton steps y = y (1.5 - (0.5 m) (y y))
// square that error down to the rounding of the last step, and the result is y 2^(-e/2), exact.  With u = d y, | |u|^2 - 1 | stays
// below 7.1e-16 < 2^-50 over 2e5 random vectors of 2^-19 .. 2^19 nm; the recorder's condition is 2^-49 (tests/test_acf.py).
VV_HOST_DEVICE inline double acf_inverse_norm(double n2) {
    const unsigned long long bits = __builtin_bit_cast(unsigned long long, n2);
    const long long e = (long long) ((bits >> 52) & 0x7FFull) - 1023;
    const long long odd = e & 1;
    const double m = __builtin_bit_cast(double, (bits & 0x000FFFFFFFFFFFFFull) | ((unsigned long long) (1023 + odd) << 52));
    const long long h = (e - odd) / 2;                                     // (e - odd is even: exact for either sign)
    double y = m < 2.0 ? 1.2929 - 0.2929 * m : 0.9142 - 0.10355 * m;
    const double hm = 0.5 * m;
    y = y * (1.5 - hm * (y * y));
    y = y * (1.5 - hm * (y * y));
    y = y * (1.5 - hm * (y * y));
    y = y * (1.5 - hm * (y * y));
    return y * __builtin_bit_cast(double, (unsigned long long) (1023 - h) << 52);
}

// ---- contact matrices (include/vvhip.h: vvhip_contacts_* states the sites, the classes, the contact and the table; vv_dev_contacts.inc)
// One matrix holds every class's bits, word-major: class c starts at class_offset[c] and its word (jw, i) -- the columns 64 jw .. 64 jw + 63
// of row i -- is at class_offset[c] + jw * rows_padded[c] + i.  rows_padded = N_a rounded up to 64 (the mask kernel stores 64 rows at a time;
// the rows and columns past the last site are 0 bits), so a class's words are a multiple of 64 and every class starts on 16 bytes.
// The recorder's words: [head_words] counts, table[C][num_lags][4], ord[R] (rounded up to an even count), then the ring of origins
// [R][sample_words] and, with the continuous correlation, the ring of the surviving contacts, the same size.  The sample's own matrix and
// the gather's planes are scratch.  Integers only: the host (vv_observe.cpp) and tests/cpp/contacts_layout_check.cpp share it.
constexpr int CONTACTS_MAX_CLASSES = 8, CONTACTS_MAX_GROUPS = 16;
constexpr int CONTACTS_CORR_PAIRS = 1024;      // pairs of words per work item of the correlate kernel (256 threads, four 128-bit loads each)
struct ContactsLayout {
    long long rows_padded[CONTACTS_MAX_CLASSES], col_words[CONTACTS_MAX_CLASSES];
    long long class_words[CONTACTS_MAX_CLASSES], class_offset[CONTACTS_MAX_CLASSES];
    long long sample_words;         // words of one matrix
    int num_origins, ord_words;     // R = ceil(num_lags / origin_every); R rounded up to 2
    long long table_words;          // num_classes * num_lags * 4
    long long ring_words;           // R * sample_words, times 2 with the continuous correlation
    long long words_bytes;          // counts, table, ord and rings: what a recovery snapshot copies
    long long scratch_bytes;        // the sample's matrix and the gather's three planes (the sites rounded up to 16)
    long long total_bytes;
};
inline ContactsLayout contacts_layout(int num_classes, const int* rows, const int* cols, int num_lags, int origin_every, bool continuous,
                                      long long sites, int head_words) {
    ContactsLayout L{};
    for (int c = 0; c < num_classes; c++) {
        L.rows_padded[c] = ((long long) rows[c] + 63) / 64 * 64;
        L.col_words[c] = ((long long) cols[c] + 63) / 64;
        L.class_words[c] = L.rows_padded[c] * L.col_words[c];
        L.class_offset[c] = L.sample_words;
        L.sample_words += L.class_words[c];
    }
    L.num_origins = (num_lags + origin_every - 1) / origin_every;
    L.ord_words = (L.num_origins + 1) / 2 * 2;
    L.table_words = (long long) num_classes * num_lags * 4;
    L.ring_words = (long long) L.num_origins * L.sample_words * (continuous ? 2 : 1);
    L.words_bytes = ((long long) head_words + L.table_words + L.ord_words + L.ring_words) * 8;
    L.scratch_bytes = L.sample_words * 8 + 3 * ((sites + 15) / 16 * 16) * 8;
    L.total_bytes = L.words_bytes + L.scratch_bytes;
    return L;
}
// A block's work in the mask kernel: the rows i0 .. i1 - 1 of class cls (multiples of 64, i1 - i0 <= rows per tile, i1 <= rows_padded)
// against the column words jw0 .. jw1 - 1
struct ContactsMaskItem { int cls, i0, i1, jw0, jw1, pad_[3]; };
// ... and in the correlate kernel: the pairs of words p0 .. p0 + np - 1 of a matrix (word 2 p), all of class cls; first != 0: the class's
// designated block, which counts the visit.  A class without words still has that one item, with np = 0
struct ContactsCorrItem { int cls, first; long long p0; int np, pad_; };
// The two work lists; out = null: only the count.  rows_per_tile is a multiple of 64, words_per_item >= 1
inline long long contacts_mask_items(const ContactsLayout& L, int num_classes, int rows_per_tile, int words_per_item, ContactsMaskItem* out) {
    long long n = 0;
    for (int c = 0; c < num_classes; c++)
        for (long long i0 = 0; i0 < L.rows_padded[c]; i0 += rows_per_tile)
            for (long long jw0 = 0; jw0 < L.col_words[c]; jw0 += words_per_item, n++) {
                if (!out) continue;
                const long long i1 = i0 + rows_per_tile < L.rows_padded[c] ? i0 + rows_per_tile : L.rows_padded[c];
                const long long jw1 = jw0 + words_per_item < L.col_words[c] ? jw0 + words_per_item : L.col_words[c];
                out[n] = {c, (int) i0, (int) i1, (int) jw0, (int) jw1, {0, 0, 0}};
            }
    return n;
}
inline long long contacts_corr_items(const ContactsLayout& L, int num_classes, ContactsCorrItem* out) {
    long long n = 0;
    for (int c = 0; c < num_classes; c++) {
        const long long pairs = L.class_words[c] / 2;
        long long p = 0;
        do {
            const long long np = pairs - p < CONTACTS_CORR_PAIRS ? pairs - p : CONTACTS_CORR_PAIRS;
            if (out) out[n] = {c, p == 0 ? 1 : 0, L.class_offset[c] / 2 + p, (int) np, 0};
            n++; p += np;
        } while (p < pairs);
    }
    return n;
}

}  // namespace vv
