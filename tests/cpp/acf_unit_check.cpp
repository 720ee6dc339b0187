// Host check of vv::acf_inverse_norm (csrc/vv_layout.h): the function is correctly rounded +, - and * and exact scalings only, so what it
// returns here is what it returns on gfx950 and what tests/acf_reference.py forms in NumPy, bit for bit.  Prints an order-independent
// digest of the unit vectors' bits over a fixed vector list -- the sum mod 2^64 of mix(index, u_x bits, u_y bits, u_z bits) -- which
// tests/test_acf.py recomputes in NumPy.
// The list: vector i (0 <= i < 2^18) has the components ((mix(4 i + a) >> 11) - 2^52) 2^-52 for a = 0, 1, 2 (53 random bits in [-1, 1),
// exact), all three scaled by 2^(mix(4 i + 3) mod 39 - 19); mix is splitmix64's finaliser of (k + 1) 0x9E3779B97F4A7C15.  The unit vector
// is d * y with n2 = (dx dx + dy dy) + dz dz as the recorder forms it; a vector whose n2 is outside [2^-40, 2^40) is skipped.
// Build: g++ -O2 -ffp-contract=off -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "vv_layout.h"

static uint64_t mix(uint64_t k) {
    uint64_t z = (k + 1) * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t bits(double x) { uint64_t u; std::memcpy(&u, &x, 8); return u; }

int main() {
    uint64_t digest = 0;
    long n = 0;
    for (uint64_t i = 0; i < (1ull << 18); i++) {
        double d[3];
        double scale = 1.0;
        const int s = (int) (mix(4 * i + 3) % 39) - 19;
        for (int k = 0; k < (s < 0 ? -s : s); k++) scale = s < 0 ? scale * 0.5 : scale * 2.0;
        for (int a = 0; a < 3; a++) d[a] = (double) ((int64_t) (mix(4 * i + a) >> 11) - ((int64_t) 1 << 52)) * 0x1p-52 * scale;
        const double n2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        if (!(n2 >= 0x1p-40 && n2 < 0x1p40)) continue;
        const double y = vv::acf_inverse_norm(n2);
        digest += (i + 1) * 0x9E3779B97F4A7C15ull + bits(d[0] * y) * 0xC2B2AE3D27D4EB4Full + bits(d[1] * y) * 0x165667B19E3779F9ull +
                  bits(d[2] * y) * 0x27D4EB2F165667C5ull;
        n++;
    }
    std::printf("%ld %016llx\n", n, (unsigned long long) digest);
    return 0;
}
