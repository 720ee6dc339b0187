// Host check of vv::phasor_turns (csrc/vv_layout.h): the function is correctly rounded +, - and * only, so what it returns here is what it
// returns on gfx950 and what tests/modes_reference.py forms in NumPy, bit for bit.  Prints an order-independent digest of the (cos, sin)
// bits over a fixed phase list -- the sum mod 2^64 of mix(phase, cos bits, sin bits) -- which tests/test_modes.py recomputes in NumPy.
// The list: 2^20 phases of a xorshift64 generator, then every multiple of 2^28 (quadrant and octant edges, sixteenths) with -1, 0, +1.
// Build: g++ -O2 -ffp-contract=off.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "vv_layout.h"

static uint64_t state = 88172645463325252ull;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }
static uint64_t bits(double x) { uint64_t u; std::memcpy(&u, &x, 8); return u; }

int main() {
    uint64_t digest = 0;
    long n = 0;
    auto probe = [&](uint32_t phi) {
        double c, s;
        vv::phasor_turns(phi, c, s);
        digest += ((uint64_t) phi + 1) * 0x9E3779B97F4A7C15ull + bits(c) * 0xC2B2AE3D27D4EB4Full + bits(s) * 0x165667B19E3779F9ull;
        n++;
    };
    for (long i = 0; i < (1l << 20); i++) probe((uint32_t) (rnd() >> 32));
    for (uint64_t e = 0; e < 16; e++)
        for (int d = -1; d <= 1; d++) probe((uint32_t) ((e << 28) + (uint64_t) (int64_t) d));
    std::printf("%ld %016llx\n", n, (unsigned long long) digest);
    return 0;
}
