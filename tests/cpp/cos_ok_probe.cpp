// Host build of vv::cos_short_range (csrc/vv_layout.h) as a probe for tests/param_range_cases.py: the predicate `ok` is +, *, fma and rint
// only, so what it says here is what it says on gfx950.  Arguments are formed as cos_kz forms them: 2 * 3.1415926 * z * invBoxZ in double.
//   cos_ok_probe ok <invBoxZ> < z values, one per line  -> "1" / "0" per line
//   cos_ok_probe node <Lz>  -> a double z just above Lz / 4 whose argument (invBoxZ = 1 / Lz) has |x| <= 1024 and ok == false: next to pi / 2
// Build: g++ -O2 -ffp-contract=off -mfma, as cos_check.cpp.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "vv_layout.h"

static double arg_of(double z, double inv) { return 2 * 3.1415926 * z * inv; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    bool ok;
    if (!std::strcmp(argv[1], "ok")) {
        const double inv = std::strtod(argv[2], nullptr);
        char line[128];
        while (std::fgets(line, sizeof line, stdin)) {
            vv::cos_short_range(arg_of(std::strtod(line, nullptr), inv), ok);
            std::printf("%d\n", (int) ok);
        }
        return 0;
    }
    const double lz = std::strtod(argv[2], nullptr), inv = 1.0 / lz;
    double z = lz / 4;                                  // x = 3.1415926 / 2: 2.7e-8 below pi / 2
    // cos(x) ~ pi / 2 - x there: jump by most of the remaining distance while it is large, then step double by double
    for (double c; (c = vv::cos_short_range(arg_of(z, inv), ok)) > 0x1p-40 && ok;) z += 0.5 * c / (2 * 3.1415926 * inv);
    for (long i = 0; ok && i < (1L << 24); i++) {
        z = std::nextafter(z, lz);
        vv::cos_short_range(arg_of(z, inv), ok);
    }
    if (ok || std::fabs(arg_of(z, inv)) > 1024.0) return 1;
    std::printf("%a\n", z);
    return 0;
}
