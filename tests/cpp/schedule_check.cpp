// schedule_check.cpp -- csrc/vv_schedule.hpp alone (tests/test_schedule.py builds this with the host sanitizers and runs it as a process).
//   schedule_check                          due_in against a plain walk of due() over every step of the window, for both kinds and both
//                                           positions of a rider; next_due strictly increasing and naming the same steps wherever it starts
//   schedule_check interval kind after n    the first n due steps after `after`, found by asking due() for every step, one per line
#include "../../openmm-velocityverlet_amd/csrc/vv_schedule.hpp"

#include <cstdio>
#include <cstdlib>

static long long cases = 0;

static int fail(const char* what, const Schedule& s, long long c0, long long n) {
    std::printf("FAILED %s: interval %d kind %d c0 %lld window %lld\n", what, s.interval, s.kind, c0, n);
    return 1;
}
// the window of `steps` steps after counter c0: a rider behind the step looks at c0 + 1 .. c0 + steps, one in front at c0 .. c0 + steps - 1
static int check_windows(const Schedule& s, long long c0) {
    for (int steps : {1, 2, 7, 20, 64})
        for (int front = 0; front < 2; front++) {
            const long long lo = front ? c0 : c0 + 1, hi = lo + steps - 1;
            std::vector<int> want;
            for (long long t = lo; t <= hi; t++)
                if (due(s, t)) want.push_back((int) (t - c0));
            if (due_in(s, lo, hi, c0) != want) return fail(front ? "window in front" : "window behind", s, c0, steps);
            cases++;
        }
    return 0;
}
// from `a`, next_due climbs strictly and visits exactly the steps of (a, a + span] that the walk from 0 (`from0`, a bitmap) visits
static int check_walk(const Schedule& s, const std::vector<char>& from0, long long a) {
    const long long last = (long long) from0.size() - 1;
    std::vector<char> seen(from0.size(), 0);
    for (long long c = a, t; c <= last; c = t) {
        t = next_due(s, c);
        if (t <= c) return fail("next_due does not increase", s, c, t);
        if (t <= last) seen[(size_t) t] = 1;
    }
    for (long long t = a + 1; t <= last; t++)
        if (seen[(size_t) t] != from0[(size_t) t]) return fail("walk depends on its start", s, a, t);
    cases++;
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5) {
        const Schedule s{std::atoi(argv[1]), std::atoi(argv[2])};
        long long t = std::atoll(argv[3]);
        for (int n = std::atoi(argv[4]); n > 0; n--) {
            do t++; while (!due(s, t));
            std::printf("%lld\n", t);
        }
        return 0;
    }
    std::vector<long long> starts;
    for (long long c = 0; c < 400; c++) starts.push_back(c);
    for (long long c : {999ll, 1000ll, 9999ll, 1000000ll - 3, 1000000000000ll - 5}) starts.push_back(c);
    for (int kind : {SCHEDULE_LINEAR, SCHEDULE_LOG10})
        for (int interval : {1, 2, 3, 7, 10, 30, 64, 150}) {
            const Schedule s{interval, kind};
            for (long long c0 : starts)
                if (check_windows(s, c0)) return 1;
            if (kind == SCHEDULE_LOG10)
                for (long long pw = 1; pw <= 1000000000000000ll; pw *= 10)
                    for (long long c0 = pw > 3 ? pw - 3 : 0; c0 <= pw + 3; c0++)
                        if (check_windows(s, c0)) return 1;
            std::vector<char> from0(2501, 0);
            for (long long t = next_due(s, 0); t < (long long) from0.size(); t = next_due(s, t)) from0[(size_t) t] = 1;
            for (long long a = 0; a < (long long) from0.size(); a++)
                if (check_walk(s, from0, a)) return 1;
        }
    std::printf("SCHEDULE OK cases=%lld\n", cases);
    return 0;
}
