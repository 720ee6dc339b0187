// vv_schedule.hpp -- when a rider of the step (vv_plan.hpp: Rider) is due, stated once: every interval-th step, or GroReporter(logarithm=True)'s
// steps (include/vvhip.h: vvhip_frames_schedule).  Integers only and no HIP: tests/cpp/schedule_check.cpp builds it alone.
#pragma once
#include <vector>

enum { SCHEDULE_LINEAR = 0, SCHEDULE_LOG10 = 1 };      // (= VVHIP_FRAMES_LINEAR / VVHIP_FRAMES_LOG10: vv_plan.hpp asserts it)
struct Schedule { int interval = 0; int kind = SCHEDULE_LINEAR; };

// The first due step after step c >= 0.  LOG10 is GroReporter's recurrence -- base = interval while c < interval, else the largest power of
// ten <= c -- which names the same steps wherever it starts.
inline long long next_due(const Schedule& s, long long c) {
    long long base = s.interval;
    if (s.kind == SCHEDULE_LOG10 && c >= s.interval)
        for (base = 1; base <= c / 10; base *= 10) {}
    return c + base - c % base;
}
// Is step t >= 0 due?  (Step 0 is a multiple of every interval, and no step of the logarithmic pattern.)
inline bool due(const Schedule& s, long long t) { return t == 0 ? s.kind == SCHEDULE_LINEAR : next_due(s, t - 1) == t; }
// The due steps t in [lo, hi] (lo >= 0), as t - origin
inline std::vector<int> due_in(const Schedule& s, long long lo, long long hi, long long origin) {
    std::vector<int> r;
    for (long long t = due(s, lo) ? lo : next_due(s, lo); t <= hi; t = next_due(s, t)) r.push_back((int) (t - origin));
    return r;
}
