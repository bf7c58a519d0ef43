"""The trigger's host twin (gsdr_trigger_* in trigger_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: a
stand-alone program with its own main, built from the host sources alone with plain g++ (no HIP header, no device part:
only GSDR_TRIGGER_HOST objects exist in such a build).  Every buffer is a heap block of exactly the documented extent,
so one sample read or written past an end is a report.  Nothing is loaded into Python, nothing is preloaded; in the
style of tests/test_sc16_tx_sanitizers.py."""
from _sanitized import build_and_run

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "gsdr.h"

// the planted case of tests/_trigger.py: 5 channels, pre 2, post 4, holdoff 3, 64 rows, channel 4 switched off
static const int N_CH = 5, PRE = 2, POST = 4, HOLDOFF = 3, ROWS = 64, S = PRE + POST;
static const int PULSES[10][3] = {{1, 0, 2}, {9, 2, 2}, {11, 1, 2}, {15, 3, 3}, {31, 0, 2}, {32, 1, 2}, {40, 4, 5},
                                  {47, 3, -2}, {47, 1, -2}, {63, 2, 2}};

static std::vector<gsdr_c64> stream() {
    std::vector<gsdr_c64> x((size_t)ROWS * N_CH);
    unsigned s = 12345u;
    for (auto &v : x) {                                   // background within +-0.3
        s = s * 1664525u + 1013904223u;
        v.x = ((float)(s >> 8) / 16777216.0f - 0.5f) * 0.6f;
        s = s * 1664525u + 1013904223u;
        v.y = ((float)(s >> 8) / 16777216.0f - 0.5f) * 0.6f;
    }
    for (auto &p : PULSES) x[(size_t)p[0] * N_CH + p[1]].x += (float)p[2];
    x[(size_t)8 * N_CH + 0].y = std::numeric_limits<float>::quiet_NaN();      // inside the snippet of row 9
    x[(size_t)14 * N_CH + 4].x = std::numeric_limits<float>::infinity();      // switched-off channel
    x[(size_t)46 * N_CH + 2].x = -0.0f;
    return x;
}

// feeds the stream cut as `cut` (0-terminated by -1), every buffer a heap block of its exact extent; returns the number of
// mismatches against the rows / dropped counts in want_rows (-1 terminated) / want_dropped
static int run(const std::vector<gsdr_c64> &x, const int *cut, int max_events, const long long *want_rows, int want_dropped) {
    std::vector<gsdr_trigger_level> lv((size_t)N_CH);
    for (int c = 0; c < N_CH; ++c) lv[(size_t)c] = gsdr_trigger_level{0.f, 0.f, 1.f, 0.f, -1.f, 1.f};
    lv[4].lo = -std::numeric_limits<float>::infinity();
    lv[4].hi = std::numeric_limits<float>::infinity();
    int max_rows = 1;
    for (const int *c = cut; *c >= 0; ++c) max_rows = *c > max_rows ? *c : max_rows;
    gsdr_trigger_level *lvh = (gsdr_trigger_level *)std::malloc(sizeof(gsdr_trigger_level) * N_CH);
    std::memcpy(lvh, lv.data(), sizeof(gsdr_trigger_level) * N_CH);
    gsdr_trigger *t = gsdr_trigger_create(N_CH, max_rows, PRE, POST, HOLDOFF, max_events, lvh, GSDR_TRIGGER_HOST);
    std::free(lvh);                                       // the levels are copied by create
    if (!t) return 100;
    int bad = 0, at = 0, seen = 0, dropped_all = 0;
    for (const int *c = cut; *c >= 0; ++c) {
        const int n = *c;
        gsdr_c64 *rows = n ? (gsdr_c64 *)std::malloc(sizeof(gsdr_c64) * (size_t)n * N_CH) : nullptr;
        if (n) std::memcpy(rows, x.data() + (size_t)at * N_CH, sizeof(gsdr_c64) * (size_t)n * N_CH);
        gsdr_trigger_event *ev = (gsdr_trigger_event *)std::malloc(sizeof(gsdr_trigger_event) * (size_t)max_events);
        gsdr_c64 *sn = (gsdr_c64 *)std::malloc(sizeof(gsdr_c64) * (size_t)max_events * S * N_CH);
        int dropped = -1;
        // n_rows == 0: nothing is touched, not even the pointers
        const int ne = n ? gsdr_trigger_feed_host(t, rows, n, ev, sn, &dropped) : gsdr_trigger_feed_host(t, nullptr, 0, nullptr, nullptr, &dropped);
        if (ne < 0 || ne > max_events || dropped < 0) ++bad;
        for (int e = 0; e < ne; ++e, ++seen) {
            if (want_rows[seen] < 0 || ev[e].row != want_rows[seen]) { ++bad; break; }
            if (std::memcmp(sn + (size_t)e * S * N_CH, x.data() + (size_t)(ev[e].row - PRE) * N_CH, sizeof(gsdr_c64) * S * N_CH)) ++bad;
        }
        dropped_all += dropped;
        at += n;
        std::free(rows);
        std::free(ev);
        std::free(sn);
    }
    if (want_rows[seen] >= 0 || dropped_all != want_dropped || gsdr_trigger_rows(t) != at) ++bad;
    if (gsdr_trigger_reset(t) != 0 || gsdr_trigger_rows(t) != 0) ++bad;
    gsdr_trigger_close(t);
    return bad;
}

int main() {
    const std::vector<gsdr_c64> x = stream();
    const long long all[] = {9, 15, 31, 47, -1}, two[] = {9, 15, -1};
    const int whole[] = {64, -1}, halves[] = {32, 32, -1}, sevens[] = {7, 7, 7, 7, 7, 7, 7, 7, 7, 1, -1}, gaps[] = {3, 0, 29, 0, 32, -1};
    int bad = 0;
    bad += run(x, whole, 8, all, 0);
    bad += run(x, halves, 8, all, 0);
    bad += run(x, sevens, 8, all, 0);
    bad += run(x, gaps, 8, all, 0);
    bad += run(x, whole, 2, two, 2);                      // the capacity rule: two written, two counted
    // a refusal leaves a NULL and no allocation behind
    if (gsdr_trigger_create(N_CH, 64, PRE, 0, HOLDOFF, 8, nullptr, GSDR_TRIGGER_HOST)) ++bad;
    gsdr_trigger_close(nullptr);
    std::printf("runs 5 bad %d\n", bad);
    return bad ? 1 : 0;
}
'''


def test_trigger_host_under_asan_and_ubsan(tmp_path):
    run = build_and_run(DRIVER, tmp_path)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.strip() == "runs 5 bad 0", run.stdout
