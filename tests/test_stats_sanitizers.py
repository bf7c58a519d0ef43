"""The row statistics' host twin (gsdr_stats_* in stats_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: a
stand-alone program with its own main, built from the host sources alone with plain g++ (no HIP header, no device part:
only GSDR_STATS_HOST objects exist in such a build).  Every buffer -- the axes, the rows of a feed, the summaries, the
counters, the quantiles, the levels, the flags -- is a heap block of exactly the documented extent, so one element read
or written past an end is a report.  Nothing is loaded into Python, nothing is preloaded; built exactly as
tests/test_sweep_sanitizers.py builds its program."""
from _sanitized import build_and_run

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "gsdr.h"

template <class T>
static T *block(size_t count) { return (T *)std::malloc(sizeof(T) * (count ? count : 1)); }

static std::vector<gsdr_c64> stream(long long rows, int n_ch) {
    std::vector<gsdr_c64> x((size_t)rows * n_ch);
    unsigned s = 4711u;
    for (auto &v : x) {
        s = s * 1664525u + 1013904223u;
        v.x = 0.3f + 0.01f * ((float)(s >> 8) / 16777216.0f - 0.5f);
        s = s * 1664525u + 1013904223u;
        v.y = -0.4f + 0.02f * ((float)(s >> 8) / 16777216.0f - 0.5f);
    }
    return x;
}

struct Result {
    std::vector<unsigned char> bytes;        // summaries, counters, quantiles and levels, one after the other
    void add(const void *p, size_t n) { bytes.insert(bytes.end(), (const unsigned char *)p, (const unsigned char *)p + n); }
};

// feeds the stream cut as `cut` (terminated by -1) and reads everything
static int run(const std::vector<gsdr_c64> &x, int n_ch, int max_rows, int n_bins, int lanes, const long long *cut, Result &out) {
    gsdr_trigger_level *axes = block<gsdr_trigger_level>((size_t)n_ch);
    for (int c = 0; c < n_ch; ++c) axes[c] = gsdr_trigger_level{0.1f, -0.2f, 1.0f, c % 2 ? 0.5f : 0.0f, 0.15f - 0.001f * c, 0.25f + 0.001f * c};
    gsdr_stats *s = gsdr_stats_create(n_ch, max_rows, n_bins, lanes, axes, GSDR_STATS_HOST);
    if (!s) return 100;
    int bad = 0;
    if (gsdr_stats_n_bins(s) != n_bins || gsdr_stats_lanes(s) < 1 || (lanes && gsdr_stats_lanes(s) != lanes)) ++bad;
    long long at = 0;
    for (const long long *c = cut; *c >= 0; ++c) {
        const int n = (int)*c;
        gsdr_c64 *rows = n ? block<gsdr_c64>((size_t)n * n_ch) : nullptr;
        if (n) std::memcpy(rows, x.data() + (size_t)at * n_ch, sizeof(gsdr_c64) * (size_t)n * n_ch);
        if (gsdr_stats_feed_host(s, rows, n) != 0) ++bad;              // n == 0: the null pointer is not touched
        at += n;
        std::free(rows);
        if (gsdr_stats_rows(s) != at) ++bad;
    }
    const size_t counters = (size_t)n_ch * (size_t)(n_bins + 3);
    gsdr_stats_summary *sum = block<gsdr_stats_summary>((size_t)n_ch);
    unsigned long long *cnt = block<unsigned long long>(counters);
    const int n_p = 3;
    double *pr = block<double>(n_p), *q = block<double>((size_t)n_ch * n_p);
    pr[0] = 0.01, pr[1] = 0.5, pr[2] = 1.0;
    gsdr_trigger_level *lv = block<gsdr_trigger_level>((size_t)n_ch);
    unsigned char *on = block<unsigned char>((size_t)n_ch);
    for (int c = 0; c < n_ch; ++c) on[c] = c != 1;
    if (gsdr_stats_read_host(s, sum) != 0 || gsdr_stats_counts(s, cnt, nullptr) != 0 || gsdr_stats_quantiles(s, pr, n_p, q, nullptr) != 0) ++bad;
    out.add(sum, sizeof(gsdr_stats_summary) * (size_t)n_ch), out.add(cnt, 8 * counters), out.add(q, 8 * (size_t)n_ch * n_p);
    for (int centre = 0; centre < 2; ++centre) {
        if (gsdr_stats_levels(s, centre, 4.0, centre ? on : nullptr, lv, nullptr) != 0) ++bad;
        out.add(lv, sizeof(gsdr_trigger_level) * (size_t)n_ch);
        if (centre && n_ch > 1 && !(std::isinf(lv[1].lo) && std::isinf(lv[1].hi))) ++bad;
    }
    // what the counters add up to
    for (int c = 0; c < n_ch; ++c) {
        unsigned long long all = 0;
        for (int b = 0; b < n_bins + 3; ++b) all += cnt[(size_t)c * (n_bins + 3) + b];
        if (all != (unsigned long long)at || sum[c].n + sum[c].bad != all) ++bad;
        if (at >= 2 && !(sum[c].var >= 0.0 && sum[c].min <= sum[c].max)) ++bad;
    }
    // refusals leave the state as it was
    if (gsdr_stats_feed_host(s, x.data(), -1) != -1 || gsdr_stats_feed_host(s, x.data(), max_rows + 1) != -1 || gsdr_stats_feed_host(s, nullptr, 1) != -1 ||
        gsdr_stats_read_host(s, nullptr) != -1 || gsdr_stats_counts(s, nullptr, nullptr) != -1 || gsdr_stats_quantiles(s, pr, 0, q, nullptr) != -1 ||
        gsdr_stats_quantiles(s, pr, GSDR_STATS_MAX_QUANTILES + 1, q, nullptr) != -1 || gsdr_stats_quantiles(s, nullptr, 1, q, nullptr) != -1 ||
        gsdr_stats_quantiles(s, pr, 1, nullptr, nullptr) != -1 || gsdr_stats_levels(s, 2, 1.0, nullptr, lv, nullptr) != -1 ||
        gsdr_stats_levels(s, 0, -1.0, nullptr, lv, nullptr) != -1 || gsdr_stats_levels(s, 0, 1.0, nullptr, nullptr, nullptr) != -1 ||
        gsdr_stats_rows(s) != at)
        ++bad;
    pr[1] = 0.0;
    if (gsdr_stats_quantiles(s, pr, n_p, q, nullptr) != -1) ++bad;
    axes[n_ch - 1].hi = axes[n_ch - 1].lo;
    if (gsdr_stats_reset(s, axes) != -1 || gsdr_stats_rows(s) != at) ++bad;
    axes[n_ch - 1].hi = 1e30f, axes[n_ch - 1].lo = -1e30f;
    if (gsdr_stats_reset(s, axes) != 0 || gsdr_stats_rows(s) != 0 || gsdr_stats_read_host(s, sum) != 0 || sum[0].n != 0 || !std::isnan(sum[0].mean)) ++bad;
    if (gsdr_stats_reset(s, nullptr) != 0) ++bad;
    std::free(sum), std::free(cnt), std::free(pr), std::free(q), std::free(lv), std::free(on), std::free(axes);
    gsdr_stats_close(s);
    return bad;
}

int main() {
    int bad = 0, runs = 0;
    // n_ch, rows, n_bins, lanes, max_rows
    const int shapes[][5] = {{1, 1, 1, 1, 1}, {3, 257, 7, 4, 257}, {5, 700, 256, 64, 300}, {2, 90, 4096, 0, 64}, {1, 10, 4, 32768, 10}, {16, 333, 33, 2, 333}};
    for (const auto &sh : shapes) {
        const int n_ch = sh[0], n_bins = sh[2], lanes = sh[3], max_rows = sh[4];
        const long long rows = sh[1];
        std::vector<gsdr_c64> x = stream(rows, n_ch);
        std::vector<long long> whole, sevens, ones, gaps;
        for (long long at = 0; at < rows; at += max_rows) whole.push_back(rows - at < max_rows ? rows - at : max_rows);
        const long long piece = max_rows < 7 ? max_rows : 7;
        for (long long at = 0; at < rows; at += piece) sevens.push_back(rows - at < piece ? rows - at : piece);
        ones.assign((size_t)rows, 1);
        gaps.push_back(0), gaps.push_back(1), gaps.push_back(0), gaps.push_back(0);
        for (long long at = 1; at < rows; at += max_rows) gaps.push_back(rows - at < max_rows ? rows - at : max_rows);
        gaps.push_back(0);
        whole.push_back(-1), sevens.push_back(-1), ones.push_back(-1), gaps.push_back(-1);
        Result a, b, c, d, e;
        bad += run(x, n_ch, max_rows, n_bins, lanes, whole.data(), a);
        bad += run(x, n_ch, max_rows, n_bins, lanes, sevens.data(), b);
        bad += run(x, n_ch, max_rows, n_bins, lanes, ones.data(), c);
        bad += run(x, n_ch, max_rows, n_bins, lanes, gaps.data(), d);
        if (a.bytes != b.bytes || a.bytes != c.bytes || a.bytes != d.bytes) ++bad;      // the twin does not see the cutting
        // poison in channel 0 changes channel 0 alone
        x[0].x = std::numeric_limits<float>::infinity();
        x[(size_t)(rows / 2) * n_ch].y = std::numeric_limits<float>::quiet_NaN();
        x[(size_t)(rows - 1) * n_ch].x = 3e38f;
        bad += run(x, n_ch, max_rows, n_bins, lanes, sevens.data(), e);
        const size_t ss = sizeof(gsdr_stats_summary);
        if (n_ch > 1 && std::memcmp(e.bytes.data() + ss, a.bytes.data() + ss, ss * (size_t)(n_ch - 1)) != 0) ++bad;
        gsdr_stats_summary s0;
        std::memcpy(&s0, e.bytes.data(), ss);
        if (s0.bad < 1 || s0.n + s0.bad != (unsigned long long)rows) ++bad;
        runs += 5;
    }
    // a refusal leaves a NULL and no allocation behind
    gsdr_trigger_level ax[2] = {{0, 0, 1, 0, -1, 1}, {0, 0, 1, 0, -1, 1}};
    if (gsdr_stats_create(0, 8, 4, 1, ax, GSDR_STATS_HOST)) ++bad;
    if (gsdr_stats_create(2, 0, 4, 1, ax, GSDR_STATS_HOST)) ++bad;
    if (gsdr_stats_create(2, 8, 0, 1, ax, GSDR_STATS_HOST)) ++bad;
    if (gsdr_stats_create(2, 8, GSDR_STATS_MAX_BINS + 1, 1, ax, GSDR_STATS_HOST)) ++bad;
    if (gsdr_stats_create(2, 8, 4, 3, ax, GSDR_STATS_HOST)) ++bad;
    if (gsdr_stats_create(2, 8, 4, 2 * GSDR_STATS_MAX_LANES, ax, GSDR_STATS_HOST)) ++bad;
    if (gsdr_stats_create(2, 8, 4, 1, nullptr, GSDR_STATS_HOST)) ++bad;
    if (gsdr_stats_create(2, 8, 4, 1, ax, -3)) ++bad;
    if (gsdr_stats_create(2, 8, 4, 1, ax, 0)) ++bad;                   // no device part in this build
    ax[1].lo = std::numeric_limits<float>::quiet_NaN();
    if (gsdr_stats_create(2, 8, 4, 1, ax, GSDR_STATS_HOST)) ++bad;
    ax[1].lo = 1.0f;
    if (gsdr_stats_create(2, 8, 4, 1, ax, GSDR_STATS_HOST)) ++bad;
    gsdr_stats_close(nullptr);
    gsdr_stats_summary sm[1];
    double one = 0.5, qq[1];
    unsigned long long cc[8];
    if (gsdr_stats_reset(nullptr, nullptr) != -1 || gsdr_stats_feed_host(nullptr, nullptr, 0) != -1 || gsdr_stats_read_host(nullptr, sm) != -1 ||
        gsdr_stats_counts(nullptr, cc, nullptr) != -1 || gsdr_stats_quantiles(nullptr, &one, 1, qq, nullptr) != -1 ||
        gsdr_stats_levels(nullptr, 0, 1.0, nullptr, ax, nullptr) != -1 || gsdr_stats_rows(nullptr) != 0 || gsdr_stats_lanes(nullptr) != 0 ||
        gsdr_stats_n_bins(nullptr) != 0)
        ++bad;
    // levels that overflow float32 become infinite, with no conversion out of range
    gsdr_trigger_level big[1] = {{0, 0, 1, 0, -3e38f, 3e38f}};
    gsdr_stats *s = gsdr_stats_create(1, 4, 8, 1, big, GSDR_STATS_HOST);
    gsdr_c64 two[2] = {{-3e38f, 0}, {2.9e38f, 0}};
    if (!s || gsdr_stats_feed_host(s, two, 2) != 0 || gsdr_stats_levels(s, GSDR_STATS_CENTRE_MEAN, 10.0, nullptr, big, nullptr) != 0 ||
        !(std::isinf(big[0].lo) && big[0].lo < 0 && std::isinf(big[0].hi) && big[0].hi > 0))
        ++bad;
    gsdr_stats_close(s);
    std::printf("runs %d bad %d\n", runs, bad);
    return bad ? 1 : 0;
}
'''


def test_stats_host_under_asan_and_ubsan(tmp_path):
    run = build_and_run(DRIVER, tmp_path)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.strip() == "runs 30 bad 0", run.stdout
