"""The channel covariance's host twin (gsdr_cov_* in cov_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: a
stand-alone program with its own main, built from the host sources alone with plain g++ (no HIP header, no device part:
only GSDR_COV_HOST objects exist in such a build).  Every buffer -- the axes, the rows of a feed, the matrix, the means
-- is a heap block of exactly the documented extent, so one element read or written past an end is a report.  Nothing is
loaded into Python, nothing is preloaded; built exactly as tests/test_stats_sanitizers.py builds its program."""
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
    std::vector<unsigned char> bytes;        // the three matrices and their means, one after the other
    void add(const void *p, size_t n) { bytes.insert(bytes.end(), (const unsigned char *)p, (const unsigned char *)p + n); }
};

static gsdr_cov_axis *axes_of(int n_var, int n_ch) {
    gsdr_cov_axis *axes = block<gsdr_cov_axis>((size_t)n_var);
    for (int i = 0; i < n_var; ++i) axes[i] = gsdr_cov_axis{(3 * i + 1) % n_ch, 0.1f, -0.2f, i % 2 ? 0.0f : 1.0f, i % 2 ? 1.0f : 0.5f, 0, i % 2 ? -0.2 : 0.1};
    return axes;
}

// feeds the stream cut as `cut` (terminated by -1) and reads everything
static int run(const std::vector<gsdr_c64> &x, int n_ch, int n_var, int max_rows, int lanes, const long long *cut, Result &out) {
    gsdr_cov_axis *axes = axes_of(n_var, n_ch);
    gsdr_cov *c = gsdr_cov_create(n_ch, n_var, max_rows, lanes, axes, GSDR_COV_HOST);
    if (!c) return 100;
    int bad = 0;
    if (gsdr_cov_n_var(c) != n_var || gsdr_cov_lanes(c) < 1 || (lanes && gsdr_cov_lanes(c) != lanes)) ++bad;
    long long at = 0;
    for (const long long *p = cut; *p >= 0; ++p) {
        const int n = (int)*p;
        gsdr_c64 *rows = n ? block<gsdr_c64>((size_t)n * n_ch) : nullptr;
        if (n) std::memcpy(rows, x.data() + (size_t)at * n_ch, sizeof(gsdr_c64) * (size_t)n * n_ch);
        if (gsdr_cov_feed_host(c, rows, n) != 0) ++bad;                // n == 0: the null pointer is not touched
        at += n;
        std::free(rows);
        if (gsdr_cov_rows(c) != at) ++bad;
    }
    const size_t nv = (size_t)n_var;
    double *m = block<double>(nv * nv), *mean = block<double>(nv);
    for (int kind = 0; kind < 3; ++kind) {
        if (gsdr_cov_read_host(c, kind, m, mean) != 0) ++bad;
        out.add(m, 8 * nv * nv), out.add(mean, 8 * nv);
        for (size_t i = 0; i < nv; ++i)
            for (size_t j = 0; j < i; ++j)
                if (std::memcmp(&m[i * nv + j], &m[j * nv + i], 8) != 0) ++bad;
        if (gsdr_cov_read_host(c, kind, m, nullptr) != 0) ++bad;       // the mean is optional
    }
    if (at >= 2)
        for (size_t i = 0; i < nv; ++i)
            if (!(m[i * nv + i] == 1.0)) ++bad;                        // the last read was GSDR_COV_CORR
    // refusals leave the state as it was
    if (gsdr_cov_feed_host(c, x.data(), -1) != -1 || gsdr_cov_feed_host(c, x.data(), max_rows + 1) != -1 || gsdr_cov_feed_host(c, nullptr, 1) != -1 ||
        gsdr_cov_read_host(c, 1, nullptr, mean) != -1 || gsdr_cov_read_host(c, 3, m, mean) != -1 || gsdr_cov_read_host(c, -1, m, mean) != -1 ||
        gsdr_cov_rows(c) != at)
        ++bad;
    axes[n_var - 1].channel = n_ch;
    if (gsdr_cov_reset(c, axes) != -1 || gsdr_cov_rows(c) != at) ++bad;
    axes[n_var - 1].channel = 0, axes[n_var - 1].pivot = std::numeric_limits<double>::infinity();
    if (gsdr_cov_reset(c, axes) != -1 || gsdr_cov_rows(c) != at) ++bad;
    axes[n_var - 1].pivot = 0.5;
    if (gsdr_cov_reset(c, axes) != 0 || gsdr_cov_rows(c) != 0 || gsdr_cov_read_host(c, 1, m, mean) != 0 || !std::isnan(m[0]) || !std::isnan(mean[0])) ++bad;
    if (gsdr_cov_read_host(c, 0, m, mean) != 0 || m[0] != 0.0 || mean[0] != 0.0) ++bad;
    if (gsdr_cov_reset(c, nullptr) != 0) ++bad;
    std::free(m), std::free(mean), std::free(axes);
    gsdr_cov_close(c);
    return bad;
}

int main() {
    int bad = 0, runs = 0;
    // n_ch, n_var, rows, lanes, max_rows
    const int shapes[][5] = {{1, 1, 1, 1, 1}, {3, 3, 257, 4, 257}, {5, 5, 300, 8, 300}, {4, 8, 120, 2, 50}, {2, 4, 10, 64, 10}, {2, 3, 90, 0, 64}, {7, 33, 60, 4096, 60}};
    for (const auto &sh : shapes) {
        const int n_ch = sh[0], n_var = sh[1], lanes = sh[3], max_rows = sh[4];
        const long long rows = sh[2];
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
        bad += run(x, n_ch, n_var, max_rows, lanes, whole.data(), a);
        bad += run(x, n_ch, n_var, max_rows, lanes, sevens.data(), b);
        bad += run(x, n_ch, n_var, max_rows, lanes, ones.data(), c);
        bad += run(x, n_ch, n_var, max_rows, lanes, gaps.data(), d);
        if (a.bytes != b.bytes || a.bytes != c.bytes || a.bytes != d.bytes) ++bad;      // the twin does not see the cutting
        runs += 4;
    }
    // poison in one variable's channel: Inf, NaN and 3e38 are taken as IEEE gives them, nothing is indexed by them
    {
        std::vector<gsdr_c64> x = stream(64, 4);                     // three variables on channels 1, 0 and 3
        x[0].x = std::numeric_limits<float>::infinity();
        x[(size_t)32 * 4].y = std::numeric_limits<float>::quiet_NaN();
        x[(size_t)63 * 4].x = 3e38f;
        const long long cut[] = {64, -1};
        Result r;
        if (run(x, 4, 3, 64, 4, cut, r) != 1) ++bad;                 // the diagonal of CORR is NaN in the poisoned variable, and there alone
        ++runs;
    }
    // a refusal leaves a NULL and no allocation behind
    gsdr_cov_axis ax[2] = {{0, 0, 0, 1, 0, 0, 0.0}, {1, 0, 0, 0, 1, 0, 0.0}};
    if (gsdr_cov_create(0, 2, 8, 1, ax, GSDR_COV_HOST)) ++bad;
    if (gsdr_cov_create((1 << 20) + 1, 2, 8, 1, ax, GSDR_COV_HOST)) ++bad;
    if (gsdr_cov_create(2, 0, 8, 1, ax, GSDR_COV_HOST)) ++bad;
    if (gsdr_cov_create(2, GSDR_COV_MAX_VARS + 1, 8, 1, ax, GSDR_COV_HOST)) ++bad;
    if (gsdr_cov_create(2, 2, 0, 1, ax, GSDR_COV_HOST)) ++bad;
    if (gsdr_cov_create(2, 2, (1 << 20) + 1, 1, ax, GSDR_COV_HOST)) ++bad;
    if (gsdr_cov_create(2, 2, 8, 3, ax, GSDR_COV_HOST)) ++bad;
    if (gsdr_cov_create(2, 2, 8, -2, ax, GSDR_COV_HOST)) ++bad;
    if (gsdr_cov_create(2, 2, 8, 2 * GSDR_COV_MAX_LANES, ax, GSDR_COV_HOST)) ++bad;
    if (gsdr_cov_create(2, GSDR_COV_MAX_VARS, 8, 32, ax, GSDR_COV_HOST)) ++bad;      // the bound on the cells, before axes[2 ..] is read
    if (gsdr_cov_create(2, 2, 8, 1, nullptr, GSDR_COV_HOST)) ++bad;
    if (gsdr_cov_create(2, 2, 8, 1, ax, -3)) ++bad;
    if (gsdr_cov_create(2, 2, 8, 1, ax, 0)) ++bad;                       // no device part in this build
    ax[1].channel = 2;
    if (gsdr_cov_create(2, 2, 8, 1, ax, GSDR_COV_HOST)) ++bad;
    ax[1].channel = -1;
    if (gsdr_cov_create(2, 2, 8, 1, ax, GSDR_COV_HOST)) ++bad;
    ax[1].channel = 1, ax[1].reserved = 7;
    if (gsdr_cov_create(2, 2, 8, 1, ax, GSDR_COV_HOST)) ++bad;
    ax[1].reserved = 0, ax[1].dx = std::numeric_limits<float>::quiet_NaN();
    if (gsdr_cov_create(2, 2, 8, 1, ax, GSDR_COV_HOST)) ++bad;
    ax[1].dx = 0, ax[0].pivot = -std::numeric_limits<double>::infinity();
    if (gsdr_cov_create(2, 2, 8, 1, ax, GSDR_COV_HOST)) ++bad;
    ax[0].pivot = 0;
    gsdr_cov *ok = gsdr_cov_create(2, 2, 8, 1, ax, GSDR_COV_HOST);
    if (!ok) ++bad;
    gsdr_cov_close(ok);
    gsdr_cov_close(nullptr);
    double m[4];
    int plan[6];
    if (gsdr_cov_reset(nullptr, nullptr) != -1 || gsdr_cov_feed_host(nullptr, nullptr, 0) != -1 || gsdr_cov_read_host(nullptr, 1, m, nullptr) != -1 ||
        gsdr_cov_rows(nullptr) != 0 || gsdr_cov_lanes(nullptr) != 0 || gsdr_cov_n_var(nullptr) != 0)
        ++bad;
    if (gsdr_cov_plan(4, 300, 8, plan) != 0 || plan[0] != 128 || plan[1] != 3 || plan[2] != 6 || plan[3] != 8 || plan[4] != 32768 || plan[5] != 256) ++bad;
    if (gsdr_cov_plan(4, 300, 8, nullptr) != -1 || gsdr_cov_plan(4, 300, 3, plan) != -1 || gsdr_cov_plan(4, 0, 8, plan) != -1 || gsdr_cov_plan(0, 3, 8, plan) != -1) ++bad;
    std::printf("runs %d bad %d\n", runs, bad);
    return bad ? 1 : 0;
}
'''


def test_cov_host_under_asan_and_ubsan(tmp_path):
    run = build_and_run(DRIVER, tmp_path)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.strip() == "runs 29 bad 0", run.stdout
