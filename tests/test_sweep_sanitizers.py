"""The sweep accumulator's host twin (gsdr_sweep_* in sweep_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer:
a stand-alone program with its own main, built from the host sources alone with plain g++ (no HIP header, no device part:
only GSDR_SWEEP_HOST objects exist in such a build).  Every buffer is a heap block of exactly the documented extent, so
one sample read or written past an end is a report.  Nothing is loaded into Python, nothing is preloaded; built exactly
as tests/test_decim_sanitizers.py builds its program."""
from _sanitized import build_and_run

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "gsdr.h"

static std::vector<gsdr_c64> stream(long long rows, int n_ch) {
    std::vector<gsdr_c64> x((size_t)rows * n_ch);
    unsigned s = 4711u;
    for (auto &v : x) {
        s = s * 1664525u + 1013904223u;
        v.x = 0.3f + 0.01f * ((float)(s >> 8) / 16777216.0f - 0.5f);
        s = s * 1664525u + 1013904223u;
        v.y = -0.4f + 0.01f * ((float)(s >> 8) / 16777216.0f - 0.5f);
    }
    return x;
}

struct Result {
    std::vector<gsdr_c64> mean, var;
    std::vector<double> d;
};

// feeds the stream cut as `cut` (terminated by -1): the rows of every feed and every result are heap blocks of their
// exact extents
static int run(const std::vector<gsdr_c64> &x, int n_ch, long long n_points, long long group, long long first_row, const long long *cut, Result &out) {
    gsdr_sweep *s = gsdr_sweep_create(n_ch, n_points, group, first_row, GSDR_SWEEP_HOST);
    if (!s) return 100;
    int bad = 0;
    long long at = 0;
    for (const long long *c = cut; *c >= 0; ++c) {
        const int n = (int)*c;
        gsdr_c64 *rows = n ? (gsdr_c64 *)std::malloc(sizeof(gsdr_c64) * (size_t)n * n_ch) : nullptr;
        if (n) std::memcpy(rows, x.data() + (size_t)at * n_ch, sizeof(gsdr_c64) * (size_t)n * n_ch);
        if (gsdr_sweep_feed_host(s, rows, n) != 0) ++bad;              // n == 0: the null pointer is not touched
        at += n;
        std::free(rows);
        if (gsdr_sweep_rows(s) != at) ++bad;
    }
    // the counts against enumeration
    std::vector<long long> cnt((size_t)n_points, 0);
    for (long long i = 0; i < at; ++i) ++cnt[(size_t)(((first_row + i) / group) % n_points)];
    long long least = cnt[0];
    for (long long p = 0; p < n_points; ++p) {
        if (gsdr_sweep_point_rows(s, p) != cnt[(size_t)p]) ++bad;
        least = cnt[(size_t)p] < least ? cnt[(size_t)p] : least;
    }
    if (gsdr_sweep_sweeps(s) != least / group || gsdr_sweep_point_rows(s, -1) != 0 || gsdr_sweep_point_rows(s, n_points) != 0) ++bad;
    const size_t cells = (size_t)n_points * n_ch;
    gsdr_c64 *mean = (gsdr_c64 *)std::malloc(sizeof(gsdr_c64) * cells), *var = (gsdr_c64 *)std::malloc(sizeof(gsdr_c64) * cells);
    gsdr_c64 *mean2 = (gsdr_c64 *)std::malloc(sizeof(gsdr_c64) * cells);
    double *d = (double *)std::malloc(sizeof(double) * 2 * (size_t)n_ch);
    if (gsdr_sweep_read_host(s, mean, var) != 0 || gsdr_sweep_read_host(s, mean2, nullptr) != 0 || gsdr_sweep_slope(s, d, nullptr) != 0) ++bad;
    if (std::memcmp(mean, mean2, sizeof(gsdr_c64) * cells) != 0) ++bad;
    out.mean.assign(mean, mean + cells), out.var.assign(var, var + cells), out.d.assign(d, d + 2 * (size_t)n_ch);
    std::free(mean), std::free(mean2), std::free(var), std::free(d);
    // refusals leave the state as it was
    if (gsdr_sweep_feed_host(s, x.data(), -1) != -1 || gsdr_sweep_feed_host(s, x.data(), GSDR_SWEEP_MAX_FEED + 1) != -1 ||
        gsdr_sweep_feed_host(s, nullptr, 1) != -1 || gsdr_sweep_read_host(s, nullptr, nullptr) != -1 || gsdr_sweep_slope(s, nullptr, nullptr) != -1 ||
        gsdr_sweep_reset(s, -1) != -1 || gsdr_sweep_rows(s) != at)
        ++bad;
    if (gsdr_sweep_reset(s, 7) != 0 || gsdr_sweep_rows(s) != 0 || gsdr_sweep_sweeps(s) != 0) ++bad;
    gsdr_sweep_close(s);
    return bad;
}

static bool same(const Result &a, const Result &b) {
    return a.mean.size() == b.mean.size() && std::memcmp(a.mean.data(), b.mean.data(), a.mean.size() * sizeof(gsdr_c64)) == 0 &&
           std::memcmp(a.var.data(), b.var.data(), a.var.size() * sizeof(gsdr_c64)) == 0 && a.d.size() == b.d.size() &&
           std::memcmp(a.d.data(), b.d.data(), a.d.size() * sizeof(double)) == 0;
}

int main() {
    int bad = 0, runs = 0;
    // n_ch, n_points, group, first_row
    const long long shapes[][4] = {{1, 5, 1, 0}, {3, 67, 1, 3}, {16, 300, 1, (1LL << 40) + 17}, {2, 25, 40, 3}, {1, 7, 3, (1LL << 62)}, {2, 1, 1, 0}};
    for (const auto &sh : shapes) {
        const int n_ch = (int)sh[0];
        const long long P = sh[1], g = sh[2], W = P * g, rows = 2 * W + (3 * W) / 7 + 2;
        std::vector<gsdr_c64> x = stream(rows, n_ch);
        const long long whole[] = {rows, -1}, gaps[] = {0, 3 < rows ? 3 : rows, 0, 0, rows - (3 < rows ? 3 : rows), 0, -1};
        const long long lng[] = {1, 2 * W + 1, rows - 2 * W - 2, -1};
        std::vector<long long> sevens, ones((size_t)rows, 1);
        for (long long at = 0; at < rows; at += 7) sevens.push_back(rows - at < 7 ? rows - at : 7);
        sevens.push_back(-1), ones.push_back(-1);
        Result a, b, c, d, e, f;
        bad += run(x, n_ch, P, g, sh[3], whole, a);
        bad += run(x, n_ch, P, g, sh[3], gaps, b);
        bad += run(x, n_ch, P, g, sh[3], sevens.data(), c);
        bad += run(x, n_ch, P, g, sh[3], ones.data(), d);
        bad += run(x, n_ch, P, g, sh[3], lng, e);
        if (!same(a, b) || !same(a, c) || !same(a, d) || !same(a, e)) ++bad;      // the twin does not see the cutting
        for (const gsdr_c64 &v : a.var)
            if (!(v.x > 0.f) || !(v.y > 0.f)) ++bad;
        // poison: an Inf and a NaN in channel 0 reach their two accumulators and nothing else
        const long long r1 = rows / 3, r2 = rows / 2;
        x[(size_t)r1 * n_ch].x = std::numeric_limits<float>::infinity();
        x[(size_t)r2 * n_ch].y = std::numeric_limits<float>::quiet_NaN();
        const long long p1 = ((sh[3] + r1) / g) % P, p2 = ((sh[3] + r2) / g) % P;
        bad += run(x, n_ch, P, g, sh[3], sevens.data(), f);
        for (size_t i = 0; i < f.mean.size(); ++i) {
            const bool hit = i == (size_t)p1 * n_ch || i == (size_t)p2 * n_ch;
            const bool finite = std::isfinite(f.mean[i].x) && std::isfinite(f.mean[i].y) && std::isfinite(f.var[i].x) && std::isfinite(f.var[i].y);
            if (hit ? finite : (std::memcmp(&f.mean[i], &a.mean[i], sizeof(gsdr_c64)) != 0 || std::memcmp(&f.var[i], &a.var[i], sizeof(gsdr_c64)) != 0)) ++bad;
        }
        for (int ch = 1; ch < n_ch; ++ch)
            if (std::memcmp(&f.d[2 * (size_t)ch], &a.d[2 * (size_t)ch], 2 * sizeof(double)) != 0) ++bad;
        runs += 6;
    }
    // a refusal leaves a NULL and no allocation behind
    if (gsdr_sweep_create(0, 5, 1, 0, GSDR_SWEEP_HOST)) ++bad;
    if (gsdr_sweep_create(1, 0, 1, 0, GSDR_SWEEP_HOST)) ++bad;
    if (gsdr_sweep_create(3, 1LL << 24, 1, 0, GSDR_SWEEP_HOST)) ++bad;
    if (gsdr_sweep_create(1, 5, 0, 0, GSDR_SWEEP_HOST)) ++bad;
    if (gsdr_sweep_create(1, 5, 1, -1, GSDR_SWEEP_HOST)) ++bad;
    if (gsdr_sweep_create(1, 5, 1, (1LL << 62) + 1, GSDR_SWEEP_HOST)) ++bad;
    if (gsdr_sweep_create(1, 5, 1, 0, -3)) ++bad;
    if (gsdr_sweep_create(1, 5, 1, 0, 0)) ++bad;                       // no device part in this build
    gsdr_sweep_close(nullptr);
    double dd[2];
    gsdr_c64 m[1];
    if (gsdr_sweep_reset(nullptr, 0) != -1 || gsdr_sweep_feed_host(nullptr, nullptr, 0) != -1 || gsdr_sweep_read_host(nullptr, m, nullptr) != -1 ||
        gsdr_sweep_slope(nullptr, dd, nullptr) != -1 || gsdr_sweep_rows(nullptr) != 0 || gsdr_sweep_sweeps(nullptr) != 0 || gsdr_sweep_point_rows(nullptr, 0) != 0)
        ++bad;
    // the helpers: the axis is written to exactly n_points doubles
    for (long long n = 1; n <= 9; n += 4) {
        double *f = (double *)std::malloc(sizeof(double) * (size_t)n);
        if (gsdr_vna_axis(2e8, -9e7, 9e7, 1000, n, 3e8, f) != 0 || f[0] != 3e8 - 9e7) ++bad;
        std::free(f);
    }
    if (gsdr_vna_axis(2e8, -9e7, 9e7, 1, 5, 0, dd) != -1 || gsdr_vna_axis(2e8, -9e7, 9e7, 1000, 5, 0, nullptr) != -1) ++bad;
    gsdr_chirp_param cp;
    long long np = 0, grp = 0;
    gsdr_chirp_derive(200000000, -100000000, 100000000, 1000000, 1.0f, &cp);
    if (gsdr_sweep_shape_for_chirp(&cp, 0, &np, &grp) != 0 || np != 1000000 || grp != 200) ++bad;
    if (gsdr_sweep_shape_for_chirp(&cp, 4, &np, &grp) != 0 || np != 250000 || grp != 1) ++bad;
    if (gsdr_sweep_shape_for_chirp(&cp, 3, &np, &grp) != -1 || gsdr_sweep_shape_for_chirp(&cp, -1, &np, &grp) != -1 ||
        gsdr_sweep_shape_for_chirp(nullptr, 1, &np, &grp) != -1)
        ++bad;
    std::printf("runs %d bad %d\n", runs, bad);
    return bad ? 1 : 0;
}
'''


def test_sweep_host_under_asan_and_ubsan(tmp_path):
    run = build_and_run(DRIVER, tmp_path)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.strip() == "runs 36 bad 0", run.stdout
