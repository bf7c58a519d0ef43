"""The FIR decimator's host twin (gsdr_decim_* in decim_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: a
stand-alone program with its own main, built from the host sources alone with plain g++ (no HIP header, no device part:
only GSDR_DECIM_HOST objects exist in such a build).  Every buffer is a heap block of exactly the documented extent, so
one sample read or written past an end is a report.  Nothing is loaded into Python, nothing is preloaded; built exactly
as tests/test_welch_sanitizers.py builds its program."""
from _sanitized import build_and_run

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "gsdr.h"

static std::vector<gsdr_c64> stream(int rows, int n_ch) {
    std::vector<gsdr_c64> x((size_t)rows * n_ch);
    unsigned s = 4711u;
    for (auto &v : x) {
        s = s * 1664525u + 1013904223u;
        v.x = 0.3f + ((float)(s >> 8) / 16777216.0f - 0.5f);
        s = s * 1664525u + 1013904223u;
        v.y = 0.4f + ((float)(s >> 8) / 16777216.0f - 0.5f);
    }
    return x;
}

static long long n_out(long long total, long long p, int q) { return total <= p ? 0 : (total - 1 - p) / q + 1; }

// feeds the stream cut as `cut` (terminated by -1): the rows and the output of every feed are heap blocks of their exact
// extents; the emitted rows go into `out`
static int run(const std::vector<gsdr_c64> &x, int n_ch, int q, int T, long long p, const int *cut, std::vector<gsdr_c64> &out) {
    int max_rows = 1, total = 0;
    for (const int *c = cut; *c >= 0; ++c) max_rows = *c > max_rows ? *c : max_rows, total += *c;
    float *taps = T ? (float *)std::malloc(sizeof(float) * (size_t)T) : nullptr;
    for (int t = 0; t < T; ++t) taps[t] = (t % 5 == 2) ? 0.f : 0.01f * (float)((t * 7) % 13 - 6);
    gsdr_decim *d = gsdr_decim_create(n_ch, max_rows, q, T, taps, p, GSDR_DECIM_HOST);
    std::free(taps);                                       // the taps are copied by create
    if (!d) return 100;
    int bad = 0, at = 0;
    const int Tn = gsdr_decim_get_taps(d, nullptr, 0);
    {
        float *w = (float *)std::malloc(sizeof(float) * (size_t)Tn);
        if (gsdr_decim_get_taps(d, w, Tn) != Tn) ++bad;
        std::free(w);
    }
    if (gsdr_decim_out_capacity(d) != (max_rows - 1) / q + 1) ++bad;
    out.clear();
    for (const int *c = cut; *c >= 0; ++c) {
        const int n = *c, want = gsdr_decim_next_rows(d, n);
        if (want != (int)(n_out(at + n, p, q) - n_out(at, p, q))) ++bad;
        gsdr_c64 *rows = n ? (gsdr_c64 *)std::malloc(sizeof(gsdr_c64) * (size_t)n * n_ch) : nullptr;
        gsdr_c64 *y = want ? (gsdr_c64 *)std::malloc(sizeof(gsdr_c64) * (size_t)want * n_ch) : nullptr;
        if (n) std::memcpy(rows, x.data() + (size_t)at * n_ch, sizeof(gsdr_c64) * (size_t)n * n_ch);
        if (gsdr_decim_feed_host(d, rows, n, y) != want) ++bad;      // n == 0, want == 0: the null pointers are not touched
        out.insert(out.end(), y, y + (size_t)want * n_ch);
        at += n;
        std::free(rows);
        std::free(y);
    }
    if (gsdr_decim_rows(d) != total || gsdr_decim_rows_out(d) != n_out(total, p, q)) ++bad;
    if (gsdr_decim_feed_host(d, x.data(), max_rows + 1, nullptr) != -1 || gsdr_decim_rows(d) != total) ++bad;
    if (gsdr_decim_reset(d) != 0 || gsdr_decim_rows(d) != 0 || gsdr_decim_rows_out(d) != 0) ++bad;
    gsdr_decim_close(d);
    return bad;
}

static bool same(const std::vector<gsdr_c64> &a, const std::vector<gsdr_c64> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(gsdr_c64)) == 0);
}

int main() {
    int bad = 0, runs = 0;
    // n_ch, q, T (0: the default taps), offset
    const long long shapes[][4] = {{3, 1, 5, 0}, {2, 2, 0, 20}, {3, 7, 6, 6}, {1, 7, 17, 30}, {2, 16, 16 * 64, 15}, {1, 5, 11, 0}};
    for (const auto &sh : shapes) {
        const int n_ch = (int)sh[0], q = (int)sh[1], T = (int)sh[2], rows = (int)sh[3] + 12 * q + 5;
        std::vector<gsdr_c64> x = stream(rows, n_ch);
        const int whole[] = {rows, -1}, gaps[] = {3, 0, q + 1, 0, rows - q - 4, -1};
        std::vector<int> sevens, ones(rows, 1);
        for (int at = 0; at < rows; at += 7) sevens.push_back(rows - at < 7 ? rows - at : 7);
        sevens.push_back(-1), ones.push_back(-1);
        std::vector<gsdr_c64> a, b, c, d, e;
        bad += run(x, n_ch, q, T, sh[3], whole, a);
        bad += run(x, n_ch, q, T, sh[3], gaps, b);
        bad += run(x, n_ch, q, T, sh[3], sevens.data(), c);
        bad += run(x, n_ch, q, T, sh[3], ones.data(), d);
        if (!same(a, b) || !same(a, c) || !same(a, d) || a.empty()) ++bad;    // the twin does not see the cutting
        // poison: an Inf and a NaN in channel 0 reach some outputs of that channel and no other channel
        x[(size_t)(rows / 2) * n_ch].x = std::numeric_limits<float>::infinity();
        x[(size_t)(rows / 2 + 1) * n_ch].y = std::numeric_limits<float>::quiet_NaN();
        bad += run(x, n_ch, q, T, sh[3], sevens.data(), e);
        int hit = 0;
        for (size_t i = 0; i < e.size() && e.size() == a.size(); ++i) {
            const bool finite = std::isfinite(e[i].x) && std::isfinite(e[i].y);
            if (i % n_ch == 0) hit += !finite;
            else if (std::memcmp(&e[i], &a[i], sizeof(gsdr_c64)) != 0) ++bad;
        }
        if (e.size() != a.size() || hit == 0) ++bad;
        runs += 5;
    }
    // a refusal leaves a NULL and no allocation behind
    const float one = 1.f, inf = std::numeric_limits<float>::infinity();
    if (gsdr_decim_create(2, 64, 0, 1, &one, 0, GSDR_DECIM_HOST)) ++bad;
    if (gsdr_decim_create(2, 64, 4, 1, &inf, 0, GSDR_DECIM_HOST)) ++bad;
    if (gsdr_decim_create(2, 64, 1, 0, nullptr, 0, GSDR_DECIM_HOST)) ++bad;
    if (gsdr_decim_create(2, 64, 4, 1, &one, 0, 0)) ++bad;             // no device part in this build
    float w[41];
    if (gsdr_decim_default_taps(2, w) != 41 || gsdr_decim_default_taps(1, w) != -1) ++bad;
    gsdr_decim_close(nullptr);
    if (gsdr_decim_reset(nullptr) != -1 || gsdr_decim_feed_host(nullptr, nullptr, 0, nullptr) != -1 || gsdr_decim_rows(nullptr) != 0) ++bad;
    std::printf("runs %d bad %d\n", runs, bad);
    return bad ? 1 : 0;
}
'''


def test_decim_host_under_asan_and_ubsan(tmp_path):
    run = build_and_run(DRIVER, tmp_path)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.strip() == "runs 30 bad 0", run.stdout
