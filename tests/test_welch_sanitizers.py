"""The Welch host twin (gsdr_welch_* in welch_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: a
stand-alone program with its own main, built from the host sources alone with plain g++ (no HIP header, no device part:
only GSDR_WELCH_HOST objects exist in such a build).  Every buffer is a heap block of exactly the documented extent, so
one sample read or written past an end is a report.  Nothing is loaded into Python, nothing is preloaded; in the style
of tests/test_trigger_sanitizers.py."""
from _sanitized import build_and_run

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "gsdr.h"

static std::vector<gsdr_c64> stream(int rows, int n_ch) {
    std::vector<gsdr_c64> x((size_t)rows * n_ch);
    unsigned s = 4711u;
    for (auto &v : x) {                                   // a carrier of 1 and noise within +-1e-3
        s = s * 1664525u + 1013904223u;
        v.x = 1.0f + ((float)(s >> 8) / 16777216.0f - 0.5f) * 2e-3f;
        s = s * 1664525u + 1013904223u;
        v.y = ((float)(s >> 8) / 16777216.0f - 0.5f) * 2e-3f;
    }
    return x;
}

// feeds the stream cut as `cut` (terminated by -1), every buffer a heap block of its exact extent; the spectra of all
// four modes and the mean go into `out`
static int run(const std::vector<gsdr_c64> &x, int n_ch, int nperseg, int step, int detrend, bool own_window, const int *cut,
               std::vector<double> &out) {
    int max_rows = 1, total = 0;
    for (const int *c = cut; *c >= 0; ++c) max_rows = *c > max_rows ? *c : max_rows, total += *c;
    float *win = nullptr;
    if (own_window) {
        win = (float *)std::malloc(sizeof(float) * (size_t)nperseg);
        for (int n = 0; n < nperseg; ++n) win[n] = 0.3f + 0.01f * (float)(n % 7);
    }
    gsdr_welch *w = gsdr_welch_create(n_ch, max_rows, nperseg, step, detrend, win, GSDR_WELCH_HOST);
    std::free(win);                                       // the window is copied by create
    if (!w) return 100;
    int bad = 0, at = 0;
    const size_t K1 = (size_t)nperseg / 2 + 1, per = (size_t)n_ch * 2 * K1;
    // a read before the first segment returns 0 and writes nothing
    {
        double *psd = (double *)std::malloc(sizeof(double) * per);
        for (size_t i = 0; i < per; ++i) psd[i] = 7.0;
        if (gsdr_welch_read_host(w, GSDR_WELCH_ROTATE, nullptr, 1.0, psd, nullptr) != 0) ++bad;
        for (size_t i = 0; i < per; ++i)
            if (psd[i] != 7.0) { ++bad; break; }
        std::free(psd);
    }
    for (const int *c = cut; *c >= 0; ++c) {
        const int n = *c;
        gsdr_c64 *rows = n ? (gsdr_c64 *)std::malloc(sizeof(gsdr_c64) * (size_t)n * n_ch) : nullptr;
        if (n) std::memcpy(rows, x.data() + (size_t)at * n_ch, sizeof(gsdr_c64) * (size_t)n * n_ch);
        if (gsdr_welch_feed_host(w, rows, n) != 0) ++bad;  // n == 0: the null pointer is not touched
        at += n;
        std::free(rows);
    }
    const long long want = total < nperseg ? 0 : (total - nperseg) / step + 1;
    if (gsdr_welch_rows(w) != total || gsdr_welch_segments(w) != want) ++bad;
    out.assign(4 * per + (size_t)n_ch * 2, 0.0);
    gsdr_c64 *gain = (gsdr_c64 *)std::malloc(sizeof(gsdr_c64) * (size_t)n_ch);
    for (int c = 0; c < n_ch; ++c) gain[c].x = 0.5f + (float)c, gain[c].y = -0.25f * (float)c;
    for (int mode = 0; mode < 4; ++mode) {
        double *psd = (double *)std::malloc(sizeof(double) * per);
        double *mean = (double *)std::malloc(sizeof(double) * (size_t)n_ch * 2);
        const int n_seg = gsdr_welch_read_host(w, mode, mode == GSDR_WELCH_GAIN ? gain : nullptr, 1e6, psd, mode == 1 ? mean : nullptr);
        if (n_seg != (int)want) ++bad;
        if (n_seg > 0) {
            std::memcpy(out.data() + (size_t)mode * per, psd, sizeof(double) * per);
            if (mode == 1) std::memcpy(out.data() + 4 * per, mean, sizeof(double) * (size_t)n_ch * 2);
            for (size_t i = 0; i < per; ++i)
                if (!(psd[i] > 0.0) || !std::isfinite(psd[i])) { ++bad; break; }
        }
        std::free(psd);
        std::free(mean);
    }
    std::free(gain);
    if (gsdr_welch_reset(w) != 0 || gsdr_welch_rows(w) != 0 || gsdr_welch_segments(w) != 0) ++bad;
    gsdr_welch_close(w);
    return bad;
}

int main() {
    int bad = 0, runs = 0;
    const int shapes[][5] = {{3, 16, 16, 2, 0}, {3, 16, 2, 2, 1}, {2, 64, 32, 1, 0}, {1, 256, 100, 0, 1}, {2, 1024, 512, 2, 0}};
    for (const auto &sh : shapes) {
        const int n_ch = sh[0], N = sh[1], step = sh[2], rows = 4 * N + 3 * step + 5;
        const std::vector<gsdr_c64> x = stream(rows, n_ch);
        const int whole[] = {rows, -1}, gaps[] = {3, 0, N + 1, 0, rows - N - 4, -1}, tiny[] = {N - 1, -1};
        std::vector<int> sevens;
        for (int at = 0; at < rows; at += 7) sevens.push_back(rows - at < 7 ? rows - at : 7);
        sevens.push_back(-1);
        std::vector<double> a, b, c, d;
        bad += run(x, n_ch, N, step, sh[3], sh[4] != 0, whole, a);
        bad += run(x, n_ch, N, step, sh[3], sh[4] != 0, gaps, b);
        bad += run(x, n_ch, N, step, sh[3], sh[4] != 0, sevens.data(), c);
        bad += run(x, n_ch, N, step, sh[3], sh[4] != 0, tiny, d);       // no segment: every read returns 0
        if (a != b || a != c) ++bad;                                     // the twin does not see the cutting
        runs += 4;
    }
    // a refusal leaves a NULL and no allocation behind
    if (gsdr_welch_create(2, 64, 48, 24, 2, nullptr, GSDR_WELCH_HOST)) ++bad;
    if (gsdr_welch_create(2, 64, 64, 4, 2, nullptr, GSDR_WELCH_HOST)) ++bad;
    if (gsdr_welch_create(2, 64, 64, 32, 2, nullptr, 0)) ++bad;         // no device part in this build
    gsdr_welch_close(nullptr);
    std::printf("runs %d bad %d\n", runs, bad);
    return bad ? 1 : 0;
}
'''


def test_welch_host_under_asan_and_ubsan(tmp_path):
    run = build_and_run(DRIVER, tmp_path)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.strip() == "runs 20 bad 0", run.stdout
