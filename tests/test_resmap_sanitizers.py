"""The resonator map's host twin and gsdr_resmap_constants (gsdr_resmap_* in resmap_host.cpp) under AddressSanitizer +
UndefinedBehaviorSanitizer: a stand-alone program with its own main, built from the host sources alone with plain g++ (no
HIP header, no device part: only GSDR_RESMAP_HOST objects exist in such a build).  Every buffer is a heap block of
exactly the documented extent, so one sample, constant, offset or channel read or written past an end is a report.
Nothing is loaded into Python, nothing is preloaded; built exactly as tests/test_sweep_sanitizers.py builds its
program."""
from _sanitized import build_and_run

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "gsdr.h"

template <typename T>
static T *block(size_t n) { return (T *)std::malloc(sizeof(T) * (n ? n : 1)); }

static bool same(const gsdr_c64 &a, const gsdr_c64 &b) {
    return ((a.x != a.x && b.x != b.x) || std::memcmp(&a.x, &b.x, 4) == 0) && ((a.y != a.y && b.y != b.y) || std::memcmp(&a.y, &b.y, 4) == 0);
}

// one shape, one kind: whole, cut, in place (identity), offsets, poison; every buffer of its exact extent
static int run(int n_ch, int n_rows, int n_out, const int *list, int kind) {
    int bad = 0;
    double *k = block<double>((size_t)n_out * GSDR_RESMAP_NCONST);
    for (int c = 0; c < n_out; ++c)
        if (gsdr_resmap_constants(4.0e8 + 1e3 * c, 400.0 + 1e-4 * c, 0.5 + 0.01 * c, 0.1 * c, 30.0 - c, 2e4 + 100.0 * c, 1e3 - 50.0 * c,
                                  k + (size_t)c * GSDR_RESMAP_NCONST) != 0)
            ++bad;
    int *channels = list ? block<int>((size_t)n_out) : nullptr;
    if (list) std::memcpy(channels, list, sizeof(int) * (size_t)n_out);
    gsdr_resmap *r = gsdr_resmap_create(n_ch, n_rows, n_out, channels, k, kind, GSDR_RESMAP_HOST);
    std::free(channels);                                           // the object keeps its own copies
    if (!r) {
        std::free(k);
        return 100;
    }
    int *got_ch = block<int>((size_t)n_out);
    double *got_k = block<double>((size_t)n_out * GSDR_RESMAP_NCONST), *got_xy = block<double>((size_t)n_out * 2);
    if (gsdr_resmap_n_out(r) != n_out || gsdr_resmap_kind(r) != kind || gsdr_resmap_get_channels(r, got_ch, n_out) != n_out ||
        gsdr_resmap_get_constants(r, got_k, n_out) != n_out || gsdr_resmap_get_offsets(r, got_xy, n_out) != n_out ||
        std::memcmp(got_k, k, sizeof(double) * (size_t)n_out * GSDR_RESMAP_NCONST) != 0)
        ++bad;
    bool identity = n_out == n_ch;
    for (int c = 0; c < n_out; ++c) {
        if (got_ch[c] != (list ? list[c] : c) || got_xy[2 * c] != 0.0 || got_xy[2 * c + 1] != 0.0) ++bad;
        identity = identity && got_ch[c] == c;
    }
    std::free(k);
    const size_t n_in = (size_t)n_rows * n_ch, n_o = (size_t)n_rows * n_out;
    gsdr_c64 *x = block<gsdr_c64>(n_in), *whole = block<gsdr_c64>(n_o);
    unsigned s = 4711u;
    for (size_t i = 0; i < n_in; ++i) {
        s = s * 1664525u + 1013904223u;
        x[i].x = 0.2f + 0.05f * ((float)(s >> 8) / 16777216.0f - 0.5f);
        s = s * 1664525u + 1013904223u;
        x[i].y = -0.1f + 0.05f * ((float)(s >> 8) / 16777216.0f - 0.5f);
    }
    if (gsdr_resmap_feed_host(r, x, n_rows, whole) != n_rows) ++bad;
    for (size_t i = 0; i < n_o; ++i)
        if (!std::isfinite(whole[i].x) || !std::isfinite(whole[i].y)) ++bad;
    // cut into feeds of 0, 1, the rest: each feed's rows and outputs are blocks of their own
    const int cut[3] = {0, n_rows > 1 ? 1 : n_rows, n_rows - (n_rows > 1 ? 1 : n_rows)};
    int at = 0;
    for (int n : cut) {
        gsdr_c64 *in = n ? block<gsdr_c64>((size_t)n * n_ch) : nullptr, *out = n ? block<gsdr_c64>((size_t)n * n_out) : nullptr;
        if (n) std::memcpy(in, x + (size_t)at * n_ch, sizeof(gsdr_c64) * (size_t)n * n_ch);
        if (gsdr_resmap_feed_host(r, in, n, out) != n) ++bad;     // n == 0: the null pointers are not touched
        for (size_t i = 0; i < (size_t)n * n_out; ++i)
            if (!same(out[i], whole[(size_t)at * n_out + i])) ++bad;
        std::free(in), std::free(out);
        at += n;
    }
    // in place with the identity; refused otherwise, and the buffer is left as it was
    {
        gsdr_c64 *io = block<gsdr_c64>(n_in);
        std::memcpy(io, x, sizeof(gsdr_c64) * n_in);
        const int rc = gsdr_resmap_feed_host(r, io, n_rows, io);
        if (identity) {
            if (rc != n_rows) ++bad;
            for (size_t i = 0; i < n_o; ++i)
                if (!same(io[i], whole[i])) ++bad;
        } else if (rc != -1 || std::memcmp(io, x, sizeof(gsdr_c64) * n_in) != 0) {
            ++bad;
        }
        std::free(io);
    }
    // offsets: exactly n_out x 2 doubles are read; back to zeros with NULL
    {
        double *xy = block<double>((size_t)n_out * 2);
        for (int c = 0; c < n_out; ++c) xy[2 * c] = (double)whole[c].x, xy[2 * c + 1] = (double)whole[c].y;
        gsdr_c64 *out = block<gsdr_c64>(n_o);
        if (gsdr_resmap_set_offsets(r, xy, nullptr) != 0 || gsdr_resmap_get_offsets(r, got_xy, n_out) != n_out ||
            std::memcmp(got_xy, xy, sizeof(double) * 2 * (size_t)n_out) != 0 || gsdr_resmap_feed_host(r, x, n_rows, out) != n_rows)
            ++bad;
        for (int c = 0; c < n_out; ++c)
            if (std::fabs(out[c].x) > 1e-6f * std::fabs(whole[c].x) || std::fabs(out[c].y) > 1e-6f * std::fabs(whole[c].y)) ++bad;
        xy[1] = std::numeric_limits<double>::infinity();
        if (gsdr_resmap_set_offsets(r, xy, nullptr) != -1) ++bad;
        if (gsdr_resmap_set_offsets(r, nullptr, nullptr) != 0 || gsdr_resmap_feed_host(r, x, n_rows, out) != n_rows) ++bad;
        for (size_t i = 0; i < n_o; ++i)
            if (!same(out[i], whole[i])) ++bad;
        std::free(xy), std::free(out);
    }
    // poison: an Inf, a NaN, a float32 denormal and 1e38 in input column got_ch[0], rows 0 and last; nothing else moves
    {
        gsdr_c64 *in = block<gsdr_c64>(n_in), *out = block<gsdr_c64>(n_o);
        std::memcpy(in, x, sizeof(gsdr_c64) * n_in);
        const int col = got_ch[0], last = n_rows - 1;
        in[(size_t)col].x = std::numeric_limits<float>::infinity();
        in[(size_t)last * n_ch + col].y = std::numeric_limits<float>::quiet_NaN();
        if (n_rows > 2) in[(size_t)n_ch + col].x = std::numeric_limits<float>::denorm_min(), in[(size_t)n_ch + col].y = 1e38f;
        if (gsdr_resmap_feed_host(r, in, n_rows, out) != n_rows) ++bad;
        for (int i = 0; i < n_rows; ++i)
            for (int c = 0; c < n_out; ++c) {
                const size_t o = (size_t)i * n_out + c;
                const bool touched = got_ch[c] == col && (i == 0 || i == last || (n_rows > 2 && i == 1));
                const bool poisoned = got_ch[c] == col && (i == 0 || i == last);
                if (poisoned && std::isfinite(out[o].x) && std::isfinite(out[o].y)) ++bad;
                if (!touched && !same(out[o], whole[o])) ++bad;
            }
        std::free(in), std::free(out);
    }
    // refusals leave everything as it was
    if (gsdr_resmap_feed_host(r, x, -1, whole) != -1 || gsdr_resmap_feed_host(r, x, n_rows + 1, whole) != -1 ||
        gsdr_resmap_feed_host(r, nullptr, 1, whole) != -1 || gsdr_resmap_feed_host(r, x, 1, nullptr) != -1)
        ++bad;
    std::free(x), std::free(whole), std::free(got_ch), std::free(got_k), std::free(got_xy);
    gsdr_resmap_close(r);
    return bad;
}

int main() {
    int bad = 0, runs = 0;
    const int rev[3] = {2, 1, 0}, sub[2] = {2, 0}, rep[5] = {63, 0, 7, 7, 31}, ident[4] = {0, 1, 2, 3}, one[1] = {6};
    for (int kind = GSDR_RESMAP_CAL; kind <= GSDR_RESMAP_X_QR; ++kind) {
        bad += run(1, 1, 1, nullptr, kind);
        bad += run(3, 7, 3, nullptr, kind);
        bad += run(3, 7, 3, rev, kind);
        bad += run(3, 5, 2, sub, kind);
        bad += run(64, 33, 5, rep, kind);
        bad += run(4, 130, 4, ident, kind);
        bad += run(7, 1, 1, one, kind);
        runs += 7;
    }
    // refusals leave a NULL and no allocation behind
    double k[GSDR_RESMAP_NCONST * 2];
    if (gsdr_resmap_constants(4e8, 400.0, 0.5, 0.1, 30.0, 2e4, 1e3, k) != 0 || gsdr_resmap_constants(4e8, 400.0, 0.5, 0.1, 30.0, 2e4, 1e3, k + GSDR_RESMAP_NCONST) != 0) ++bad;
    const int out_of_range[2] = {0, 2}, negative[2] = {-1, 0};
    if (gsdr_resmap_create(0, 4, 2, sub, k, 0, GSDR_RESMAP_HOST)) ++bad;
    if (gsdr_resmap_create(2, 0, 2, nullptr, k, 0, GSDR_RESMAP_HOST)) ++bad;
    if (gsdr_resmap_create(2, 4, 0, nullptr, k, 0, GSDR_RESMAP_HOST)) ++bad;
    if (gsdr_resmap_create(3, 4, 2, nullptr, k, 0, GSDR_RESMAP_HOST)) ++bad;
    if (gsdr_resmap_create(2, 4, 2, out_of_range, k, 0, GSDR_RESMAP_HOST)) ++bad;
    if (gsdr_resmap_create(2, 4, 2, negative, k, 0, GSDR_RESMAP_HOST)) ++bad;
    if (gsdr_resmap_create(2, 4, 2, nullptr, nullptr, 0, GSDR_RESMAP_HOST)) ++bad;
    if (gsdr_resmap_create(2, 4, 2, nullptr, k, 3, GSDR_RESMAP_HOST)) ++bad;
    if (gsdr_resmap_create(2, 4, 2, nullptr, k, 0, -3)) ++bad;
    if (gsdr_resmap_create(2, 4, 2, nullptr, k, 0, 0)) ++bad;             // no device part in this build
    k[3] = std::numeric_limits<double>::quiet_NaN();
    if (gsdr_resmap_create(2, 4, 2, nullptr, k, 0, GSDR_RESMAP_HOST)) ++bad;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (gsdr_resmap_constants(nan, 400.0, 0.5, 0.1, 30.0, 2e4, 1e3, k) != -1 || gsdr_resmap_constants(4e8, 0.0, 0.5, 0.1, 30.0, 2e4, 1e3, k) != -1 ||
        gsdr_resmap_constants(4e8, 400.0, 0.0, 0.1, 30.0, 2e4, 1e3, k) != -1 || gsdr_resmap_constants(4e8, 400.0, 0.5, 0.1, 30.0, 0.0, 0.0, k) != -1 ||
        gsdr_resmap_constants(4e8, 400.0, 0.5, 0.1, 30.0, 2e4, 1e3, nullptr) != -1)
        ++bad;
    gsdr_resmap_close(nullptr);
    gsdr_c64 m[1];
    if (gsdr_resmap_feed_host(nullptr, m, 1, m) != -1 || gsdr_resmap_set_offsets(nullptr, nullptr, nullptr) != -1 || gsdr_resmap_n_out(nullptr) != 0 ||
        gsdr_resmap_kind(nullptr) != 0 || gsdr_resmap_get_constants(nullptr, k, 1) != 0 || gsdr_resmap_get_offsets(nullptr, k, 1) != 0 ||
        gsdr_resmap_get_channels(nullptr, nullptr, 0) != 0)
        ++bad;
    std::printf("runs %d bad %d\n", runs, bad);
    return bad ? 1 : 0;
}
'''


def test_resmap_host_under_asan_and_ubsan(tmp_path):
    run = build_and_run(DRIVER, tmp_path)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.strip() == "runs 21 bad 0", run.stdout
