"""gsdr_narrow_sc16_host under AddressSanitizer + UndefinedBehaviorSanitizer with float-cast-overflow: converting a
NaN or an out-of-range float to an integer is undefined behaviour, so the host code has to test before it converts.
A stand-alone program with its own main (CPU build; nothing is loaded into Python), in the style of the driver of
tests/test_sanitizers.py."""
from _sanitized import build_and_run

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "gsdr.h"

// the contract of include/gsdr.h, written independently (double arithmetic on the float32 product)
static int model(float c, float gain, long long *clipped) {
    volatile float v = c * gain;
    if (v != v) { ++*clipped; return 0; }
    const double r = std::nearbyint((double)v);
    if (r > 32767.0) { ++*clipped; return 32767; }
    if (r < -32768.0) { ++*clipped; return -32768; }
    return (int)r;
}

static int check(const std::vector<float> &vals, float gain) {
    // heap buffers of exactly n samples: one byte too many read or written is a report
    const long long n = (long long)vals.size();
    gsdr_c64 *in = (gsdr_c64 *)std::malloc((size_t)n * sizeof(gsdr_c64));
    gsdr_sc16 *out = (gsdr_sc16 *)std::malloc((size_t)n * sizeof(gsdr_sc16));
    for (long long k = 0; k < n; ++k) {
        in[k].x = vals[(size_t)k];
        in[k].y = vals[(size_t)(n - 1 - k)];         // every value in the I and in the Q position
    }
    const long long got = gsdr_narrow_sc16_host(in, out, n, gain);
    long long want = 0;
    int bad = 0;
    for (long long k = 0; k < n; ++k) {
        const int i = model(in[k].x, gain, &want), q = model(in[k].y, gain, &want);
        if (out[k].i != i || out[k].q != q) ++bad;
    }
    if (got != want) ++bad;
    std::free(in);
    std::free(out);
    return bad;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> v;
    for (int k = -32768; k <= 32767; ++k)
        for (float d : {0.f, -0.75f, -0.5f, -0.25f, 0.25f, 0.5f, 0.75f}) v.push_back((float)k + d);
    for (float s : {0.f, -0.f, 1e-45f, -1e-45f, 1e-39f, -1e-39f, 1e10f, -1e10f, inf, -inf, nan, -nan, 3e38f, -3e38f,
                    2147483648.f, -2147483648.f, 4294967296.f})
        v.push_back(s);
    int bad = check(v, 1.0f);
    bad += check(v, 32767.0f);                        // products that overflow to Inf
    bad += check(v, 1.0f / 3.0f);
    for (long long n : {1, 2, 3, 5}) bad += check(std::vector<float>(v.end() - n, v.end()), 1.0f);
    // n == 0 touches nothing, not even the pointers
    if (gsdr_narrow_sc16_host(nullptr, nullptr, 0, 1.0f) != 0) ++bad;
    std::printf("values %zu bad %d\n", v.size(), bad);
    return bad ? 1 : 0;
}
'''


def test_narrow_host_under_asan_and_ubsan(tmp_path):
    run = build_and_run(DRIVER, tmp_path)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.startswith("values ") and run.stdout.split()[3] == "0", run.stdout
