"""The owners of gpu_sdr_amd/csrc/dev_owner.h (device buffer, stream, event) under AddressSanitizer +
UndefinedBehaviorSanitizer, without a GPU and without the HIP runtime: a stand-alone program with its own main includes
the real HIP header and the owner header, and defines hipMalloc, hipFree, hipMemset, hipMemcpy and the stream and event
create / destroy functions itself.  They work on host memory of exactly the size asked for (one byte too many zeroed or
copied is a report), count calls and live objects, and fail at the k-th call when told to.  In the style of
tests/test_sc16_tx_sanitizers.py; nothing is loaded into Python."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "dev_owner.h"

// ---- the stand-ins ---------------------------------------------------------------------------------------------
static std::set<void *> live;                 // what was created and not released yet: buffers, streams, events
static long n_malloc, n_free, n_memset, n_memcpy, n_create, n_destroy, n_calls, n_bad;
static long fail_at = 0;                      // > 0: the fail_at-th call from now on that can fail, fails
static size_t last_malloc, last_fill;         // bytes of the last hipMalloc / hipMemset or hipMemcpy

static bool failing() { return fail_at > 0 && --fail_at == 0; }
static hipError_t release(void *p, long &counter) {
    ++n_calls, ++counter;
    if (!live.erase(p)) ++n_bad;              // released twice, or never created
    else std::free(p);
    return hipSuccess;
}
template <typename H>
static hipError_t create(H *h) {
    ++n_calls;
    if (failing()) return hipErrorOutOfMemory;
    ++n_create;                               // (the successful ones: each is owed one destroy)
    *h = (H)std::malloc(1);
    live.insert((void *)*h);
    return hipSuccess;
}

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) {
    ++n_calls;
    last_malloc = bytes;
    if (failing()) return hipErrorOutOfMemory;
    ++n_malloc;                               // (the successful ones: each is owed one hipFree)
    *p = std::malloc(bytes);
    live.insert(*p);
    return hipSuccess;
}
hipError_t hipFree(void *p) { return release(p, n_free); }
hipError_t hipMemset(void *dst, int value, size_t bytes) {
    ++n_calls, ++n_memset;
    last_fill = bytes;
    if (failing()) return hipErrorInvalidValue;
    std::memset(dst, value, bytes);
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    ++n_calls, ++n_memcpy;
    last_fill = bytes;
    if (kind != hipMemcpyHostToDevice) ++n_bad;
    if (failing()) return hipErrorInvalidValue;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return create(s); }
hipError_t hipStreamDestroy(hipStream_t s) { return release((void *)s, n_destroy); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return create(e); }
hipError_t hipEventDestroy(hipEvent_t e) { return release((void *)e, n_destroy); }
}

// ---- the checks ------------------------------------------------------------------------------------------------
static int bad = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("line %d: %s\n", __LINE__, #cond);              \
            ++bad;                                                      \
        }                                                               \
    } while (0)

using gsdr::DevBuf;
using gsdr::Event;
using gsdr::Stream;
using Buf = DevBuf<double>;

// the three ways to fill a buffer, and how many calls that can fail each makes
static hipError_t fill(Buf &b, int how) {
    const std::vector<double> v{1.0, 2.0, 3.0};
    return how == 0 ? b.alloc(3) : how == 1 ? b.alloc_zeroed(3) : b.upload(v);
}
static const int steps[3] = {1, 2, 2};

int main() {
    {   // count 0 allocates one element; alloc_zeroed zeroes what was asked for, as the idiom it replaces did
        Buf a, z;
        CHECK(a.alloc(0) == hipSuccess && a && last_malloc == sizeof(double));
        CHECK(z.alloc_zeroed(0) == hipSuccess && z && last_malloc == sizeof(double) && last_fill == 0);
        CHECK(z.alloc_zeroed(5) == hipSuccess && last_malloc == 5 * sizeof(double) && last_fill == 5 * sizeof(double));
        for (int i = 0; i < 5; ++i) CHECK(z[i] == 0.0);
        CHECK(live.size() == 2);
    }
    CHECK(live.empty());
    {   // upload: the values arrive; an empty vector allocates one element and copies nothing
        Buf u;
        const long c0 = n_memcpy;
        CHECK(u.upload(std::vector<double>{4.0, 5.0}) == hipSuccess && u[0] == 4.0 && u[1] == 5.0 && n_memcpy == c0 + 1);
        CHECK(last_malloc == 2 * sizeof(double) && last_fill == 2 * sizeof(double));
        CHECK(u.upload(std::vector<double>()) == hipSuccess && u && last_malloc == sizeof(double) && n_memcpy == c0 + 1);
        CHECK(live.size() == 1);
    }
    CHECK(live.empty());
    // a failed alloc, alloc_zeroed (either step) or upload (either step) leaves the owner empty and nothing live --
    // into an empty owner and into one that held something
    for (int how = 0; how < 3; ++how)
        for (int step = 1; step <= steps[how]; ++step)
            for (int held = 0; held < 2; ++held) {
                Buf b;
                if (held) CHECK(b.alloc(7) == hipSuccess);
                fail_at = step;
                CHECK(fill(b, how) != hipSuccess);
                CHECK(fail_at == 0 && !b && live.empty());
                CHECK(fill(b, how) == hipSuccess && b && live.size() == 1);      // and it can be used again
            }
    CHECK(live.empty());
    {   // allocating into a non-empty owner frees once
        Buf b;
        CHECK(b.alloc(3) == hipSuccess);
        double *first = b;
        const long f0 = n_free;
        CHECK(b.alloc(4) == hipSuccess && n_free == f0 + 1 && !live.count(first) && live.size() == 1);
        b.reset();
        CHECK(!b && n_free == f0 + 2 && live.empty());
        b.reset();
        CHECK(n_free == f0 + 2);
    }
    {   // move construction and move assignment transfer, and free exactly once; self-move is harmless
        const long f0 = n_free;
        {
            Buf a;
            CHECK(a.alloc(3) == hipSuccess);
            double *p = a;
            Buf b(std::move(a));
            CHECK(!a && b == p && n_free == f0);
            Buf c;
            CHECK(c.alloc(2) == hipSuccess);
            c = std::move(b);                                   // frees what c held, takes p
            CHECK(!b && c == p && n_free == f0 + 1 && live.size() == 1);
            Buf &same = c;
            c = std::move(same);
            CHECK(c == p && n_free == f0 + 1 && live.size() == 1);
        }
        CHECK(n_free == f0 + 2 && live.empty());
        const long d0 = n_destroy;
        {
            Stream s;
            Event e, e2;
            CHECK(hipStreamCreateWithFlags(s.out(), 0) == hipSuccess && hipEventCreateWithFlags(e.out(), 0) == hipSuccess);
            hipStream_t rs = s;
            hipEvent_t re = e;
            Stream t(std::move(s));
            CHECK(!s && t == rs);
            e2 = std::move(e);
            CHECK(!e && e2 == re && n_destroy == d0);
            Event &same = e2;
            e2 = std::move(same);
            CHECK(e2 == re && n_destroy == d0);
            Event e3;
            CHECK(hipEventCreateWithFlags(e3.out(), 0) == hipSuccess);
            hipEvent_t r3 = e3;
            e3 = std::move(e2);                                 // destroys what e3 held, takes re
            CHECK(!e2 && e3 == re && n_destroy == d0 + 1 && !live.count((void *)r3));
            e2 = std::move(e3);
            CHECK(hipEventCreateWithFlags(e2.out(), 0) == hipSuccess && n_destroy == d0 + 2 && !live.count((void *)re));
            fail_at = 1;                                        // a failed creation leaves the owner empty
            CHECK(hipEventCreateWithFlags(e2.out(), 0) != hipSuccess && !e2 && n_destroy == d0 + 3);
        }
        CHECK(n_destroy == d0 + 4 && live.empty());
    }
    {   // destruction, move and reset() of empty owners make no call at all
        const long c0 = n_calls;
        {
            Buf a, b(std::move(a)), arr[4];
            Stream s, t(std::move(s));
            Event e, f(std::move(e));
            a = std::move(b);
            s = std::move(t);
            e = std::move(f);
            a.reset(), s.reset(), e.reset();
            arr[1] = std::move(arr[2]);
            std::vector<std::pair<Event, Event>> pool(3);
            pool.emplace_back(Event(), Event());
            CHECK(!a && !s && !e);
        }
        CHECK(n_calls == c0);
    }
    {   // an array of owners and a std::vector of event pairs (which moves them when it grows) end with nothing live
        {
            Buf arr[4];
            Stream st[3];
            for (auto &b : arr) CHECK(b.alloc_zeroed(9) == hipSuccess);
            for (auto &s : st) CHECK(hipStreamCreateWithFlags(s.out(), 0) == hipSuccess);
            std::vector<std::pair<Event, Event>> pool;
            for (int i = 0; i < 37; ++i) {
                Event a, b;
                CHECK(hipEventCreateWithFlags(a.out(), 0) == hipSuccess && hipEventCreateWithFlags(b.out(), 0) == hipSuccess);
                pool.emplace_back(std::move(a), std::move(b));
            }
            CHECK(live.size() == 4 + 3 + 2 * 37);
            for (auto &pr : pool) CHECK(live.count((void *)(hipEvent_t)pr.first) && live.count((void *)(hipEvent_t)pr.second));
            arr[0] = std::move(arr[3]);
            st[0].reset();
            CHECK(live.size() == 3 + 2 + 2 * 37);
        }
        CHECK(live.empty());
    }
    // the totals: everything that was created was released, once
    CHECK(n_bad == 0 && n_malloc == n_free && n_create == n_destroy);
    std::printf("malloc %ld free %ld create %ld destroy %ld live %zu bad %d\n", n_malloc, n_free, n_create, n_destroy,
                live.size(), bad);
    return bad ? 1 : 0;
}
'''


def rocm_include():
    for d in [os.environ.get("ROCM_PATH"), "/opt/rocm"] + sorted(glob.glob("/opt/rocm-*"), reverse=True):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime.h")):
            return os.path.join(d, "include")
    return None


def test_owners_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    inc = rocm_include()
    if not inc:
        pytest.skip("no ROCm headers")
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = tmp_path / "driver"
    build = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", inc,
                            "-I", os.path.join(ROOT, "gpu_sdr_amd", "csrc"), str(tmp_path / "driver.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    words = run.stdout.split()
    counts = {k: int(words[words.index(k) + 1]) for k in ("malloc", "free", "create", "destroy", "live", "bad")}
    assert counts["live"] == 0 and counts["bad"] == 0, run.stdout
    assert counts["malloc"] == counts["free"] and counts["create"] == counts["destroy"], run.stdout
    assert counts["malloc"] > 0 and counts["create"] > 0, run.stdout     # (the program did run its cases)
