// sweep_kernels.hip -- the VNA sweep accumulator on demodulated rows (the contract: include/gsdr.h, "VNA sweep
// accumulator on the device"; the fold: sweep_state.h; the design: DESIGN.md section 4.12).
//   sweep_accumulate_kernel     one launch per feed, one thread per (touched point, channel), the channel running
//                               fastest across the lanes.  The thread is the only owner of its accumulator in the
//                               launch: it loads the four doubles, walks its rows of the feed in stream order -- the
//                               rest of a group an earlier feed began, whole groups, the start of one the feed leaves
//                               open, and the same again one pass later where the feed is longer than a pass -- and
//                               stores them.  No atomics, and a chain of additions does not see where the stream was
//                               cut.  With group == 1 consecutive lanes hold consecutive (row, channel): the row loads
//                               and the 32-byte read-modify-writes of a wave are contiguous.  With group > 1 a lane
//                               walks `group` rows n_ch samples apart; kSweepDepth of them are in flight.
//   sweep_read_kernel           one thread per (point, channel): n[p] by the closed form, the mean and the variance.
//   sweep_slope_block_kernel    one thread per (block of 256 terms, channel): the terms in ascending p from +0.  The
//                               float32 means are recomputed from the sums, so the slope needs no read before it.
//   sweep_slope_combine_kernel  one thread per channel: the block sums in ascending order, from block 0's.
// The 64-bit arithmetic of the fold is done once per thread (sweep_state.h, and the launcher for what is uniform).
// Compiler-scheduled and GSDR_NO_PK: they run beside another handle's matrix-core loop.
//
// Contraction is off for the whole file: hipcc contracts by default and the host twin must see the same roundings.  The
// two fused operations of the contract are written out (__fma_rn); x*x of a float32 and the products of two float32 are
// exact in double, so the sums of squares and the slope's terms round once however they are written.
#pragma clang fp contract(off)
#include "sweep_kernels.h"

#include "ddc_kernels.h"

namespace gsdr {
namespace {

constexpr int kSweepDepth = 8;           // rows a thread of sweep_accumulate_kernel has in flight

__device__ __forceinline__ float2 f2(float x, float y) {
    float2 v;
    v.x = x, v.y = y;
    return v;
}

struct SweepAcc {
    const float2 *rows;
    double *acc;
    unsigned long long items;            // touched points x n_ch
    int n, n_ch;
    unsigned n_points, p0;               // p0: point of slot 0
    long long group, pass;               // pass = n_points * group
    long long rel0;                      // feed row on which slot 0's first group begins, in (-group, 0]
};

__device__ __forceinline__ void sweep_add(double &sx, double &sy, double &qx, double &qy, float2 v) {
    const double x = (double)v.x, y = (double)v.y;
    const double xx = x * x, yy = y * y;              // exact: 48 bits
    sx = sx + x, sy = sy + y;
    qx = qx + xx, qy = qy + yy;
}

__global__ __launch_bounds__(256) GSDR_NO_PK void sweep_accumulate_kernel(const SweepAcc a) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256ULL + (unsigned long long)threadIdx.x;
    if (g >= a.items) return;
    const unsigned t = (unsigned)(g / (unsigned)a.n_ch);          // slot: < n_points <= 2^24
    const unsigned c = (unsigned)(g - (unsigned long long)t * (unsigned)a.n_ch);
    unsigned p = a.p0 + t;                                          // < 2^25
    p = p >= a.n_points ? p - a.n_points : p;
    double *s = a.acc + ((size_t)p * (size_t)a.n_ch + c) * 4;
    double sx = s[0], sy = s[1], qx = s[2], qy = s[3];
    const float2 *x = a.rows + c;
    const size_t step = (size_t)a.n_ch;
    // the groups of this slot: they begin on feed rows rel, rel + pass, ... while that is inside the feed
    for (long long rel = a.rel0 + (long long)t * a.group; rel < (long long)a.n; rel += a.pass) {
        const long long end = rel + a.group;
        const int lo = rel < 0 ? 0 : (int)rel, hi = end < (long long)a.n ? (int)end : a.n;
        int i = lo;
        for (; i + kSweepDepth <= hi; i += kSweepDepth) {
            float2 v[kSweepDepth];
#pragma unroll
            for (int u = 0; u < kSweepDepth; ++u) v[u] = x[(size_t)(i + u) * step];
#pragma unroll
            for (int u = 0; u < kSweepDepth; ++u) sweep_add(sx, sy, qx, qy, v[u]);
        }
        for (; i < hi; ++i) sweep_add(sx, sy, qx, qy, x[(size_t)i * step]);
    }
    s[0] = sx, s[1] = sy, s[2] = qx, s[3] = qy;
}

// mean of one component: one double division, one rounding to float
__device__ __forceinline__ float sweep_mean(double s, double n) { return (float)(s / n); }

// variance of one component, n >= 2
__device__ __forceinline__ float sweep_var(double s, double q, double n) {
    const double v = __fma_rn(-s, s / n, q) / (n - 1.0);
    return (float)(v < 0.0 ? 0.0 : v);                             // a NaN is not < 0: it stays
}

struct SweepReadArgs {
    SweepRead r;
    float2 *mean, *var;
    unsigned long long items;            // n_points x n_ch
};

__global__ __launch_bounds__(256) GSDR_NO_PK void sweep_read_kernel(const SweepReadArgs a) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256ULL + (unsigned long long)threadIdx.x;
    if (g >= a.items) return;
    const unsigned p = (unsigned)(g / (unsigned)a.r.n_ch);
    const long long cnt = gsdr_sweep_rows_of(a.r.a, a.r.b, (long long)p, a.r.group);
    float2 m = f2(0.f, 0.f), v = f2(0.f, 0.f);
    if (cnt > 0) {
        const double *s = a.r.acc + (size_t)g * 4;
        const double n = (double)cnt, sx = s[0], sy = s[1];
        m = f2(sweep_mean(sx, n), sweep_mean(sy, n));
        if (a.var && cnt > 1) v = f2(sweep_var(sx, s[2], n), sweep_var(sy, s[3], n));
    }
    a.mean[g] = m;
    if (a.var) a.var[g] = v;
}

// the float32 mean of (p, c) as a read returns it
__device__ __forceinline__ float2 sweep_mean_of(const SweepRead &r, long long p, unsigned c) {
    const long long cnt = gsdr_sweep_rows_of(r.a, r.b, p, r.group);
    if (cnt <= 0) return f2(0.f, 0.f);
    const double *s = r.acc + ((size_t)p * (size_t)r.n_ch + c) * 4;
    const double n = (double)cnt;
    return f2(sweep_mean(s[0], n), sweep_mean(s[1], n));
}

struct SweepSlope {
    SweepRead r;
    double2 *blocks;                     // [n_blocks][n_ch]
    double2 *d;                          // [n_ch]
    unsigned long long items;            // n_blocks x n_ch
    long long n_blocks;
};

__global__ __launch_bounds__(256) GSDR_NO_PK void sweep_slope_block_kernel(const SweepSlope a) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256ULL + (unsigned long long)threadIdx.x;
    if (g >= a.items) return;
    const unsigned b = (unsigned)(g / (unsigned)a.r.n_ch);
    const unsigned c = (unsigned)(g - (unsigned long long)b * (unsigned)a.r.n_ch);
    const long long first = (long long)b * kSweepSlopeBlock;      // terms [first, last): term p is m[p+1] conj(m[p])
    const long long terms = a.r.n_points - 1;
    const long long last = first + kSweepSlopeBlock < terms ? first + kSweepSlopeBlock : terms;
    double dx = 0.0, dy = 0.0;
    if (first < last) {
        float2 m0 = sweep_mean_of(a.r, first, c);
        for (long long p = first; p < last; ++p) {
            const float2 m1 = sweep_mean_of(a.r, p + 1, c);
            const double ar = (double)m1.x, ai = (double)m1.y, br = (double)m0.x, bi = (double)m0.y;
            const double rr = ar * br, ii = ai * bi, ir = ai * br, ri = ar * bi;      // exact
            const double tx = rr + ii, ty = ir - ri;
            dx = dx + tx, dy = dy + ty;
            m0 = m1;
        }
    }
    double2 out;
    out.x = dx, out.y = dy;
    a.blocks[g] = out;
}

__global__ __launch_bounds__(256) GSDR_NO_PK void sweep_slope_combine_kernel(const SweepSlope a) {
    const unsigned c = blockIdx.x * 256u + threadIdx.x;
    if (c >= (unsigned)a.r.n_ch) return;
    const size_t step = (size_t)a.r.n_ch;
    const double2 *b = a.blocks + c;
    double2 s = b[0];
    long long k = 1;
    for (; k + 8 <= a.n_blocks; k += 8) {                          // the additions are a chain, the loads are not
        double2 t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = b[(size_t)(k + u) * step];
#pragma unroll
        for (int u = 0; u < 8; ++u) s.x = s.x + t[u].x, s.y = s.y + t[u].y;
    }
    for (; k < a.n_blocks; ++k) {
        const double2 t = b[(size_t)k * step];
        s.x = s.x + t.x, s.y = s.y + t.y;
    }
    a.d[c] = s;
}

bool read_ok(const SweepRead &r) {
    return r.acc && r.n_ch >= 1 && r.n_points >= 1 && r.group >= 1 && r.n_points * (long long)r.n_ch <= (1LL << 25);
}

unsigned blocks_of(unsigned long long items) { return (unsigned)((items + 255ULL) / 256ULL); }

}  // namespace

hipError_t launch_sweep_feed(const SweepFeed &f, hipStream_t st) {
    if (f.n < 1 || f.n > (1 << 24) || f.n_ch < 1 || f.n_points < 1 || f.n_points > (1LL << 24) || f.group < 1 || f.group > (1LL << 30) ||
        f.n_points * (long long)f.n_ch > (1LL << 25) || !f.rows || !f.acc || f.row0 < 0)
        return hipErrorInvalidValue;
    const gsdr_sweep_span sp = gsdr_sweep_span_of(f.row0, f.n, f.n_points, f.group);
    if (sp.touched < 1 || sp.touched > f.n_points || sp.p0 < 0 || sp.p0 >= f.n_points || sp.rel0 > 0 || sp.rel0 <= -f.group)
        return hipErrorInvalidValue;
    SweepAcc a{};
    a.rows = f.rows, a.acc = f.acc;
    a.items = (unsigned long long)sp.touched * (unsigned long long)f.n_ch;          // <= 2^25
    a.n = f.n, a.n_ch = f.n_ch;
    a.n_points = (unsigned)f.n_points, a.p0 = (unsigned)sp.p0;
    a.group = f.group, a.pass = f.n_points * f.group;
    a.rel0 = sp.rel0;
    hipLaunchKernelGGL(sweep_accumulate_kernel, dim3(blocks_of(a.items)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_sweep_read(const SweepRead &r, float2 *mean, float2 *var, hipStream_t st) {
    if (!read_ok(r) || !mean) return hipErrorInvalidValue;
    SweepReadArgs a{};
    a.r = r, a.mean = mean, a.var = var;
    a.items = (unsigned long long)r.n_points * (unsigned long long)r.n_ch;
    hipLaunchKernelGGL(sweep_read_kernel, dim3(blocks_of(a.items)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_sweep_slope(const SweepRead &r, double2 *blocks, double2 *d, hipStream_t st) {
    if (!read_ok(r) || !blocks || !d) return hipErrorInvalidValue;
    SweepSlope a{};
    a.r = r, a.blocks = blocks, a.d = d;
    a.n_blocks = gsdr_sweep_slope_blocks(r.n_points);
    a.items = (unsigned long long)a.n_blocks * (unsigned long long)r.n_ch;
    hipLaunchKernelGGL(sweep_slope_block_kernel, dim3(blocks_of(a.items)), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sweep_slope_combine_kernel, dim3(blocks_of((unsigned long long)r.n_ch)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace gsdr
