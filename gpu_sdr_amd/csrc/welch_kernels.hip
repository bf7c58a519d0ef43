// welch_kernels.hip -- Welch spectra from demodulated rows (the contract: include/gsdr.h, "Welch spectra on the
// device"; the design: DESIGN.md section 4.10).  Three launches per feed:
//   welch_append_kernel      transposes the feed's [row][channel] rows through the LDS into the channel-major history
//                            ring, so that a segment is one contiguous run (two at the ring's seam);
//   welch_segment_kernel     one (channel, segment) per workgroup -- several short segments per workgroup below 1024
//                            points: loads N samples, reduces the detrend sums in double, subtracts in double, rounds,
//                            windows, runs the radix stages of fft_lds.h between two LDS buffers and leaves |X|^2, |Y|^2
//                            and Re X conj Y of the bins k <= N/2 in this feed's staging;
//   welch_accumulate_kernel  adds the staged segments into the double accumulators, one thread per bin, in segment order.
// A segment's arithmetic is the same whichever feed completes it and whichever slot of a workgroup it gets, and the
// sums over segments run in segment order: the accumulators do not depend on the cutting, bit for bit.
// welch_read_kernel turns the accumulators into densities.  All compiler-scheduled and GSDR_NO_PK: they run beside
// another handle's matrix-core loop.
#include "welch_kernels.h"

#include <atomic>

#include "ddc_kernels.h"
#include "fft_lds.h"

namespace gsdr {
namespace {

// (the HIP headers' __syncthreads and __shfl_xor are not always_inline: inside a GSDR_NO_PK kernel they would stay
//  real calls; the builtins they wrap are used directly, as in trigger_kernels.hip)
__device__ __forceinline__ void wg_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the value lane ^ off holds (every lane of the wave is active where this is used)
__device__ __forceinline__ double shfl_xor_d(double v, int lane, int off) {
    const int addr = (lane ^ off) << 2;
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)(unsigned)b);
    const unsigned hi = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)(unsigned)(b >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// ---- append ---------------------------------------------------------------------------------------------------------
// A tile is 1024 samples: TC = 1 << ltc channels (the smallest power of two that holds min(n_ch, 32)) by TR = 1024 / TC
// rows, so that a feed of few channels still reads and writes whole lines.  Read along the channels, written along the
// rows; the LDS rows are padded by one sample.
__global__ __launch_bounds__(256) GSDR_NO_PK void welch_append_kernel(const float2 *__restrict__ rows, int n, int n_ch, int ltc,
                                                                      float2 *__restrict__ hist, unsigned H, unsigned row_pos,
                                                                      unsigned tiles_c) {
    __shared__ float2 tile[1056];
    const int tid = (int)threadIdx.x;
    const int TC = 1 << ltc, TR = 1024 >> ltc, pitch = TR + 1;
    const unsigned br = blockIdx.x / tiles_c, bc = blockIdx.x - br * tiles_c;
    const int c0 = (int)bc * TC, i0 = (int)br * TR;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = tid + 256 * j;
        const int tc = e & (TC - 1), tr = e >> ltc;
        const int i = i0 + tr, c = c0 + tc;
        if (i < n && c < n_ch) tile[tc * pitch + tr] = rows[(size_t)i * (size_t)n_ch + (size_t)c];
    }
    wg_sync();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = tid + 256 * j;
        const int tr = e & (TR - 1), tc = e >> (10 - ltc);
        const int i = i0 + tr, c = c0 + tc;
        if (i < n && c < n_ch) {
            unsigned pos = row_pos + (unsigned)i;                 // row_pos < H, i < max_rows < H
            pos = pos >= H ? pos - H : pos;
            hist[(size_t)c * H + pos] = tile[tc * pitch + tr];
        }
    }
}

// ---- segments -------------------------------------------------------------------------------------------------------
struct WelchSeg {
    const float2 *hist;
    unsigned H, seg_pos, n_items;        // items: (channel, segment) pairs, the segment running fastest
    int n_ch, n_segs, step, detrend;
    const float *window;
    const float2 *tw;
    float *stage;
    double *stage_mean;
};

// N points: NT threads take G segments of N points each, TPS threads and E samples per thread and segment
template <int N>
struct WelchShape {
    static constexpr int NT = N >= 2048 ? 1024 : 256;
    static constexpr int G = N >= 1024 ? 1 : 1024 / N;
    static constexpr int PTS = G * N;
    static constexpr int E = PTS / NT;
    static constexpr int TPS = NT / G;
    static constexpr size_t lds = (size_t)2 * PTS * sizeof(float2) + 16 * 6 * sizeof(double);
};

constexpr unsigned welch_magic(int d) { return d <= 1 ? 0u : (unsigned)(0x100000000ULL / (unsigned long long)d + 1ULL); }

// the radix of the stage behind P points: 16s first, then what is left (8, 4 or 2)
constexpr int welch_radix(int N, int P) { return (N / P) % 16 == 0 ? 16 : N / P; }
constexpr bool welch_result_in_b(int N) {
    bool flip = false;
    for (int P = 1; P < N; P *= welch_radix(N, P)) flip = !flip;
    return flip;
}

// the stages are unrolled at compile time: source and destination are fixed offsets from one LDS base in every stage
// (a pointer pair swapped at run time reads through the flat aperture)
template <int N, int G, int NT, int P, bool FLIP>
__device__ __forceinline__ void welch_stages(float2 *lds, const float2 *__restrict__ tw, int tid) {
    if constexpr (P < N) {
        constexpr int R = welch_radix(N, P), t = N / R, tws = N / (P * R);
        lds_stage<R>(lds + (FLIP ? G * N : 0), lds + (FLIP ? 0 : G * N), N, P, t, tws, welch_magic(t), welch_magic(P), tw, G, tid, NT);
        wg_sync();
        welch_stages<N, G, NT, P * R, !FLIP>(lds, tw, tid);
    }
}

template <int N>
__global__ __launch_bounds__(WelchShape<N>::NT) GSDR_NO_PK void welch_segment_kernel(const WelchSeg a) {
    using S = WelchShape<N>;
    constexpr int NT = S::NT, G = S::G, E = S::E, TPS = S::TPS, K1 = N / 2 + 1;
    extern __shared__ float2 welch_lds[];
    double *part = reinterpret_cast<double *>(welch_lds + 2 * S::PTS);       // [wave][6]
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int g = tid / TPS, l = tid - g * TPS;
    const unsigned item = blockIdx.x * (unsigned)G + (unsigned)g;
    const bool live = item < a.n_items;
    const unsigned c = live ? item / (unsigned)a.n_segs : 0u, sl = live ? item - c * (unsigned)a.n_segs : 0u;
    const unsigned p0 = (a.seg_pos + sl * (unsigned)a.step) % a.H;           // sl * step <= max_rows
    const float2 *h = a.hist + (size_t)c * a.H;
    constexpr double mid = 0.5 * (double)(N - 1);
    float2 x[E];
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int j = l + TPS * e;
        unsigned pos = p0 + (unsigned)j;                                     // p0 < H, j < N <= H
        pos = pos >= a.H ? pos - a.H : pos;
        x[e] = live ? h[pos] : mk2(0.f, 0.f);
        const double t = (double)j - mid, xr = (double)x[e].x, xi = (double)x[e].y;
        s[0] += xr;
        s[1] += xi;
        s[2] += xr * t;
        s[3] += xi * t;
        s[4] += j < a.step ? xr : 0.0;
        s[5] += j < a.step ? xi : 0.0;
    }
    // every thread of a segment ends with the same six sums: an xor tree inside the wave (a + b == b + a, so both sides
    // of an exchange hold the same bits), then the waves of the segment in ascending order
#pragma unroll
    for (int off = 1; off < (TPS < 64 ? TPS : 64); off <<= 1) {
#pragma unroll
        for (int q = 0; q < 6; ++q) s[q] += shfl_xor_d(s[q], lane, off);
    }
    if constexpr (TPS > 64) {
        constexpr int WPS = TPS / 64;
        const int wave = tid >> 6;
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 6; ++q) part[wave * 6 + q] = s[q];
        }
        wg_sync();
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            double v = part[(g * WPS) * 6 + q];
            for (int w = 1; w < WPS; ++w) v += part[(g * WPS + w) * 6 + q];
            s[q] = v;
        }
    }
    // detrend in double, one rounding; window in float
    constexpr double inv_n = 1.0 / (double)N, inv_tt = 12.0 / ((double)N * ((double)N * (double)N - 1.0));
    const bool lin = a.detrend == GSDR_WELCH_DETREND_LINEAR, raw = a.detrend == GSDR_WELCH_DETREND_NONE;
    const double mr = s[0] * inv_n, mi = s[1] * inv_n;
    const double br = lin ? s[2] * inv_tt : 0.0, bi = lin ? s[3] * inv_tt : 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int j = l + TPS * e;
        const double t = (double)j - mid;
        const float w = a.window[j];
        const float dr = raw ? x[e].x : (float)((double)x[e].x - (mr + br * t));
        const float di = raw ? x[e].y : (float)((double)x[e].y - (mi + bi * t));
        welch_lds[g * N + j] = mk2(dr * w, di * w);
    }
    wg_sync();
    welch_stages<N, G, NT, 1, false>(welch_lds, a.tw, tid);
    const float2 *Z = welch_lds + (welch_result_in_b(N) ? G * N : 0);
    for (int idx = tid; idx < G * K1; idx += NT) {
        const int gg = idx / K1, k = idx - gg * K1;
        const unsigned it = blockIdx.x * (unsigned)G + (unsigned)gg;
        if (it >= a.n_items) continue;
        const unsigned cc = it / (unsigned)a.n_segs, ss = it - cc * (unsigned)a.n_segs;
        const float2 z = Z[gg * N + k], u = Z[gg * N + ((N - k) & (N - 1))];
        // Zm = conj u:  X = (z + Zm) / 2,  Y = (z - Zm) / (2i)
        const double Xr = 0.5 * ((double)z.x + (double)u.x), Xi = 0.5 * ((double)z.y - (double)u.y);
        const double Yr = 0.5 * ((double)z.y + (double)u.y), Yi = -0.5 * ((double)z.x - (double)u.x);
        float *o = a.stage + ((size_t)ss * (size_t)a.n_ch + cc) * (size_t)(3 * K1);
        o[k] = (float)(Xr * Xr + Xi * Xi);
        o[K1 + k] = (float)(Yr * Yr + Yi * Yi);
        o[2 * K1 + k] = (float)(Xr * Yr + Xi * Yi);
    }
    if (live && l == 0) {
        double *o = a.stage_mean + ((size_t)sl * (size_t)a.n_ch + c) * 2;
        o[0] = s[4];
        o[1] = s[5];
    }
}

// ---- accumulate -----------------------------------------------------------------------------------------------------
// thread g < per: bin g of the accumulators; per <= g < per + per_mean: a component of the mean sums
__global__ __launch_bounds__(256) GSDR_NO_PK void welch_accumulate_kernel(const float *__restrict__ stage, const double *__restrict__ stage_mean,
                                                                          int n_segs, long long per, long long per_mean,
                                                                          double *__restrict__ acc, double *__restrict__ msum) {
    const long long g = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    if (g < per) {
        // the additions are a chain, in segment order by contract; what a thread can overlap is the loads: 32 in flight
        // (with 8 a feed of hundreds of segments on a few channels waited a memory round trip per 8 segments)
        double v = acc[g];
        int s = 0;
        for (; s + 32 <= n_segs; s += 32) {
            float t[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) t[u] = stage[(size_t)(s + u) * (size_t)per + (size_t)g];
#pragma unroll
            for (int u = 0; u < 32; ++u) v += (double)t[u];
        }
        for (; s < n_segs; ++s) v += (double)stage[(size_t)s * (size_t)per + (size_t)g];
        acc[g] = v;
    } else if (g - per < per_mean) {
        const long long m = g - per;
        double v = msum[m];
#pragma unroll 8
        for (int s = 0; s < n_segs; ++s) v += stage_mean[(size_t)s * (size_t)per_mean + (size_t)m];
        msum[m] = v;
    }
}

// ---- read -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) GSDR_NO_PK void welch_read_kernel(const WelchRead r, long long total) {
    const long long g = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    if (g >= total) return;
    const int N = r.nperseg, K1 = N / 2 + 1;
    const long long c = g / K1;
    const int k = (int)(g - c * K1);
    const double mr = r.msum[2 * c] / r.rows_in, mi = r.msum[2 * c + 1] / r.rows_in;
    if (r.mean && k == 0) r.mean[c] = mk2((float)mr, (float)mi);
    if (!r.psd) return;
    double gr = 1.0, gi = 0.0;
    const double m2 = mr * mr + mi * mi;
    if (r.mode == GSDR_WELCH_GAIN) {
        const float2 gn = r.gain[c];
        gr = (double)gn.x, gi = (double)gn.y;
    } else if (r.mode != GSDR_WELCH_RAW && m2 > 0.0 && m2 < __builtin_inf()) {
        const double d = r.mode == GSDR_WELCH_ROTATE ? __builtin_sqrt(m2) : m2;      // |m| / m = conj m / |m|, 1 / m = conj m / |m|^2
        gr = mr / d, gi = -mi / d;
    }
    const double *acc = r.acc + (size_t)c * (size_t)(3 * K1);
    const double a0 = acc[k], a1 = acc[K1 + k], a2 = acc[2 * K1 + k];
    const double f = (k > 0 && k < N / 2) ? 2.0 : 1.0;
    float *out = r.psd + (size_t)c * (size_t)(2 * K1);
    out[k] = (float)((gr * gr * a0 + gi * gi * a1 - 2.0 * gr * gi * a2) * f * r.scale);
    out[K1 + k] = (float)((gi * gi * a0 + gr * gr * a1 + 2.0 * gr * gi * a2) * f * r.scale);
}

template <int N>
hipError_t launch_segments(const WelchSeg &a, hipStream_t st) {
    using S = WelchShape<N>;
    const void *fn = reinterpret_cast<const void *>(welch_segment_kernel<N>);
    if (S::lds > 64 * 1024) {
        // (a function attribute belongs to the device it was set on: once per device of this process)
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return hipErrorInvalidDevice;
        static std::atomic<unsigned long long> done{0};
        if (!(done.load() >> dev & 1ULL)) {
            const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)S::lds);
            if (e != hipSuccess) return e;
            done.fetch_or(1ULL << dev);
        }
    }
    const unsigned blocks = (a.n_items + (unsigned)S::G - 1u) / (unsigned)S::G;
    WelchSeg arg = a;
    void *kargs[] = {&arg};
    return hipLaunchKernel(fn, dim3(blocks), dim3(S::NT), kargs, S::lds, st);
}

}  // namespace

hipError_t launch_welch_feed(const WelchFeed &f, hipStream_t st) {
    const int N = f.nperseg, K1 = N / 2 + 1;
    if (f.n < 1 || f.n_ch < 1 || f.n_segs < 0 || !f.rows || !f.hist || f.H < (unsigned)N || (unsigned)f.n > f.H - (unsigned)(N - 1) ||
        f.row_pos >= f.H || f.seg_pos >= f.H || f.step < 1 || f.step > N || ((long long)f.n_segs - 1) * f.step >= (long long)f.n ||      // the last segment starts at most n - 1 rows behind the first
        (long long)f.n_segs * f.n_ch > 0x7fffffffLL)
        return hipErrorInvalidValue;
    int ltc = 0;
    while ((1 << ltc) < f.n_ch && ltc < 5) ++ltc;
    const long long tiles_c = ((long long)f.n_ch + (1 << ltc) - 1) >> ltc, tiles_r = ((long long)f.n + (1024 >> ltc) - 1) / (1024 >> ltc);
    if (tiles_c * tiles_r > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(welch_append_kernel, dim3((unsigned)(tiles_c * tiles_r)), dim3(256), 0, st, f.rows, f.n, f.n_ch, ltc, f.hist, f.H,
                       f.row_pos, (unsigned)tiles_c);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || f.n_segs == 0) return e;
    if (!f.window || !f.tw || !f.stage || !f.stage_mean || !f.acc || !f.msum) return hipErrorInvalidValue;
    WelchSeg a{};
    a.hist = f.hist, a.H = f.H, a.seg_pos = f.seg_pos, a.n_items = (unsigned)((long long)f.n_segs * f.n_ch);
    a.n_ch = f.n_ch, a.n_segs = f.n_segs, a.step = f.step, a.detrend = f.detrend;
    a.window = f.window, a.tw = f.tw, a.stage = f.stage, a.stage_mean = f.stage_mean;
    switch (N) {
        case 16: e = launch_segments<16>(a, st); break;
        case 32: e = launch_segments<32>(a, st); break;
        case 64: e = launch_segments<64>(a, st); break;
        case 128: e = launch_segments<128>(a, st); break;
        case 256: e = launch_segments<256>(a, st); break;
        case 512: e = launch_segments<512>(a, st); break;
        case 1024: e = launch_segments<1024>(a, st); break;
        case 2048: e = launch_segments<2048>(a, st); break;
        case 4096: e = launch_segments<4096>(a, st); break;
        case 8192: e = launch_segments<8192>(a, st); break;
        default: return hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    const long long per = (long long)f.n_ch * 3 * K1, per_mean = (long long)f.n_ch * 2;
    const long long blocks = (per + per_mean + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(welch_accumulate_kernel, dim3((unsigned)blocks), dim3(256), 0, st, f.stage, f.stage_mean, f.n_segs, per, per_mean,
                       f.acc, f.msum);
    return hipGetLastError();
}

hipError_t launch_welch_read(const WelchRead &r, hipStream_t st) {
    if (r.n_ch < 1 || r.nperseg < 2 || !r.acc || !r.msum || (!r.psd && !r.mean) || (r.psd && r.mode == GSDR_WELCH_GAIN && !r.gain))
        return hipErrorInvalidValue;
    const long long total = (long long)r.n_ch * (r.nperseg / 2 + 1), blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(welch_read_kernel, dim3((unsigned)blocks), dim3(256), 0, st, r, total);
    return hipGetLastError();
}

}  // namespace gsdr
