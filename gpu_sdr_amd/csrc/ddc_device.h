// ddc_device.h -- small device helpers shared by the DDC kernels (internal).
#pragma once
#include <hip/hip_runtime.h>

#include "ddc_kernels.h"

namespace gsdr {

// First block of chunk c when nblk blocks are split into nch chunks whose
// lengths differ by at most one (the first `crem` chunks are one block longer).
// No division: cbase = nblk / nch and crem = nblk % nch come from the host.
__device__ __forceinline__ int chunk_begin(int c, const DdcShape &sh) {
    return c * sh.cbase + (c < sh.crem ? c : sh.crem);
}

// x mod rate for x < 2^63 with magic = floor((2^64 - 1) / rate) (Barrett): the
// quotient estimate is at most 2 short, so at most two subtractions follow.
__device__ __forceinline__ unsigned long long mod_rate(unsigned long long x, unsigned rate,
                                                       unsigned long long magic) {
    const unsigned long long q = __umul64hi(x, magic);
    unsigned long long r = x - q * rate;
    if (r >= rate) r -= rate;
    if (r >= rate) r -= rate;
    return r;
}

// exp(-2*pi*i * ph/rate) for an exact integer phase 0 <= ph < rate, in double to
// ~1e-13: octant reduction on t = ph/rate (t - k/8 is exact), Taylor series of
// degree 11/10 on |theta| <= pi/8, then a rotation by k*pi/4.
__device__ __forceinline__ void exact_phasor(unsigned long long ph, double inv_rate, double &re,
                                             double &im) {
    const double t = (double)ph * inv_rate;            // turns, [0, 1]
    const int k = (int)(t * 8.0 + 0.5);                // nearest eighth of a turn, 0..8
    const double th = (t - 0.125 * (double)k) * 6.283185307179586476925;   // |th| <= pi/8
    const double z = th * th;
    double s = -2.5052108385441718775e-08;             // -1/11!
    s = fma(s, z, 2.7557319223985890653e-06);          //  1/9!
    s = fma(s, z, -1.9841269841269841270e-04);         // -1/7!
    s = fma(s, z, 8.3333333333333333333e-03);          //  1/5!
    s = fma(s, z, -1.6666666666666666667e-01);         // -1/3!
    s = fma(s * z, th, th);
    double c = -2.7557319223985890653e-07;             // -1/10!
    c = fma(c, z, 2.4801587301587301587e-05);          //  1/8!
    c = fma(c, z, -1.3888888888888888889e-03);         // -1/6!
    c = fma(c, z, 4.1666666666666666667e-02);          //  1/4!
    c = fma(c, z, -0.5);
    c = fma(c, z, 1.0);
    // rotate by k * pi/4: (ck, sk) in {0, +-1, +-sqrt(1/2)}
    const double h = 0.70710678118654752440;
    const int kk = k & 7;
    const double ck = (kk == 0) ? 1.0 : (kk == 1 || kk == 7) ? h : (kk == 2 || kk == 6) ? 0.0
                    : (kk == 4) ? -1.0 : -h;
    const double sk = (kk == 0 || kk == 4) ? 0.0 : (kk == 1 || kk == 3) ? h : (kk == 2) ? 1.0
                    : (kk == 6) ? -1.0 : -h;
    const double cs = c * ck - s * sk;                 // cos(2*pi*t)
    const double sn = s * ck + c * sk;                 // sin(2*pi*t)
    re = cs;
    im = -sn;
}

// ---- sc16 output: a float32 component narrowed to int16 (include/gsdr.h, "sc16 output") ------------------
// v = c * gain (one IEEE multiply: the callers are compiled without contraction), r = v rounded to the nearest
// integer, ties to even (v_rndne_f32), saturated to [-32768, 32767], NaN -> 0.  The clamp comes before the
// conversion, so the conversion only ever sees an integer it can represent.  `clips` counts the components
// that did not fit (NaN included; r == -32768 fits).
__device__ __forceinline__ int narrow_component(float c, float gain, int &clips) {
#pragma clang fp contract(off)
    const float v = c * gain;
    const float r = __builtin_rintf(v);
    const bool nan = v != v, hi = r > 32767.0f, lo = r < -32768.0f;
    clips += (nan || hi || lo) ? 1 : 0;
    const float cl = nan ? 0.0f : hi ? 32767.0f : lo ? -32768.0f : r;
    return (int)cl;
}

// one sample as the dword a gsdr_sc16 is: I in the low half, Q in the high half (little endian: I first)
__device__ __forceinline__ int narrow_sample(float re, float im, float gain, int &clips) {
    const int i = narrow_component(re, gain, clips), q = narrow_component(im, gain, clips);
    return (i & 0xffff) | (int)((unsigned)q << 16);
}

// Integer sum over the 64 lanes of a wave with DPP row operations; the total arrives in lane 63.  Every lane of
// the wave must be active.
__device__ __forceinline__ int wave_isum_to_lane63(int x) {
#define GSDR_DPP_IADD(ctrl, row_mask) x += __builtin_amdgcn_update_dpp(0, x, ctrl, row_mask, 0xf, false)
    GSDR_DPP_IADD(0xB1, 0xf);    // quad_perm [1,0,3,2]
    GSDR_DPP_IADD(0x4E, 0xf);    // quad_perm [2,3,0,1]
    GSDR_DPP_IADD(0x141, 0xf);   // row_half_mirror
    GSDR_DPP_IADD(0x140, 0xf);   // row_mirror: every lane holds the sum of its row of 16
    GSDR_DPP_IADD(0x142, 0xa);   // row_bcast:15 into rows 1 and 3
    GSDR_DPP_IADD(0x143, 0xc);   // row_bcast:31 into rows 2 and 3
#undef GSDR_DPP_IADD
    return x;
}

// The clipped components of a wave added to the caller's counter: one vector atomic from lane 63, none when the
// wave clipped nothing (or no counter was given).  Called by whole waves, outside divergent control flow.
__device__ __forceinline__ void add_clips(unsigned long long *__restrict__ clipped, int clips, int lane) {
    const int total = wave_isum_to_lane63(clips);
    if (clipped && lane == 63 && total > 0)
        (void)__hip_atomic_fetch_add(clipped, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace gsdr
