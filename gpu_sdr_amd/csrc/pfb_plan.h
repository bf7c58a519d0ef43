// pfb_plan.h -- which kernel takes a TONES / NOISE call in the LDS and in what shape, decided in one place:
// launch_pfb_lds (fft_kernels.hip) launches what pfb_choose says, the demodulator (demod_pfb.cpp) asks the same functions
// when a handle is created, gsdr_pfb_plan (host_logic.cpp) shows the choice to a caller without a GPU.  No HIP here:
// host_logic.cpp is built alone by a host compiler.  A Bluestein plan enters as plain integers (its padded length m
// and the stages of m), not as an FftPlan, which owns device buffers.
#ifndef GSDR_PFB_PLAN_H
#define GSDR_PFB_PLAN_H

#include <cstddef>

#include "switches.h"

namespace gsdr {

// The whole PFB of a frame in one workgroup (filter, in-LDS transform, bin selection): frames of up to
// kPfbLdsMaxN points whose prime factors do not exceed kPfbLdsMaxPrime.
constexpr int kPfbLdsMaxN = 8192;
constexpr int kPfbLdsMaxPrime = 127;
constexpr int kPfbLdsTwMaxN = 4096;                       // up to here the twiddle table sits in the LDS as well
constexpr int kPfbLdsMaxBytes = (2 * kPfbLdsMaxN + kPfbLdsMaxPrime + 1) * 8;   // two frame buffers + roots: 129 KiB of the 160 KiB
// the run kernel (pfb_cu_kernel)
constexpr int kPfbCuThreads = 1024;
constexpr int kPfbCuPts = 6;                     // filter points per thread at most: G * n <= 6 * 1024
constexpr int kPfbCuMaxBytes = 156 * 1024;       // of the 160 KiB of a compute unit

// Which of the two kernels launch_pfb_lds() runs for a call of frames_n frames, and its shape
struct PfbChoice {
    bool cu;                   // pfb_cu_kernel (a run of frames per compute unit); false: pfb_lds_kernel
    int threads;               // per workgroup
    int G;                     // frames per workgroup (pfb_lds_kernel: FR)
    int twl;                   // the twiddle table sits in the LDS too
    size_t lds;                // dynamic LDS bytes
    int b_off, b_len, col, direct, dir_s, dir_gs, teams;   // pfb_cu_kernel only, see PfbCuArgs
};

// Stages of a transform through global memory, and of Bluestein's padded length m: 16s, 4s, then 2, then odd primes up
// to 13.  The number of stages (at most `cap` are written); 0 when a larger prime remains.
inline int fft_radices(int n, int *radices, int cap) {
    int cnt = 0, m = n;
    auto push = [&](int r) { if (cnt < cap) radices[cnt] = r; ++cnt; };
    while (m % 16 == 0) { push(16); m /= 16; }             // (round 3) two radix-4 levels per pass through memory
    while (m % 4 == 0) { push(4); m /= 4; }
    for (int p : {2, 3, 5, 7, 11, 13})
        while (m % p == 0) { push(p); m /= p; }
    return m == 1 ? cnt : 0;
}

// Stages of the in-LDS transform: 16s, 4s, 2, then every odd prime factor (3, 5, 7 with register
// butterflies, any larger prime through the one-output-per-item stage).  Empty when n does not fit:
// n > kPfbLdsMaxN, more than 16 stages, or a prime factor above kPfbLdsMaxPrime (its stage is O(R) per
// output: a 1021-point prime frame would be a plain DFT).
inline int pfb_lds_plan(int n, int *radices, bool radix8) {    // number of stages, -1 when the length does not fit
    if (n < 1 || n > kPfbLdsMaxN) return -1;
    int cnt = 0, m = n;
    auto push = [&](int r) { if (cnt < 16) radices[cnt] = r; ++cnt; };
    // prime factors above 13 first, the largest in front (its stage then needs no twiddles)
    int small = 1;
    for (int q : {2, 3, 5, 7, 11, 13})
        while (m % q == 0) { small *= q; m /= q; }
    int big[16], nbig = 0;
    for (int q = 17; q <= m; q += 2)
        while (m % q == 0) {
            if (q > kPfbLdsMaxPrime || nbig == 16) return -1;
            big[nbig++] = q;
            m /= q;
        }
    if (m != 1) return -1;
    for (int i = nbig - 1; i >= 0; --i) push(big[i]);
    m = small;
    // (round 3) Fewer, fatter stages -- every stage is a barrier, an LDS round trip and ~60 instructions of index
    // arithmetic per butterfly whatever its radix:
    //   * 16 (two radix-4 levels in registers) for frames of 4096 points and more: 4096 points 14.8 -> 13.3 us per
    //     buffer, 8192 27.0 -> 23.2.  Below that it does not pay: one thread in sixteen points busy leaves too few
    //     waves to hide each other's latencies (1024 points: two radix-16 stages take what four radix-4 stages took);
    //   * 8 (= 4 x 2) otherwise: one thread in eight points keeps half of the threads busy;
    //   * a single 2 left over joins a 3 or a 5: radix 6 / 10 (1230 = 41 * 6 * 5, 1000 = 8 * 5 * 5 * 5).
    // radix8 = false (GSDR_PFB_RADIX8=0): 4s and 2s as in round 2 (A/B runs)
    if (n >= 4096)
        while (m % 16 == 0) { push(16); m /= 16; }
    if (radix8)
        while (m % 8 == 0) { push(8); m /= 8; }
    while (m % 4 == 0) { push(4); m /= 4; }
    if (radix8 && m % 2 == 0 && m % 3 == 0) { push(6); m /= 6; }
    if (radix8 && m % 2 == 0 && m % 5 == 0) { push(10); m /= 10; }
    for (int q : {2, 3, 5, 7, 11, 13})
        while (m % q == 0) { push(q); m /= q; }
    return cnt <= 16 ? cnt : -1;
}

// Up to four taps and frames of 128 points and more: the run kernel filters straight out of global memory (one load per
// block and column instead of four, no trip through the LDS) and is the faster one for powers of two as well --
// same box, per 1 M-sample buffer: 256 points 10.1 against 10.3 us, 512: 10.2 / 10.8, 1024: 10.7 / 12.2, 2048:
// 10.4 / 11.9; 16 points 9.9 against 9.4 and 64 points equal: short frames stay a frame set per workgroup
// (profiles/r03_pfb_ab_direct.log).  GSDR_PFB_DIRECT=0 switches the direct filter off, and this rule with it.
inline bool pfb_cu_direct_pays(int nfft, int avg, const Switches &sw) {
    return sw.pfb_direct && avg >= 1 && avg <= 4 && nfft >= 128;
}

// Shape of the run-per-compute-unit kernel for frames of nfft points transformed at length `len` (nfft, or
// Bluestein's m): frames per workgroup G (at most `want`), the offset and size of the second LDS buffer, whether
// the twiddle table fits beside them.  False when not even one frame fits.
inline bool pfb_cu_shape(int nfft, int avg, int len, int want, int &G, int &b_off, int &b_len, int &twl, size_t &bytes,
                         int threads = kPfbCuThreads, long long max_bytes = kPfbCuMaxBytes, bool staged = true) {
    for (G = want < 1 ? 1 : want; G >= 1; --G) {
        if (staged && (long long)G * nfft > (long long)kPfbCuPts * threads) continue;
        const long long al = ((long long)G * len + 1) & ~1LL;                 // even: 16-byte LDS stores into the buffer behind
        long long bl = staged ? (long long)(G + avg - 1) * nfft : 0;          // (the direct filter stages no raw samples)
        if (bl < (long long)G * len) bl = (long long)G * len;
        bl = (bl + 1) & ~1LL;
        for (twl = len <= kPfbLdsTwMaxN ? 1 : 0; twl >= 0; --twl) {
            // + the bin table (n_out <= nfft ints)
            const long long total = (al + bl + kPfbLdsMaxPrime + 1 + (twl ? len : 0) + (nfft + 1) / 2 + 32) * 8LL;   // (+ 64 team counters)
            if (total <= max_bytes) {
                b_off = (int)al;
                b_len = (int)bl;
                bytes = (size_t)total;
                return true;
            }
        }
    }
    return false;
}

// Long frames, few of them: the run kernel gives every compute unit ceil(frames / units) frames, and with 325 frames
// of 3072 points that is two for 163 units and none for the rest (21 us per buffer against 15 a frame per workgroup,
// two workgroups per unit; profiles/r03_pfb_ab_4096.log).  The share of (unit, frame) slots a launch fills; below
// 0.7 the frame-per-workgroup kernel takes the call where it can (no matrix-core stage, no Bluestein).
inline double pfb_cu_fill(int nfft, int avg, int len, int frames_n, int cus) {
    if (frames_n <= 0 || cus <= 0) return 1.0;
    const int want = (frames_n + cus - 1) / cus;
    int G = 0, bo, bl, twl;
    size_t bytes;
    if (!pfb_cu_shape(nfft, avg, len, want, G, bo, bl, twl, bytes) &&
        !pfb_cu_shape(nfft, avg, len, want, G, bo, bl, twl, bytes, kPfbCuThreads, kPfbCuMaxBytes, false))
        return 1.0;
    const long long blocks = (frames_n + G - 1) / G, rounds = (blocks + cus - 1) / cus;
    return (double)frames_n / ((double)G * cus * rounds);
}

// does one frame fit the run kernel's LDS layout
inline bool pfb_cu_fits(int nfft, int avg, int len, const Switches &sw) {
    int G, bo, bl, twl;
    size_t bytes;
    if (!(nfft >= 1 && avg >= 1 && len >= nfft && len <= kPfbLdsMaxN)) return false;
    if (pfb_cu_shape(nfft, avg, len, 1, G, bo, bl, twl, bytes)) return true;
    // the direct filter keeps no raw samples in the LDS: a frame of up to four columns per thread fits without them
    return pfb_cu_direct_pays(nfft, avg, sw) && nfft <= 4 * kPfbCuThreads &&
           pfb_cu_shape(nfft, avg, len, 1, G, bo, bl, twl, bytes, kPfbCuThreads, kPfbCuMaxBytes, false);
}

// The padded length m = 2^ceil(log2(2 nfft - 1)) a handle transforms its frames at through Bluestein's identity inside
// the workgroup, 0 when it does not: a prime factor above kPfbLdsMaxPrime (or pfb_bluestein 1, GSDR_PFB_BLUESTEIN=1: any
// length, for tests; 0: never), when a frame at that length fits the LDS.
inline int pfb_blue_length(int nfft, int avg, int pfb_bluestein, const Switches &sw) {
    int r[16];
    const bool direct_ok = pfb_lds_plan(nfft, r, sw.pfb_radix8) >= 0;
    long long m = 1;
    while (m < 2LL * nfft - 1) m <<= 1;
    const bool ok = (pfb_bluestein < 0 ? !direct_ok : pfb_bluestein != 0) && m <= kPfbLdsMaxN && pfb_cu_fits(nfft, avg, (int)m, sw);
    return ok ? (int)m : 0;
}

// The run kernel's shape for a call of frames_n frames; false when it does not take the call.  radices: the stages
// of the transform (of length len: nfft, or Bluestein's m when blue).
inline bool pfb_cu_choose(PfbChoice &c, int nfft, int avg, int len, bool blue, int n_radices, const int *radices,
                          int frames_n, int n_out, int cus, const Switches &sw) {
    // one workgroup per compute unit: G consecutive frames each (frames_n == 0: a launch that only copies the carry)
    const int want = frames_n > 0 ? (frames_n + cus - 1) / cus : 1;
    if (n_out > nfft) return false;                       // the bin table in the LDS is sized for n_out <= nfft
    const bool big_prime = n_radices > 0 && radices[0] > 13;
    // the direct filter's variant for G frames on `threads` threads: 0 = none
    // (GSDR_PFB_DIRECT=0: staged through the LDS; GSDR_PFB_COL=0/1, GSDR_PFB_CU_NT=512/1024: A/B runs)
    auto direct_variant = [&](int G, int threads, int &dir_s, int &dir_gs) {
        const int cpt = (nfft + threads - 1) / threads;
        dir_s = cpt == 1 ? threads / nfft : 1;             // groups of threads (frames shorter than the workgroup)
        dir_gs = (G + dir_s - 1) / dir_s;                  // frames per group
        const int nb = dir_gs + 3;                         // (the register shapes are those of four taps)
        if (avg < 1 || avg > 4 || !sw.pfb_direct) return 0;
        if (cpt == 1 && nb <= 11) return dir_s > 1 ? 4 : 1;
        if (cpt <= 2 && nb <= 7) return 2;
        if (cpt <= 3 && nb <= 5) return 5;
        if (cpt <= 4 && nb <= 4) return 3;
        return 0;
    };
    c.threads = kPfbCuThreads;
    // two workgroups of 512 threads per unit, half the frames each, when the direct filter takes them -- for frames
    // below 1024 points without a matrix-core stage: same box, 128 ... 512 points 9.7 - 10.0 against 10.2 - 10.3 us,
    // 1000: 12.4 / 12.9; from 1024 points on the full workgroup wins (1024: 10.9 against 11.2, 2048: 10.5 / 11.9,
    // and the matrix-core stage wants its sixteen waves: 1230: 13.5 / 17.0), profiles/r03_pfb_ab_nt.log
    const bool half_pays = sw.pfb_cu_nt == 512 || (sw.pfb_cu_nt == 0 && nfft < 1024 && !big_prime);
    if (half_pays && avg >= 1 && avg <= 4 && sw.pfb_direct) {
        const int want2 = frames_n > 0 ? (frames_n + 2 * cus - 1) / (2 * cus) : 1;
        int G2 = 0, bo = 0, bl = 0, twl2 = 0, ds = 1, dg = 1;
        size_t lds2 = 0;
        if (pfb_cu_shape(nfft, avg, len, want2, G2, bo, bl, twl2, lds2, 512, kPfbCuMaxBytes / 2, false)) {
            const int v = direct_variant(G2, 512, ds, dg);
            if (v) {
                c.threads = 512;
                c.G = G2; c.b_off = bo; c.b_len = bl; c.twl = twl2; c.lds = lds2;
                c.direct = v; c.dir_s = ds; c.dir_gs = dg; c.col = 1;
            }
        }
    }
    if (c.threads == kPfbCuThreads) {
        if (pfb_cu_shape(nfft, avg, len, want, c.G, c.b_off, c.b_len, c.twl, c.lds)) {
            // column-wise filter: four taps, and enough columns for every thread
            c.col = avg == 4 && (sw.pfb_col < 0 ? nfft >= kPfbCuThreads / 2 : sw.pfb_col == 1);
            c.direct = direct_variant(c.G, kPfbCuThreads, c.dir_s, c.dir_gs);
        } else {
            // no room for the raw samples of a run: the direct filter needs none (4096 points: a frame per unit)
            if (!pfb_cu_shape(nfft, avg, len, want, c.G, c.b_off, c.b_len, c.twl, c.lds, kPfbCuThreads, kPfbCuMaxBytes, false))
                return false;                              // does not fit: the other kernel
            c.col = 1;
            while (c.G >= 1 && !(c.direct = direct_variant(c.G, kPfbCuThreads, c.dir_s, c.dir_gs))) --c.G;
            if (c.G < 1) return false;
        }
    }
    if (!blue && sw.pfb_cu != 1 && c.threads == kPfbCuThreads && !big_prime && pfb_cu_fill(nfft, avg, len, frames_n, cus) < 0.7)
        return false;                                      // the frame-per-workgroup kernel fills the chip better
    // teams: the frames of a run go through their stages independently (GSDR_PFB_TEAMS=0: all waves in step)
    bool plain = !blue && n_radices > 0;
    for (int i = 0; i < n_radices; ++i) plain = plain && radices[i] <= 16;
    c.teams = plain && sw.pfb_teams && c.G >= 2 && c.threads % c.G == 0 && (c.threads / c.G) % 64 == 0;
    c.cu = true;
    return true;
}

// blue_m > 0: the frames go through Bluestein's identity at that padded length, whose stages are blue_radices
inline PfbChoice pfb_choose(int nfft, int avg, int blue_m, int blue_n_radices, const int *blue_radices, int frames_n, int n_out,
                            int cus, const Switches &sw) {
    PfbChoice c{};
    int r[16];
    const int nr = pfb_lds_plan(nfft, r, sw.pfb_radix8);
    const bool blue = blue_m > 0;
    // A run of frames per compute unit (round 3) when the run fits the LDS and the length has a stage other than
    // radix 2 / 4 / 8 / 16 -- a prime above 13 (its stage runs on the matrix cores there), 3, 5, 7 ... --, goes
    // through Bluestein, or has four taps and at least 128 points (the direct filter, pfb_cu_direct_pays()).
    // Measured per 1 M-sample buffer (profiles/r03_pfb_sweep.log): 1230 points 19.7 -> 13.1 us, 1016: 21.5 -> 13.5,
    // 1024: 12.6 -> 10.9.  GSDR_PFB_CU=0 / 1 forces.
    const int cu_mode = sw.pfb_cu < 0 ? -1 : (sw.pfb_cu != 0);
    bool cu_wanted = cu_mode == 1 || blue;
    if (cu_mode < 0 && !blue) {
        for (int i = 0; i < nr; ++i) cu_wanted |= (r[i] != 4 && r[i] != 2 && r[i] != 16 && r[i] != 8);
        cu_wanted |= pfb_cu_direct_pays(nfft, avg, sw);
    }
    if (cu_wanted && (blue ? pfb_cu_choose(c, nfft, avg, blue_m, true, blue_n_radices, blue_radices, frames_n, n_out, cus, sw)
                           : nr >= 0 && pfb_cu_choose(c, nfft, avg, nfft, false, nr, r, frames_n, n_out, cus, sw)))
        return c;
    // a frame set per workgroup: short frames share one, at least ~1024 points of work per workgroup; GSDR_PFB_FR sets
    // the frames, GSDR_PFB_WIDE the 512 threads per frame (A/B runs)
    c = PfbChoice{};
    c.G = nfft >= 1024 ? 1 : (1024 + nfft - 1) / nfft;
    if (sw.pfb_fr > 0 && (long long)sw.pfb_fr * nfft <= 4096) c.G = sw.pfb_fr;
    if (c.G > 64) c.G = 64;
    c.twl = nfft <= kPfbLdsTwMaxN;
    c.threads = (sw.pfb_wide >= 0 ? sw.pfb_wide != 0 : nfft >= 2048) ? 512 : 256;
    c.lds = ((size_t)2 * c.G * nfft + kPfbLdsMaxPrime + 1 + (c.twl ? nfft : 0)) * 8;   // two frame sets + roots (+ twiddles)
    return c;
}

inline const char *pfb_kernel_name(const PfbChoice &c) { return c.cu ? "pfb_cu_kernel" : "pfb_lds_kernel"; }

}  // namespace gsdr

#endif
