// ddc_kernels.h -- launch interface of the fused DDC kernels (internal).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "chirp_plan.h"
#include "ddc_plan.h"
#include "pfb_plan.h"
#include "switches.h"
#include "dev_owner.h"

// No packed FP32 (v_pk_*_f32) in a kernel that may share a SIMD with the matrix-core DDC loop of another
// launch -- another handle on the same GPU, or the neighbouring buffer of this one: a v_pk_*_f32 with a
// high-half broadcast returned stale values in some lanes while another wave of the SIMD ran an MFMA loop
// (rule R3; tools/ubench_pk_hazard.hip; scratch/concurrent_handles.py shows it across
// kernels).  Device helpers used by such a kernel must be always_inline.
#ifndef GSDR_NO_PK        // (scratch/pk_hazard_ab.sh builds a variant with packed FP32 to show the hazard)
#define GSDR_NO_PK __attribute__((target("no-packed-fp32-ops")))
#endif

namespace gsdr {

// Shape of one DDC launch; passed to the kernels by value.
struct DdcShape {
    int N;                     // tones
    int Npad;                  // tones rounded up to 64 (table pitch)
    int TW;                    // tone waves = Npad / 64
    int M;                     // samples per block (decimation / nfft)
    int nblk;                  // input blocks in this launch
    int nch;                   // chunks the blocks are split into
    int cbase, crem;           // nblk / nch and nblk % nch (chunk_begin(), no device division)
    int g_off;                 // first output kept; out row = G - g_off
    unsigned rate;             // NCO modulus (sample rate, or nfft for TONES)
    unsigned long long idx0;   // NCO index of x[0] (mod rate)
    unsigned long long rate_magic;  // floor((2^64-1)/rate), Barrett reduction mod rate
    double inv_rate;           // 1.0 / rate
    unsigned m_mod_rate;       // M mod rate
    long long total;           // mix_kernel only: number of samples
    long long xlast;           // ddc_flat_kernel: x[0 .. xlast+4) is readable
    int prefetch;              // ddc_flat_kernel: LDS-DMA L2 prefetch of the IQ stream on/off
};

struct DdcLaunch {
    const float2 *x;
    const float *taps_t;    // [M][F]                 (ddc_kernel)
    const float *taps_p;    // [nsub*PK+2][FP] zero padded (ddc_flat_kernel), FP = 1,2,4
    const float2 *btab;
    const double2 *wk;
    const double2 *wrem;
    const unsigned *fmod;
    float2 *out;
    float2 *tails;
    int tails_nch;          // chunk slots `tails` was allocated for (launch_ddc refuses more)
    const float2 *carry_in;
    float2 *carry_out;
    DdcShape sh;
    unsigned lds_bytes;     // dynamic LDS per workgroup (occupancy cap, see launch_flat_fk)
    bool pipe;              // use ddc_flat_kernel (F <= 4, phasor table length K in {12,16,20})
    bool few;               // use ddc_few_kernel (a wave per (chunk, tone): a handful of tones at a long decimation)
};

// F = tap phases (pf_average, 1..8), K = phasor-table length (16 or 32; 12/16/20
// when a.pipe selects ddc_flat_kernel).
// Enqueues ddc_kernel<F,K> and, when F > 1, ddc_fixup.  `stop` (may be null)
// is recorded right after ddc_kernel, before the fixup.
hipError_t launch_ddc(int F, int K, const DdcLaunch &a, hipStream_t st, hipEvent_t stop);
const char *ddc_few_kernel_name();
// Undecimated DIRECT (decim == 0); mix_few: Switches::mix_few.
hipError_t launch_mix(int K, const DdcLaunch &a, int mix_few, hipStream_t st);

hipError_t launch_ddc_flat_main(int F, int PK, const DdcLaunch &a, hipStream_t st);
const char *ddc_kernel_name();
const char *ddc_flat_kernel_name();
const char *mix_kernel_name(int n_tones, int tw, long long total, int K, int mix_few);   // what launch_mix runs
// sc16 input: out[k] = (float(in[k].i) * scale, float(in[k].q) * scale), k < n; `in` holds n interleaved int16 pairs
// (4-byte aligned), `out` is 8-byte aligned; cus = compute units the grid is sized to.  n <= 0 launches nothing.
hipError_t launch_widen_sc16(const void *in, float2 *out, long long n, float scale, int cus, hipStream_t st);
// sc16 output: out[k] = narrowed in[k] (include/gsdr.h, "sc16 output"); `in` 8-byte, `out` 4-byte aligned device
// pointers to n samples, `clipped` (may be null, 8-byte aligned) gets the number of clipped components added.
hipError_t launch_narrow_sc16(const float2 *in, void *out, long long n, float gain, unsigned long long *clipped, int cus,
                              hipStream_t st);

// ---- DDC on the matrix cores (ddc_mfma.hip) --------------------------------
struct MfmaShape {
    int N;                     // tones
    int NT32;                  // 32-tone tiles the tables hold (= ntg * TT)
    int ntg;                   // tone groups (one wave each) = ceil(ceil(N/32) / TT)
    int ntq;                   // workgroups per row tile = ceil(ntg / 4)
    int ngt;                   // row tiles = ceil(nout / 32)
    int M;                     // samples per block
    int MF;                    // window length in samples (M * F)
    int F;                     // tap phases (blocks of M samples a window spans)
    int nk8;                   // MFMA k-steps of 8 samples = ceil(MF / 8)
    int nout;                  // output rows of this launch
    int woff;                  // row o's window starts at sample (o + woff) * M
    int carry_len;             // samples of history in front of sample 0 (in `head`)
    long long tail0;           // first sample held by `tail`
    long long nx;              // x[0 .. nx) is readable
    unsigned rate;             // NCO modulus
    unsigned long long rate_magic;
    double inv_rate;
    unsigned m_mod_rate;
    unsigned idx_base;         // NCO index of sample woff*M (mod rate)
    int seg_k;                 // blocks of M samples per segment of the maxima table (segment = seg_k * M samples)
    float unscale;             // power of two the taps were divided by
    int rt;                    // ring kernel: row tiles a workgroup does one after the other (0, 1: one)
    int timing_mode;           // GSDR_MFMA_TIMING (wrong results): 1 = no stores, 2 = one block only, 3 = both
};

struct MfmaLaunch {
    const float2 *x;
    const float2 *head;        // row tile 0 reads here: sample s at head[s + carry_len]
    const float2 *tail;        // last row tile reads here: sample s at tail[s - tail0], zeros past nx
    const float *taps;         // [nk8*8 + 8] scaled, zero padded
    const uint4 *bfrag;        // phasor-table operand images, see mfma_build_tables
    const float2 *ptab;        // [ceil(nk8/KS)][NT32*32]  w_n^(hi*PK)
    const float2 *dtab;        // [32][NT32*32]            w_n^(row*M)
    const unsigned *fmod;      // [NT32*32]
    const unsigned *segmax;    // this call's table of segment maxima (float bits) over [carry | buffer], see absmax_kernel
    float2 *out;
    const uint4 *img;          // AsmRing16P: [ngt][nhi] pre-converted ring-slot images of 8 KiB (ddc_convert_kernel);
                               // AsmRing16P3: of 12 KiB (ddc_convert3_kernel); AsmRing16P3F: [ngt][ceil(nhi/2)] of 16 KiB
                               // (ddc_convert3f_kernel); AsmRing16P4F: the same of ddc_convert4f_kernel; AsmRing16P4FW2:
                               // [ngt][ceil(nhi/4)] of 32 KiB (ddc_convert4f2_kernel)
    const uint4 *bfrag3;       // AsmRing16P3 / AsmRing16P3R2: phasor images c, d-c, c+d of mfma_build_tables3, span 1 / 2
                               // AsmRing16P3F: c, d, c+d, c-d of mfma_build_tables3f; AsmRing16P4F: c, d of mfma_build_tables4f
    const float4 *ptab3;       // AsmRing16P3: [ceil(nk8/4) + 1][NT32*32]  (Pr, Pi, Pr-Pi, Pr+Pi) of w_n^(hi*32);
                               // AsmRing16P3R2: [ceil(ceil(nk8/4) / 2) + 1][NT32*32] of w_n^(pair*64)
    MfmaShape sh;
};

struct MfmaPlan {
    int TT, PK;                // tone tiles per wave (1, 2), phasor block (16, 32)
    int ntg, nk8, MF, M;
    unsigned rate;
    bool x16;                  // phasor images in the v_mfma_f32_16x16x32_f16 layout (AsmRing16)
};

void mfma_build_tables(const MfmaPlan &pl, const std::vector<unsigned> &fmod_in, const float *window,
                       std::vector<uint4> &bfrag, std::vector<float2> &ptab,
                       std::vector<float2> &dtab, std::vector<float> &taps,
                       std::vector<unsigned> &fmod, float &unscale);
// span: blocks of 32 samples per rotation of the three-product loop, 1 (AsmRing16P3) or 2 (AsmRing16P3R2)
void mfma_build_tables3(const MfmaPlan &pl, int span, const std::vector<unsigned> &fmod, std::vector<uint4> &bfrag3,
                        std::vector<float4> &ptab3);
// the folded loop (AsmRing16P3F): images c, d, c+d, c-d of w^(j - 31.5), j < 32, and (Pr, Pi, Pi-Pr, Pr+Pi) of w_n^(64*span + 31.5)
void mfma_build_tables3f(const MfmaPlan &pl, const std::vector<unsigned> &fmod, std::vector<uint4> &bfrag3,
                         std::vector<float4> &ptab3);
// the direct folded loop (AsmRing16P4F): images c, d of w^(j - 31.5), j < 32, and the span phasors of mfma_build_tables3f
void mfma_build_tables4f(const MfmaPlan &pl, const std::vector<unsigned> &fmod, std::vector<uint4> &bfrag3,
                         std::vector<float4> &ptab3);
// the direct folded loop over 128-sample spans (AsmRing16P4FW2): images c, d of w^(j - 63.5), j < 64 (K-half 0: j < 32, then K-half 1),
// and (Pr, Pi, Pi-Pr, Pr+Pi) of w_n^(128*span + 63.5)
void mfma_build_tables4f2(const MfmaPlan &pl, const std::vector<unsigned> &fmod, std::vector<uint4> &bfrag3,
                          std::vector<float4> &ptab3);
// The staging pass in front of the matrix-core kernels.  The logical stream of a call is T = [B | A]: A the new
// buffer x[0 .. n), B what the previous call left in front of it (DIRECT: the raw-sample carry, read from the head
// copy the previous pass wrote; TONES: the unconsumed end of the previous raw window, copied to b_dst).  One pass
//   * folds max |finite component| of every segment T[q*seg_len, (q+1)*seg_len) into seg[q] (float bits,
//     atomicMax on a table the previous pass cleared; NaN and Inf patterns are left out: they must not set the
//     scale of the ordinary samples around them) and clears seg_clear[0 .. nseg_alloc) for the next call;
//   * lays out the copies the main kernels read without boundary cases: head_cur[carry_len + i] = x[i], i < head_n;
//     head_next[i - (n - carry_len)] = x[i] for the last carry_len samples; tail[i - tail0] = x[i], i >= tail0.
struct StageLaunch {
    const float2 *x;           // A
    long long n;
    const float2 *b;           // B (may be null when nb == 0)
    long long nb;
    float2 *b_dst;             // copy of B (TONES), or null
    unsigned *seg, *seg_clear;
    int nseg_alloc;            // entries of a table
    long long seg_len;         // samples per segment
    float2 *head_cur;
    long long head_n;
    float2 *head_next;
    int carry_len;
    float2 *tail;
    long long tail0;
};
hipError_t launch_absmax(const StageLaunch &s, hipStream_t st);
// (the kernels: enum class MfmaKernel, ddc_plan.h)
hipError_t launch_ddc_mfma(MfmaKernel kind, int TT, int PK, int W, const MfmaLaunch &a, hipStream_t st);
const char *ddc_mfma_kernel_name(MfmaKernel kind);
// What the host knows of one loop of the pre-converted family (AsmRing16P ... AsmRing16P4FW, all named
// ddc_mfma_ring16p_kernel).  The rows stand in ddc_mfma.hip next to launch_ddc_mfma, which keeps each loop's conversion
// kernel, loop kernel and grid rule beside them; demod_ddc.cpp picks a handle's row once (product_loop_chosen, ddc_plan.h) and sizes,
// fills, launches and describes by it.
struct ProductLoop {
    MfmaKernel kind;
    int complex_mac, rotation_blocks, fold, fold_products, wave_tones;      // the handle's describe() values
    int image_blocks;          // 32-sample blocks an image of MfmaLaunch::img holds: 1, 2 (a folded span) or 4 (a folded span of 128 samples)
    int image_uint4;           // uint4 per image: 512 (8 KiB), 768 (12 KiB), 1024 (16 KiB) or 2048 (32 KiB)
    // bfrag3 / ptab3 of the loop; null: AsmRing16P reads the tables of mfma_build_tables only
    void (*build_tables)(const MfmaPlan &pl, const std::vector<unsigned> &fmod, std::vector<uint4> &bfrag3, std::vector<float4> &ptab3);
};
const ProductLoop *product_loop(MfmaKernel kind);      // null: `kind` is not of the family

// ---- batched FFT of arbitrary length + polyphase filter (NOISE mode, fft_kernels.hip) ----
struct FftPlan {
    int n = 0;                 // transform length
    int m = 0;                 // 0: mixed-radix Stockham stages over n; else Bluestein through length m = 2^k
    int n_radices = 0;
    int radices[32] = {};      // stages of n (m == 0) or of m
    DevBuf<float2> d_tw;       // w_len^k, len = n or m
    DevBuf<float2> d_chirp;    // Bluestein: exp(+i pi k^2 / n), k < n
    DevBuf<float2> d_bhat;     // Bluestein: transform of the wrapped chirp, length m
};
int fft_plan_build(FftPlan &pl, int n);   // (a plan releases its tables when it is destroyed or built anew)
// [batch][n] in src -> [batch][n] in dst; src and tmp are scratch of batch * max(n, m) each (src is destroyed)
hipError_t fft_forward(const FftPlan &pl, float2 *src, float2 *dst, float2 *tmp, int batch, hipStream_t st);
// frames[r][k] = sum_{i<avg} raw[(r+i)*nfft + k] * window[i*nfft + k], r < frames_n (ref: cpp/kernels.cu:474-516)
hipError_t launch_pfb_filter(const float2 *raw, const float *window, int nfft, int avg, int frames_n, float2 *frames,
                             hipStream_t st);
// out[frame][u] = spectra[frame][sel[u]], u < n_out (ref: tone_select, cpp/kernels.cu:520-554)
hipError_t launch_pfb_select(const float2 *spectra, int nfft, int frames_n, const int *sel, int n_out, float2 *out, hipStream_t st);
// mean of k consecutive frames per channel (the contract: include/gsdr.h, gsdr_frame_average_device): frames
// [n_frames][n_ch] behind `count` < k frames already summed in acc_in; (count + n_frames) / k rows to out, the open
// group's sums (or zeros) to acc_out; one launch, also when n_frames == 0
hipError_t launch_pfb_average(const float2 *frames, long long n_frames, int n_ch, int k, int kind, int count, const float2 *acc_in,
                              float2 *acc_out, float2 *out, hipStream_t st);
const char *fft_kernel_name();
// The whole PFB of a frame in one workgroup (filter, in-LDS transform, bin selection): frames of up to
// kPfbLdsMaxN points whose prime factors do not exceed kPfbLdsMaxPrime.  Which kernel takes a call, and in what
// shape, is pfb_plan.h's to say (pfb_lds_plan, pfb_cu_fits, pfb_choose, PfbChoice, the kPfb* limits).
// logical window [carry (new_0 samples) | in (window_len - new_0)]; frames_n complete frames -> out[frame][n_out]
// (sel: bin per output column, nullptr = all nfft bins); W[spare_begin .. +spare_n) -> carry_out
// (round 3) a run of consecutive frames per compute unit when it fits the LDS, else a frame per workgroup; `blue`:
// transform through Bluestein's identity at length blue->m (frame lengths with a prime factor above kPfbLdsMaxPrime;
// tw is then the table of length m, blue->d_tw)
// `*kernel`: the name of the kernel launched (left alone when nothing was); `*used`, when given: the choice the call
// was launched by (also when it had nothing to launch)
hipError_t launch_pfb_lds(const float2 *carry, int new_0, const float2 *in, const float *window, const float2 *tw,
                          int nfft, int avg, int frames_n, const int *sel, int n_out, float2 *out,
                          float2 *carry_out, int spare_begin, int spare_n, long long window_len, hipStream_t st,
                          const FftPlan *blue, const Switches &sw, const char **kernel, PfbChoice *used = nullptr);

// ---- chirp ---------------------------------------------------------------
// (every chirp launcher below leaves the form it launched in *used when that is given: chirp_plan.h)
struct ChirpShape {
    unsigned long long num_steps, length, period;  // period = num_steps*length
    unsigned chirpness;
    int f0;
};

// out[o] = in[o] * conj(chirp(index0 + o)), o < n
hipError_t launch_chirp_demod(const float2 *in, float2 *out, long long n,
                              unsigned long long index0, const ChirpShape &cs, hipStream_t st, ChirpPlan *used = nullptr);
// y[v] = sum_p demod(stage[v*ppt+p]) * profile[p], v < valid, where the logical
// stage is [carry (carry_len samples) | in]; index0 is the chirp index of stage[0].
hipError_t launch_chirp_lockin(const float2 *carry, int carry_len, const float2 *in,
                               const float *profile, int ppt, int valid, float2 *out,
                               unsigned long long index0, const ChirpShape &cs, hipStream_t st,
                               bool split, float2 *partial, int partial_cap,    // partial sums of split points (may be null)
                               ChirpPlan *used = nullptr);
hipError_t launch_warm(hipStream_t st);
// TX tone comb: out[s] = sum_k q0[k] w_k^(start + s), s < n; fmod = f mod rate, btab[k][64] = w_k^lo,
// ctab[k][16] = w_k^(64 j), w_k = e^(+2 pi i f_k / rate) (ref: tone_gen, cpp/kernels.cu:589-684)
hipError_t launch_tones_synth(float2 *out, long long n, unsigned long long start, unsigned rate, const unsigned *fmod,
                              const float2 *q0, const float2 *btab, const float2 *ctab, int n_tones, hipStream_t st);
// the same samples narrowed to sc16 in the lane that holds them (out: 4-byte aligned, gsdr_sc16)
hipError_t launch_tones_synth_sc16(void *out, long long n, unsigned long long start, unsigned rate, const unsigned *fmod,
                                   const float2 *q0, const float2 *btab, const float2 *ctab, int n_tones, float gain,
                                   unsigned long long *clipped, hipStream_t st);
const char *chirp_demod_kernel_name();
const char *chirp_lockin_kernel_name();

// ---- several chirps in one pass (GSDR_CREATE_MULTI_CHIRP) ------------------
// The chirps share swipe_s and chirp_t, so num_steps, length and the period are common and the running index is one;
// only f0 and chirpness differ.  Passed to the kernels by value: every field is wave-uniform.
constexpr int kMultiChirpMax = 16;      // GSDR_MULTI_CHIRP_MAX
constexpr int kChirpGroup = 4;          // the lock-in kernels keep their per-chirp state in register arrays of whole groups
// (The per-chirp tables are vectors, not arrays: a kernel takes the structure as an argument and indexes it with a loop
//  counter, and an array indexed that way makes the compiler copy the whole argument to scratch memory first; a vector
//  is one value in scalar registers, whatever the index.)
typedef int MultiChirpI __attribute__((ext_vector_type(kMultiChirpMax)));
typedef unsigned MultiChirpU __attribute__((ext_vector_type(kMultiChirpMax)));
typedef float MultiChirpF __attribute__((ext_vector_type(kMultiChirpMax)));
struct MultiChirp {
    unsigned long long num_steps, length, period;
    int n;                              // 1 ... kMultiChirpMax
    MultiChirpI f0;
    MultiChirpU chirpness;
};
struct MultiScale {
    MultiChirpF s;
};
__host__ __device__ __forceinline__ ChirpShape chirp_shape_of(const MultiChirp &mc, int c) {
    ChirpShape cs;
    cs.num_steps = mc.num_steps;
    cs.length = mc.length;
    cs.period = mc.period;
    cs.chirpness = mc.chirpness[c];
    cs.f0 = mc.f0[c];
    return cs;
}
// out[o * n + c] = in[o] * conj(chirp_c(index0 + o)), o < n_samples: the samples are read once
hipError_t launch_chirp_multi_demod(const float2 *in, float2 *out, long long n_samples, unsigned long long index0,
                                    const MultiChirp &mc, hipStream_t st, ChirpPlan *used = nullptr);
// launch_chirp_lockin for every chirp of mc at once: out[v * n + c]; partial holds [point][part][chirp]
hipError_t launch_chirp_multi_lockin(const float2 *carry, int carry_len, const float2 *in, const float *profile, int ppt,
                                     int valid, float2 *out, unsigned long long index0, const MultiChirp &mc, hipStream_t st,
                                     bool split, float2 *partial, int partial_cap, ChirpPlan *used = nullptr);
const char *chirp_multi_demod_kernel_name();
const char *chirp_multi_lockin_kernel_name();

// ---- synthetic sources ---------------------------------------------------
hipError_t launch_source_tones(float2 *out, long long n, long long start, unsigned rate,
                               const unsigned *fmod_dev, const float *ampl_dev,
                               const float *phase_dev, int n_tones, float sigma,
                               unsigned long long seed, hipStream_t st);
hipError_t launch_source_chirp(float2 *out, long long n, unsigned long long index0,
                               const ChirpShape &cs, float scale, hipStream_t st);
hipError_t launch_source_chirp_sc16(void *out, long long n, unsigned long long index0, const ChirpShape &cs, float scale,
                                    float gain, unsigned long long *clipped, hipStream_t st);
// out[s] = term_0 + term_1 + ... in chirp order, term_c the sample launch_source_chirp writes for chirp c with sc.s[c];
// every addition one IEEE single-precision operation.  _sc16: that sum narrowed, clipped components counted on the sum.
hipError_t launch_source_multichirp(float2 *out, long long n, unsigned long long index0, const MultiChirp &mc,
                                    const MultiScale &sc, hipStream_t st);
hipError_t launch_source_multichirp_sc16(void *out, long long n, unsigned long long index0, const MultiChirp &mc,
                                         const MultiScale &sc, float gain, unsigned long long *clipped, hipStream_t st);

}  // namespace gsdr
