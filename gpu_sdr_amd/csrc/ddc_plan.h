// ddc_plan.h -- which engine takes a DIRECT (or TONES-through-the-DDC) handle and how each of its launches is shaped,
// decided in one place: the demodulator (demod_ddc.cpp) asks these functions when a handle is created and for every
// launch, gsdr_ddc_plan (host_logic.cpp) shows the same answers to a caller without a GPU.  Functions of integers and
// of the switches only; no handle is passed.  No HIP here: host_logic.cpp is built alone by a host compiler.
// gsdr::product_loop(kind) in ddc_mfma.hip stays the one host description of a loop (image sizes, table builders); the
// rules here say which loop, and what describe() reports of it.
#ifndef GSDR_DDC_PLAN_H
#define GSDR_DDC_PLAN_H

#include <cmath>

#include "switches.h"

namespace gsdr {

// AsmRing16 / AsmRing16P / AsmRing16W8: assembly main loops on the 16x16x32 MFMA (production, pre-converted
// operands, eight-wave workgroups); AsmRing16P3: the pre-converted loop with three real products per complex
// multiply (chosen per handle, product_loop_chosen), AsmRing16P3R2: that loop rotating its partial sums once per pair of
// blocks (tables of mfma_build_tables3 with span 2 in bfrag3 / ptab3), AsmRing16P3F: three products over 64-sample spans
// folded about their centre (images of ddc_convert3f_kernel, tables of mfma_build_tables3f in bfrag3 / ptab3), AsmRing16P4F: that fold with the plain four products (images of
// ddc_convert4f_kernel, tables of mfma_build_tables4f), AsmRing16P4FW: that loop, images and tables on wave tiles of 16 rows x 64 tones; AsmRing16P4FW2: the wide-tile loop
// over spans of 128 samples folded about their centre (images of ddc_convert4f2_kernel, tables of mfma_build_tables4f2); AsmRing:
// round 1's loop on the 32x32x16 MFMA; Cxx: compiler-scheduled (TT, PK, W apply to it only; the assembly kernels are
// TT = 1, PK = 32, W = 4).
enum class MfmaKernel { AsmRing, Cxx, AsmRing16, AsmRing16W8, AsmRing16P, AsmRing16P3, AsmRing16P3R2, AsmRing16P3F, AsmRing16P4F, AsmRing16P4FW, AsmRing16P4FW2 };

constexpr int kMaxF = 8;           // tap phases the DDC kernel is instantiated for

// ---------------------------------------------------------------------------
// the engine of a handle
// ---------------------------------------------------------------------------

// ddc_flat_kernel (packed math, pipelined scalar loads) covers F <= 4 and is the engine of
// GSDR_DDC_MFMA=0, where no matrix-core loop runs on the GPU at all.  With the matrix cores enabled,
// a shape they do not take (windows shorter than a buffer row, ...) goes to the generic ddc_kernel:
// it is compiled without packed FP32, which is not safe beside the matrix-core loop of another
// handle on the same GPU (rule 3).  GSDR_DDC_PIPE=0 forces the generic kernel.
// (allow_flat false: the undecimated mix, which needs the NCO tables alone.)
inline bool ddc_flat_takes(int F, bool allow_flat, const Switches &sw) {
    return allow_flat && sw.ddc_pipe && F <= 4 && !sw.ddc_mfma;
}

// A handful of tones at a long decimation: every other engine walks a block's samples in sequence per
// tone lane / matrix column, and a launch is as long as one workgroup's walk (72 us per 1 M-sample
// buffer for 1 ... 256 tones at decim 1000).  ddc_few_kernel splits the block over the lanes of a wave
// per (chunk, tone): 16 tones at decim 1000 in 15 us (profiles/r03_shape_sweep.log).  GSDR_DDC_FEW=0: off.
// (N tones of a DIRECT handle in TW = ceil(N / 64) tone waves.)
inline bool ddc_few_takes(int N, int M, bool flat, const Switches &sw) {
    const int TW = (N + 63) / 64;
    return sw.ddc_mfma && sw.ddc_few && !flat && M >= 512 && N <= 32 && TW == 1;
}

// The matrix cores take a DIRECT shape of L samples per buffer, blocks of M samples and F tap phases when a buffer
// holds the carry of F - 1 blocks
// (rows read whole 32-sample phasor blocks: the padding behind a window must stay
//  within the next block, or middle rows would read past the buffer)
inline bool ddc_mfma_takes_direct(long long L, int M, int F, const Switches &sw) {
    return sw.ddc_mfma && L / M >= F - 1 && L >= 4 && F <= 33 && (M * F + 31) / 32 * 32 - M * F <= M;
}

enum class DdcEngine { Mix, Few, Flat, Generic, Mfma };      // (GSDR_DDC_ENGINE_* of include/gsdr.h, in this order)

// decim <= 0: the undecimated mix; else blocks of M = decim samples and F = pf_average tap phases
inline DdcEngine ddc_direct_engine(long long decim, int N, int M, int F, long long L, const Switches &sw) {
    if (decim <= 0) return DdcEngine::Mix;
    const bool flat = ddc_flat_takes(F, true, sw);
    if (ddc_few_takes(N, M, flat, sw)) return DdcEngine::Few;
    if (ddc_mfma_takes_direct(L, M, F, sw)) return DdcEngine::Mfma;
    return flat ? DdcEngine::Flat : DdcEngine::Generic;
}

// ---------------------------------------------------------------------------
// the VALU kernels: sub-block length and chunks
// ---------------------------------------------------------------------------

// K: the phasor-table length (the flat kernel's sub-block); pad: samples the flat kernel reads past a block
// (nsub*K - M); R: length of the last sub-block in real samples (generic kernel: M mod K)
struct DdcBlocking {
    int K, pad, R;
};
inline DdcBlocking ddc_blocking(bool flat, int M, const Switches &sw) {
    DdcBlocking b{16, 0, 0};
    if (flat) {
        // sub-block length: whole sub-blocks per block, cheapest total
        // (padded samples + ~3.3 sample-equivalents of fold work per sub-block).  40 since round 3: half the
        // folds and phasor steps of 20 at 124 instead of 82 registers (4 waves per SIMD instead of 5):
        // C3 460 -> 440 us in order (profiles/r03_flat_k.log)
        int forced = sw.ddc_k;
        if (forced != 12 && forced != 16 && forced != 20 && forced != 40) forced = 0;
        double best = 1e300;
        for (int k : {40, 20, 16, 12}) {
            if (forced && forced != k) continue;
            const long long nsub = (M + k - 1) / k;
            const double cost = (double)nsub * (k + 3.3);
            if (cost < best) {
                best = cost;
                b.K = k;
            }
        }
        const int nsub = (M + b.K - 1) / b.K;
        b.pad = nsub * b.K - M;
        b.R = M - (nsub - 1) * b.K;   // length of the last sub-block in real samples
    } else {
        b.K = sw.ddc_k == 32 ? 32 : 16;
        b.R = M % b.K;
    }
    return b;
}

// resident waves the DDC grid is sized for: per SIMD those of the kernel actually used (VGPR-limited)
inline int ddc_target_waves(int simds, bool flat, const Switches &sw) {
    return simds * (sw.ddc_waves > 0 ? sw.ddc_waves : flat ? 6 : 4);
}

// the tails buffer must hold the largest chunk count any launch may pick:
// largest autotune ratio (1.7) x the +20 % window of balanced_near(), or the
// forced count, but never more than one chunk per F-1 blocks
inline int ddc_tails_nch(int F, int max_nblk, int target_waves, int TW, int ddc_nch) {
    const long long cap = (F > 1) ? max_nblk / (F - 1) : max_nblk;
    long long worst = (long long)(1.7 * 1.2 * target_waves) / TW + 2;
    if (ddc_nch > worst) worst = ddc_nch;
    if (worst > cap) worst = cap;
    return (int)(worst < 1 ? 1 : worst);
}

// Chunk count closest to `want` (within +-20 %) that splits nblk blocks most
// evenly: the launch ends with its longest chunk.
inline long long balanced_near(long long want, int nblk, long long cap) {
    if (want < 1) want = 1;
    if (want > cap) want = cap;
    long long lo = want - want / 5, hi = want + want / 5;
    if (lo < 1) lo = 1;
    if (hi > cap) hi = cap;
    long long best_nch = want;
    double best = -1.0;
    for (long long nch = lo; nch <= hi; ++nch) {
        const long long longest = (nblk + nch - 1) / nch;
        const double balance = ((double)nblk / (double)nch) / (double)longest;
        const double score = balance - 0.05 * std::fabs((double)(nch - want)) / (double)want;
        if (score > best) {
            best = score;
            best_nch = nch;
        }
    }
    return best_nch;
}

// Number of chunks the blocks of one launch are cut into (one wave per chunk x
// 64 tones).  `waves_ratio` = grid waves / resident waves; 1.3 by default
// (measured on C3: a grid 1.3x what is resident -- the dispatcher hands the
// surplus workgroups to whichever CU frees up first -- beats an exactly
// resident one by 9 %), replaced by the autotuned value when create() could
// time the candidates (profiles/r01_chunk_sweeps.log shows why a fixed rule is
// not enough: C2 is best at 0.8, C3 at 1.3-1.7).
inline int pick_chunks(int nblk, double waves_ratio, int target_waves, int TW, int F, int tails_nch, int ddc_nch) {
    if (nblk <= 0) return 1;
    if (TW < 1) TW = 1;
    const long long cap = (F > 1) ? nblk / (F - 1) : nblk;  // every chunk >= F-1 blocks
    if (cap < 1) return 1;
    long long nch = ddc_nch > 0 ? (ddc_nch < cap ? ddc_nch : cap)
                                : balanced_near((long long)(waves_ratio * target_waves) / TW, nblk, cap);
    // never more chunks than the tails buffer has slots for (0 = not allocated yet)
    if (tails_nch > 0 && nch > tails_nch) nch = tails_nch;
    return (int)(nch < 1 ? 1 : nch);
}

// ---------------------------------------------------------------------------
// the matrix cores: kernel, product loop, and the choice per launch
// ---------------------------------------------------------------------------

// TT, PK, W: tone tiles per wave, phasor block, waves per workgroup (of the C++ kernel; the assembly kernels have one
// shape); kind: the main loop.
// the assembly main loops exist for the default shape only; GSDR_MFMA_ASM: 4 = LDS operand ring
// on v_mfma_f32_16x16x32_f16 (default since round 2: the same cycles per FLOP for less energy,
// +7 % on C3 under the power cap), 5 = that loop for workgroups of eight waves, 2 = the ring on
// v_mfma_f32_32x32x16_f16 (round 1's production kernel), 0 = the compiler-scheduled kernel (A/B runs, tests)
struct MfmaTile {
    int TT, PK, W;
    MfmaKernel kind;
};
inline MfmaTile mfma_tile(const Switches &sw) {
    MfmaTile t{sw.mfma_tt, sw.mfma_pk, sw.mfma_w, MfmaKernel::Cxx};
    if (t.W > t.PK / 8) t.W = t.PK / 8;   // every wave converts whole k-steps
    const bool asm_shape = t.TT == 1 && t.PK == 32 && t.W == 4;
    if (sw.mfma_asm == 2 && asm_shape) t.kind = MfmaKernel::AsmRing;
    if (sw.mfma_asm == 4 && asm_shape) t.kind = MfmaKernel::AsmRing16;      // tools/gen_ddc_mfma_ring16.py
    if (sw.mfma_asm == 5 && asm_shape) t.kind = MfmaKernel::AsmRing16W8;    // tools/gen_ddc_mfma_ring16w8.py
    return t;
}

// Pre-converted operands (ddc_convert_kernel + ddc_mfma_ring16p_kernel) for a launch of
// ngt row tiles of the AsmRing16 kernel.  GSDR_MFMA_PREC: 1 = always (tests), 0 = never, default:
//   in-order entries      launches of four rounds of workgroups or more (-9 % at 16 k ... 64 k tones;
//                         below that the pass, which runs in front of the loop there, costs more);
//   overlapped entries    launches of half a round or more with windows of 32 blocks or more: the
//                         pass of buffer j+1 runs beside the loop of buffer j (C3 139 -> 130.5 us per
//                         buffer, TONES 1024/1230 76.8 -> 74.0; C2, 13 blocks: neutral, not used).
// (simds: SIMDs of the device, 4 per compute unit; ntq: workgroups per row tile; nk8: k-steps of 8 samples of a window)
inline bool prec_pays(int simds, long long ngt, int ntq, int nk8, bool overlap, const Switches &sw) {
    const long long wgs4 = ((ngt + 7) / 8) * 8 * ntq;
    const long long nhi = (nk8 + 3) / 4;
    return sw.mfma_prec == 1 ||
           (sw.mfma_prec < 0 && (wgs4 >= 4LL * (simds / 2) || (overlap && wgs4 >= simds / 4 && nhi >= 32)));
}

// Three real products per complex multiply for a handle that has pre-converted images.
// The three operands a+b, d-c, c+d carry sqrt(2) more quantisation noise than a, b, c, d; on the weakest tones of a
// 60 dB comb that stays inside the project's rule (error <= max(1e-5, 3 x the reference's own fp32 error)) only
// where the window is long enough to average it: kMac3MinBlocks is the shortest window, in 32-sample blocks, from
// which test_gpu_mfma3.py::test_hdr_comb_sets_threshold measured the rule kept at every tested length.
// GSDR_MFMA_3M: 1 = wherever there are images, 0 = never.
constexpr long long kMac3MinBlocks = 94;

// A three-product handle rotates its partial sums into the accumulators once per pair of blocks
// (ddc_mfma_ring16p3r2_kernel) instead of once per block: half the rotation FMAs, phasor images
// of 64 samples instead of 32, and fewer fp32 roundings at the size of the partial sums (one rotation stage per pair,
// the small cross terms of the hi/lo split summed first).  kRot2MinBlocks is the shortest window from which
// test_gpu_mfma3r2.py::test_hdr_comb_default_keeps_the_rule measured the rule of kMac3MinBlocks kept at every tested
// length (err / bound 0.84, 0.78, 0.56 at 94, 125, 250 blocks; shorter windows were not measured and keep the
// 32-sample loop).  GSDR_MFMA_3M_ROT: 2 = every three-product handle, 1 (or anything else) = never.
constexpr long long kRot2MinBlocks = 94;

// A handle that rotates once per pair folds each 64-sample span about its centre (ddc_convert3f_kernel +
// ddc_mfma_ring16p3f_kernel): the phasor of sample j and of its partner 63 - j are conjugates, so
// two of the three sums run over 32 sums / differences of partners: 48 MFMAs per span instead of 72, still three real
// products per complex multiply and one rotation per two blocks.  The folded operands are sums of two products, which
// costs precision on the weakest tones of a 60 dB comb; kFoldMinBlocks is the shortest of the tested windows (94, 125,
// 250 blocks) from which test_gpu_fold.py::test_hdr_comb_fold_keeps_the_rule measured the rule of kMac3MinBlocks kept at
// it and every longer tested one (err / bound 0.84, 0.70, 0.51 at 94, 125, 250 blocks, against 0.84, 0.78, 0.56 not
// folded; DESIGN.md section 4.1f, profiles/fold_parity_margins.json).  GSDR_MFMA_FOLD: 1 = every handle that rotates per pair, 0 (or anything else) = never.
constexpr long long kFoldMinBlocks = 94;

// The arithmetic of a folded handle.  The plain four products fold completely -- the same
// four units of K = 32 and 48 MFMAs per span as the Gauss fold, whose third sum has no symmetry -- and need two
// product tile sets, the images of c and d only and 64 rotation FMAs per span instead of 96.  complex_mac,
// rotation_blocks and fold in describe() name the rule that selected the handle (the three above: unchanged);
// fold_products names what it computes.  GSDR_MFMA_FOLD_PRODUCTS: 3 = the Gauss fold, 4 = the
// direct fold, unset = kFoldProductsDefault.
constexpr int kFoldProductsDefault = 4;

// The wave tile of a handle that sums the plain four products: 16 rows x 64 tones
// (ddc_mfma_ring16p4fw_kernel) copies and reads half the operand bytes of 32 x 32 (ddc_mfma_ring16p4f_kernel) for the
// same MFMAs per wave and the same bits, but splits the rows over twice the workgroups and the tones over half of them.
// It is taken where it launches no more waves for the handle's largest row count -- many tones; with 128 tones or
// fewer it would run twice the workgroups, half of their waves idle.  GSDR_MFMA_WAVE_TONES: 64 = every such handle,
// 32 = never, unset = by that rule.
//
// The span of a handle on the wide tile: 128 samples folded about their centre
// (ddc_convert4f2_kernel + ddc_mfma_ring16p4fw2_kernel) take the MFMAs of two 64-sample spans and one rotation, one P
// load, one barrier and one ring rotation instead of two.  GSDR_MFMA_SPAN: 128 = every handle on the wide tile, 64 = never,
// unset = a handle that took the wide tile by its own rule (GSDR_MFMA_WAVE_TONES unset: a forced wave tile keeps the
// 64-sample spans and their bits) with a window of kSpan128MinBlocks blocks or more; 0: the unset rule never takes it.
constexpr long long kSpan128MinBlocks = 125;

// The six rules above for a handle that has images, each asked only of a handle the one before it took (a field is
// false where its rule was not asked).  nhi: the window in 32-sample blocks; max_rows, ntg: the handle's largest row
// count and its tone groups.
struct ProductRule {
    bool mac3, rot2, fold;
    int products;              // of a folded handle: 3 or 4; else 0
    bool wide, span128;
};
inline ProductRule product_rule(long long nhi, long long max_rows, long long ntg, const Switches &sw) {
    ProductRule r{};
    r.mac3 = sw.mfma_3m == 1 || (sw.mfma_3m < 0 && nhi >= kMac3MinBlocks);
    r.rot2 = r.mac3 && nhi >= 1 && (sw.mfma_3m_rot == 2 || (sw.mfma_3m_rot < 0 && nhi >= kRot2MinBlocks));
    r.fold = r.rot2 && (sw.mfma_fold == 1 || (sw.mfma_fold < 0 && nhi >= kFoldMinBlocks));
    const int p = sw.mfma_fold_products, w = sw.mfma_wave_tones;
    r.products = !r.fold ? 0 : p == 3 || p == 4 ? p : kFoldProductsDefault;
    r.wide = r.products == 4 &&
             (w == 32 || w == 64 ? w == 64 : ((max_rows + 15) / 16) * ((ntg + 7) / 8) <= ((max_rows + 31) / 32) * ((ntg + 3) / 4));
    r.span128 = r.wide && (sw.mfma_span == 128 || (sw.mfma_span < 0 && w < 0 && kSpan128MinBlocks > 0 && nhi >= kSpan128MinBlocks));
    return r;
}

// The loop of gsdr::product_loop for a handle with images by those rules (AsmRing16P: four products per block, the
// loop chosen per launch)
inline MfmaKernel product_loop_chosen(const ProductRule &r) {
    using K = MfmaKernel;
    return !r.mac3 ? K::AsmRing16P : !r.rot2 ? K::AsmRing16P3 : !r.fold ? K::AsmRing16P3R2 : r.products != 4 ? K::AsmRing16P3F
           : !r.wide ? K::AsmRing16P4F : r.span128 ? K::AsmRing16P4FW2 : K::AsmRing16P4FW;
}
inline MfmaKernel product_loop_chosen(long long nhi, long long max_rows, long long ntg, const Switches &sw) {
    return product_loop_chosen(product_rule(nhi, max_rows, ntg, sw));
}

// What describe() reports of a handle on the loop of rule r (the ProductLoop row of that loop holds the same values,
// tests/test_gpu_ddc_plan.py); ProductRule{}: every handle without a product loop of its own
struct ProductDescribe {
    int complex_mac, rotation_blocks, fold, fold_products, wave_tones, span_samples;
};
inline ProductDescribe product_describe(const ProductRule &r) {
    return {r.mac3 ? 3 : 4, r.rot2 ? 2 : 1, r.fold ? 1 : 0, r.products, r.wide ? 64 : 32, r.span128 ? 128 : 64};
}

// Row tiles per workgroup of one launch of ngt row tiles.  one_loop: the handle sends every launch through the
// kernel pair of its product loop, a row tile per workgroup.  GSDR_MFMA_RT: 1, 2 = forced.
inline int mfma_row_tiles(bool one_loop, bool overlap, int nk8, long long ngt, int ntq, const Switches &sw) {
    if (one_loop) return 1;       // one kernel pair for every launch of the handle
    if (sw.mfma_rt != 0) return sw.mfma_rt;
    // Two row tiles per workgroup (the second keeps the phasor images: 64 KiB less to load, one
    // preamble less, half as many workgroups).  Measured at decim 100 (13-block windows) for
    // 128 .. 2048 tones, in order and overlapped (scratch/rt_probe.py): it pays in exactly one
    // place, a launch of between one and two rounds of workgroups in the overlapped entries
    // (256 tones, 626 workgroups: 31.3 -> 29.4 us per buffer), where the neighbouring launches
    // fill the compute units that 313 longer workgroups leave free; everywhere else it is
    // neutral or costs up to 15 % (in order, few workgroups).
    const int nblk = (nk8 + 3) / 4;
    const long long wgs = ngt * ntq;
    return overlap && nblk <= 32 && wgs >= 512 && wgs < 1024 ? 2 : 1;
}

// The kernel of one launch of a handle whose main loop is `base` and that has no product loop of its own.  images:
// the handle has image sets; rt: mfma_row_tiles of the launch.
inline MfmaKernel mfma_launch_kernel(MfmaKernel base, bool images, int rt, int simds, long long ngt, int ntq, int ntg, int nk8,
                                     bool overlap, const Switches &sw) {
    if (base != MfmaKernel::AsmRing16) return base;
    if (images && rt <= 1 && prec_pays(simds, ngt, ntq, nk8, overlap, sw)) return MfmaKernel::AsmRing16P;
    // One launch at a time (in-order entries) that needs the two workgroups per compute unit the
    // 4-wave kernel is resident with: the hardware serves the older of the two first, the younger ends
    // 40 % later and runs the tail alone.  If the launch fits the compute
    // units as 8-wave workgroups (same tables, same loop, the two waves of a SIMD barrier-coupled
    // partners), that kernel ends 4-7 % earlier (C3: 145 against 152-158 us).  The overlapped entries
    // keep the 4-wave kernel: there the next buffer's workgroups fill the slots the older ones free.
    if (!overlap && sw.mfma_w8) {
        const long long wgs4 = ((ngt + 7) / 8) * 8 * ntq;
        const long long wgs8 = ((ngt + 7) / 8) * 8 * ((ntg + 7) / 8);
        if (rt <= 1 && wgs4 > simds / 4 && wgs4 <= simds / 2 && wgs8 <= simds / 4) return MfmaKernel::AsmRing16W8;
    }
    return base;
}

}  // namespace gsdr

#endif
