// demod_ddc.cpp -- DIRECT, and the DDC engines every tone mode can run on: the NCO tables and taps of the VALU kernels,
// the tables and staging of the matrix-core kernels, and the launch of either.  Which engine, which loop and which
// kernel per launch is ddc_plan.h's to say; nothing here decides.
//
// "ref:" citations name the reference's files, as in demod.cpp.
#include "demod_state.h"

namespace gsdr {
namespace rx {

namespace {

// Builds the per-tone NCO tables of the DDC kernel (see ddc_kernels.hip):
//   fmod[n] = f_n mod rate, btab[lo][n] = w_n^lo, wk[n] = w_n^K, wrem[n] = w_n^R.
int build_nco_tables(gsdr_demod *h, const std::vector<long long> &tone, unsigned rate) {
    const int Npad = h->ddc.Npad, K = h->ddc.K;
    std::vector<unsigned> fmod(Npad, 0u);
    std::vector<float2> btab((size_t)K * Npad);
    std::vector<double2> wk(Npad), wrem(Npad);
    for (int n = 0; n < Npad; ++n) {
        const unsigned long long fm = n < h->ddc.channels ? mod_rate(tone[n], rate) : 0u;
        fmod[n] = (unsigned)fm;
        for (int lo = 0; lo < K; ++lo) {
            double re, im;
            phasor((fm * (unsigned long long)lo) % rate, rate, re, im);
            btab[(size_t)lo * Npad + n] = make_float2((float)re, (float)im);
        }
        double re, im;
        phasor((fm * (unsigned long long)K) % rate, rate, re, im);
        wk[n] = make_double2(re, im);
        phasor((fm * (unsigned long long)h->ddc.R) % rate, rate, re, im);
        wrem[n] = make_double2(re, im);
    }
    HIPCHK(h, h->ddc.d_fmod.upload(fmod));
    HIPCHK(h, h->ddc.d_btab.upload(btab));
    HIPCHK(h, h->ddc.d_wk.upload(wk));
    HIPCHK(h, h->ddc.d_wrem.upload(wrem));
    return 0;
}

// taps_t[m*F + j] = h[j*M + m]: the F tap phases of input sample m, contiguous.
int upload_taps_transposed(gsdr_demod *h) {
    std::vector<float> t((size_t)h->ddc.M * h->ddc.F);
    for (int j = 0; j < h->ddc.F; ++j)
        for (int m = 0; m < h->ddc.M; ++m) t[(size_t)m * h->ddc.F + j] = h->window[(size_t)j * h->ddc.M + m];
    HIPCHK(h, h->ddc.d_taps_t.upload(t));
    if (h->ddc.flat) {
        const int FP = h->ddc.F == 3 ? 4 : h->ddc.F;
        std::vector<float> p((size_t)(h->ddc.M + h->ddc.pad + 2) * FP, 0.f);
        for (int j = 0; j < h->ddc.F; ++j)
            for (int m = 0; m < h->ddc.M; ++m) p[(size_t)m * FP + j] = h->window[(size_t)j * h->ddc.M + m];
        HIPCHK(h, h->ddc.d_taps_p.upload(p));
    }
    return 0;
}

}  // namespace

// gsdr::pick_chunks (ddc_plan.h) for a launch of nblk blocks of this handle
int pick_chunks(const gsdr_demod *h, int nblk) {
    return gsdr::pick_chunks(nblk, h->ddc.waves_ratio, h->ddc.target_waves, h->ddc.TW, h->ddc.F, h->ddc.tails_nch, h->sw.ddc_nch);
}

int setup_ddc_common(gsdr_demod *h, int F, int M, unsigned rate,
                     const std::vector<long long> &tone, int max_nblk, bool allow_flat) {
    h->ddc.F = F;
    h->ddc.M = M;
    h->ddc.nco_rate = rate;
    if (h->ddc.channels <= 0) h->ddc.channels = h->N;
    h->ddc.Npad = ((h->ddc.channels + 63) / 64) * 64;
    h->ddc.TW = h->ddc.Npad / 64;
    // the engine's kernel, its sub-block length and the grid it is sized for: ddc_plan.h
    h->ddc.flat = gsdr::ddc_flat_takes(F, allow_flat, h->sw);
    const gsdr::DdcBlocking b = gsdr::ddc_blocking(h->ddc.flat, M, h->sw);
    h->ddc.K = b.K;
    h->ddc.pad = b.pad;
    h->ddc.R = b.R;
    h->ddc.simds = device_cus() * 4;
    h->ddc.target_waves = gsdr::ddc_target_waves(h->ddc.simds, h->ddc.flat, h->sw);
    h->ddc.tails_nch = gsdr::ddc_tails_nch(F, max_nblk, h->ddc.target_waves, h->ddc.TW, h->sw.ddc_nch);
    h->ddc.waves_ratio = 1.3;
    h->ddc.nch_max = pick_chunks(h, max_nblk);
    if (build_nco_tables(h, tone, rate)) return -1;
    if (upload_taps_transposed(h)) return -1;
    const size_t tail_elems = (size_t)(h->ddc.tails_nch + 1) * (size_t)(F > 1 ? F - 1 : 1) * h->ddc.Npad;
    HIPCHK(h, h->ddc.d_tails.alloc_zeroed(tail_elems));
    return 0;
}

// What every launch of the VALU kernels of this handle carries: the tables, the launch switches and the fields of the
// shape that do not change from call to call.  The caller adds the buffers, the blocks and chunks of the call and
// finish_shape().
DdcLaunch ddc_launch_of(const gsdr_demod *h) {
    DdcLaunch a{};
    a.taps_t = h->ddc.d_taps_t;
    a.taps_p = h->ddc.d_taps_p;
    a.btab = h->ddc.d_btab;
    a.wk = h->ddc.d_wk;
    a.wrem = h->ddc.d_wrem;
    a.fmod = h->ddc.d_fmod;
    a.tails = h->ddc.d_tails;
    a.tails_nch = h->ddc.tails_nch;
    a.lds_bytes = h->sw.ddc_lds;
    a.sh.N = h->ddc.channels;
    a.sh.Npad = h->ddc.Npad;
    a.sh.TW = h->ddc.TW;
    a.sh.rate = h->ddc.nco_rate;
    a.sh.prefetch = h->sw.ddc_prefetch;
    return a;
}

// fields of DdcShape the kernels derive nothing from on the device
void finish_shape(DdcShape &sh) {
    sh.cbase = sh.nblk / (sh.nch > 0 ? sh.nch : 1);
    sh.crem = sh.nblk % (sh.nch > 0 ? sh.nch : 1);
    sh.rate_magic = 0xffffffffffffffffULL / sh.rate;
    sh.inv_rate = 1.0 / (double)sh.rate;
    sh.m_mod_rate = (unsigned)sh.M % sh.rate;
}

// Tables and fixed shape of ddc_mfma_kernel.  `direct`: rows reach F-1 blocks
// back into the previous buffer (raw-sample carry); otherwise (TONES/NOISE) row o
// starts at block o of the raw window.  max_rows: the most rows a call puts out; t_max: the longest logical stream
// [carry | buffer] of a call (TONES: the raw window as allocated).
int setup_mfma(gsdr_demod *h, bool direct, const std::vector<long long> &tone, long long max_rows, long long t_max) {
    const int F = h->ddc.F, M = h->ddc.M;
    const unsigned rate = h->ddc.nco_rate;
    const gsdr::MfmaTile tile = gsdr::mfma_tile(h->sw);
    h->mx.mf_TT = tile.TT;
    h->mx.mf_PK = tile.PK;
    h->mx.mf_W = tile.W;
    h->mx.mf_kind = tile.kind;
    gsdr::MfmaPlan pl{};
    pl.TT = h->mx.mf_TT;
    pl.PK = h->mx.mf_PK;
    pl.M = M;
    pl.MF = M * F;
    pl.nk8 = (pl.MF + 7) / 8;
    pl.rate = rate;
    pl.x16 = h->mx.mf_kind == gsdr::MfmaKernel::AsmRing16 || h->mx.mf_kind == gsdr::MfmaKernel::AsmRing16W8;
    const int nt32 = (h->ddc.channels + 31) / 32;
    pl.ntg = (nt32 + pl.TT - 1) / pl.TT;
    std::vector<unsigned> fmod_in(h->ddc.channels);
    for (int n = 0; n < h->ddc.channels; ++n) fmod_in[n] = mod_rate(tone[n], rate);
    std::vector<uint4> bfrag;
    std::vector<float2> ptab, dtab;
    std::vector<float> taps;
    std::vector<unsigned> fmod;
    float unscale = 1.f;
    gsdr::mfma_build_tables(pl, fmod_in, h->window.data(), bfrag, ptab, dtab, taps, fmod, unscale);
    HIPCHK(h, h->mx.d_bfrag.upload(bfrag));
    HIPCHK(h, h->mx.d_ptab.upload(ptab));
    HIPCHK(h, h->mx.d_dtab.upload(dtab));
    HIPCHK(h, h->mx.d_mtaps.upload(taps));
    HIPCHK(h, h->mx.d_mfmod.upload(fmod));
    {
        // maxima per segment of the call's logical stream [carry | buffer] (TONES: the raw window, allocated
        // 2 * nfft * batching long): a segment is one block of M samples, several when blocks are short
        h->mx.seg_k = M >= 64 ? 1 : (64 + M - 1) / M;
        const long long seg_len = (long long)h->mx.seg_k * M;
        h->mx.nseg_alloc = (int)((t_max + seg_len - 1) / seg_len) + 2;
        HIPCHK(h, h->mx.d_segmax.alloc_zeroed((size_t)kScaleSlots * h->mx.nseg_alloc));
    }
    gsdr::MfmaShape &sh = h->mx.mf;
    sh.N = h->ddc.channels;
    sh.NT32 = pl.ntg * pl.TT;
    sh.ntg = pl.ntg;
    sh.ntq = (pl.ntg + h->mx.mf_W - 1) / h->mx.mf_W;
    sh.M = M;
    sh.MF = pl.MF;
    sh.F = F;
    sh.nk8 = pl.nk8;
    sh.woff = direct ? -(F - 1) : 0;
    sh.carry_len = direct ? (F - 1) * M : 0;
    sh.rate = rate;
    sh.rate_magic = 0xffffffffffffffffULL / rate;
    sh.inv_rate = 1.0 / (double)rate;
    sh.m_mod_rate = (unsigned)M % rate;
    sh.unscale = unscale;
#ifdef GSDR_TIMING_BUILD
    sh.timing_mode = h->sw.mfma_timing;   // ablation builds only (scratch/), never shipped
#else
    sh.timing_mode = 0;
#endif
    sh.rt = h->sw.mfma_rt;   // 0: chosen per launch in enqueue_mfma
    if (direct) {
        // row tile 0 and the last row tile read from copies with the carry in front
        // and zeros behind (sizes: ddc_mfma_kernel's reach, 8*nk8 samples per row)
        const size_t reach = (size_t)((pl.nk8 + pl.PK / 8 - 1) / (pl.PK / 8)) * pl.PK;   // whole phasor blocks
        const size_t head_n = (size_t)sh.carry_len + 32u * (size_t)M + reach + 8;
        const size_t tail_n = (size_t)(32 + F) * (size_t)M + reach + 8;
        for (int i = 0; i < kStageSets; ++i) {
            HIPCHK(h, h->mx.d_head[i].alloc_zeroed(head_n));
            HIPCHK(h, h->mx.d_tail[i].alloc_zeroed(tail_n));
        }
    }
    // pre-converted operands: allocated when a launch of this handle may use them (the largest row count, in an
    // overlapped entry), up to 8 GiB of images
    if (h->mx.mf_kind == gsdr::MfmaKernel::AsmRing16) {
        const long long ngt_max = (max_rows + 31) / 32;
        const long long nhi = (pl.nk8 + 3) / 4;
        const bool images = gsdr::prec_pays(h->ddc.simds, ngt_max, sh.ntq, pl.nk8, /*overlap=*/true, h->sw);
        const gsdr::ProductLoop *row = images ? gsdr::product_loop(gsdr::product_loop_chosen(nhi, max_rows, pl.ntg, h->sw)) : nullptr;
        // uint4 per image set: 12 / 8 KiB per block, folded 16 KiB per pair of blocks
        const size_t img_n = row ? (size_t)ngt_max * (size_t)((nhi + row->image_blocks - 1) / row->image_blocks) * row->image_uint4 : 0;
        if (img_n * sizeof(uint4) > (size_t)8 << 30) row = nullptr;
        for (int i = 0; i < kStageSets && row; ++i) HIPCHK(h, h->mx.d_img[i].alloc(img_n));
        h->mx.prec = row != nullptr;
        h->mx.loop = row && row->build_tables ? row : nullptr;      // AsmRing16P's row: chosen per launch
        if (h->mx.loop) {
            std::vector<uint4> bfrag3;
            std::vector<float4> ptab3;
            row->build_tables(pl, fmod, bfrag3, ptab3);
            HIPCHK(h, h->mx.d_bfrag3.upload(bfrag3));
            HIPCHK(h, h->mx.d_ptab3.upload(ptab3));
        }
    }
    h->mx.on = true;
    h->kernel_name = gsdr::ddc_mfma_kernel_name(h->mx.loop ? h->mx.loop->kind : h->mx.mf_kind);
    return 0;
}

// Grid size of the DDC launch, measured instead of guessed: times the real
// launch (ddc kernel + fixup) on scratch buffers for a few grid/resident ratios
// and keeps the fastest.  Runs once in create(); GSDR_DDC_AUTOTUNE=0 keeps 1.3.
int autotune_chunks(gsdr_demod *h, int nblk) {
    h->ddc.waves_ratio = 1.3;
    if (!h->ddc.flat || h->sw.ddc_nch > 0 || !h->sw.ddc_autotune || nblk < 1) {
        h->ddc.nch_max = pick_chunks(h, nblk);
        return 0;
    }
    const size_t n_in = (size_t)nblk * h->ddc.M + h->ddc.pad + 8;
    const size_t n_out = (size_t)nblk * h->ddc.channels;
    gsdr::DevBuf<float2> x, y;
    HIPCHK(h, x.alloc(n_in));
    if (y.alloc(n_out) != hipSuccess) {
        h->err = "autotune scratch allocation failed";
        return -1;
    }
    (void)hipMemset(x, 0x3c, n_in * sizeof(float2));  // 0.0115f everywhere: finite, non-zero
    gsdr::Event e0, e1;
    (void)hipEventCreate(e0.out());
    (void)hipEventCreate(e1.out());
    const double cand[] = {0.8, 1.0, 1.3, 1.7};
    double best_ms = 1e30, best_ratio = 1.3;
    int rc = 0;
    for (double r : cand) {
        h->ddc.waves_ratio = r;
        DdcLaunch a = ddc_launch_of(h);
        a.x = x;
        a.out = y;
        a.pipe = true;
        a.sh.M = h->ddc.M;
        a.sh.nblk = nblk;
        a.sh.nch = pick_chunks(h, nblk);
        a.sh.xlast = (long long)nblk * h->ddc.M + h->ddc.pad - 4;
        finish_shape(a.sh);
        float ms = 0.f;
        for (int it = 0; it < 4 && !rc; ++it) {  // first iteration warms up
            if (it == 1) rc |= hipEventRecord(e0, h->stream) != hipSuccess;
            rc |= gsdr::launch_ddc(h->ddc.F, h->ddc.K, a, h->stream, nullptr) != hipSuccess;
        }
        rc |= hipEventRecord(e1, h->stream) != hipSuccess;
        rc |= hipEventSynchronize(e1) != hipSuccess;
        if (rc || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) {
            rc = 1;
            break;
        }
        if (ms < best_ms) {
            best_ms = ms;
            best_ratio = r;
        }
    }
    if (rc) {
        h->err = "autotune launch failed";
        return -1;
    }
    h->ddc.waves_ratio = best_ratio;
    h->ddc.nch_max = pick_chunks(h, nblk);
    return 0;
}

int enqueue_mfma(gsdr_demod *h, const float2 *in, float2 *raw, long long raw_new0, long long nx,
                 int nout, unsigned idx_base, float2 *out, hipStream_t st, const float2 *spare_src,
                 long long spare_n) {
    // tables of segment maxima: this call's, and the one the staging pass clears for the next call.
    // kScaleSlots of them, so that the pass of call j (filling table j, clearing table j+1) leaves
    // alone what the main kernels of the calls still in flight read (tables j-1 .. j-kPipeStreams+1).
    const int cur = (int)(h->mx.call_no % kScaleSlots), next = (int)((h->mx.call_no + 1) % kScaleSlots);
    const int hs = (int)(h->mx.call_no % kStageSets), hs_next = (int)((h->mx.call_no + 1) % kStageSets);
    gsdr::MfmaLaunch a{};
    a.sh = h->mx.mf;
    a.sh.nout = nout;
    a.sh.ngt = (nout + 31) / 32;
    a.sh.nx = nx;
    a.sh.idx_base = idx_base;
    a.sh.seg_k = h->mx.seg_k;
    gsdr::StageLaunch sg{};
    sg.x = in;
    sg.n = h->L;
    sg.seg = h->mx.d_segmax + (size_t)cur * h->mx.nseg_alloc;
    sg.seg_clear = h->mx.d_segmax + (size_t)next * h->mx.nseg_alloc;
    sg.nseg_alloc = h->mx.nseg_alloc;
    sg.seg_len = (long long)h->mx.seg_k * a.sh.M;
    a.sh.rt = gsdr::mfma_row_tiles(h->mx.loop != nullptr, h->pl.overlap, a.sh.nk8, a.sh.ngt, a.sh.ntq, h->sw);
    h->mx.last_rt = a.sh.rt;
    if (raw) {
        // TONES: one pass brings the carried samples to the front of this call's raw window,
        // appends the buffer and takes its maximum; every row reads the window itself
        // (allocated twice as long as it gets)
        if (spare_n != raw_new0) {
            h->err = "raw window bookkeeping out of step";
            return -1;
        }
        sg.b = spare_src;
        sg.nb = spare_n;
        sg.b_dst = raw;
        sg.head_cur = raw + raw_new0;
        sg.head_n = h->L;
        sg.tail0 = h->L;
        HIPCHK(h, gsdr::launch_absmax(sg, st));
        if (record_staged(h, st)) return -1;
        a.x = a.head = a.tail = raw;
        a.sh.tail0 = 0;
    } else {
        const int cl = a.sh.carry_len;
        const long long t0 = a.sh.ngt > 1 ? (long long)(32 * (a.sh.ngt - 1) + a.sh.woff) * a.sh.M : h->L;
        const int ks = h->mx.mf_PK / 8;
        long long head_n = 32LL * a.sh.M + (long long)((a.sh.nk8 + ks - 1) / ks) * h->mx.mf_PK + 8;
        if (head_n > h->L) head_n = h->L;
        sg.b = h->mx.d_head[hs];       // the carry: the last cl samples of the previous buffer, left there by its pass
        sg.nb = cl;
        sg.head_cur = h->mx.d_head[hs];
        sg.head_n = head_n;
        sg.head_next = h->mx.d_head[hs_next];
        sg.carry_len = cl;
        sg.tail = h->mx.d_tail[hs];
        sg.tail0 = t0;
        HIPCHK(h, gsdr::launch_absmax(sg, st));
        if (record_staged(h, st)) return -1;
        a.x = in;
        a.head = h->mx.d_head[hs];
        a.tail = h->mx.d_tail[hs];
        a.sh.tail0 = t0;
    }
    a.taps = h->mx.d_mtaps;
    a.bfrag = h->mx.d_bfrag;
    a.ptab = h->mx.d_ptab;
    a.dtab = h->mx.d_dtab;
    a.fmod = h->mx.d_mfmod;
    a.segmax = sg.seg;
    a.out = out;
    hipEvent_t stop = nullptr;
    if (record_begin(h, st, &stop)) return -1;
    // the kernel of this launch (ddc_plan.h): the handle's product loop, or the main loop as its row count asks
    gsdr::MfmaKernel kind;
    if (h->mx.loop) {
        // whatever the entry, the stream pattern or the row count: one arithmetic per handle
        kind = h->mx.loop->kind;
        a.bfrag3 = h->mx.d_bfrag3;
        a.ptab3 = h->mx.d_ptab3;
    } else {
        kind = gsdr::mfma_launch_kernel(h->mx.mf_kind, h->mx.prec, a.sh.rt, h->ddc.simds, a.sh.ngt, a.sh.ntq, a.sh.ntg, a.sh.nk8, h->pl.overlap, h->sw);
    }
    if (h->mx.loop || kind == gsdr::MfmaKernel::AsmRing16P) a.img = h->mx.d_img[hs];
    h->kernel_name = gsdr::ddc_mfma_kernel_name(kind);
    HIPCHK(h, gsdr::launch_ddc_mfma(kind, h->mx.mf_TT, h->mx.mf_PK, h->mx.mf_W, a, st));
    if (stop) HIPCHK(h, hipEventRecord(stop, st));
    h->mx.call_no++;
    return 0;
}

// ref: process_direct, cpp/USRP_demodulator.cpp:400-464
int enqueue_direct(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st) {
    long long ret;
    hipEvent_t stop = nullptr;
    if (h->decim > 0 && h->mx.on) {
        const unsigned rate = h->ddc.nco_rate;
        const unsigned back = (unsigned)(((unsigned long long)(h->ddc.F - 1) * h->ddc.M) % rate);
        const unsigned idx_base = (unsigned)((h->ddc.idx + rate - back) % rate);
        if (enqueue_mfma(h, in, nullptr, 0, h->L, (int)(h->L / h->ddc.M), idx_base, out, st)) return -1;
        ret = (long long)h->N * (h->L / h->ddc.M);               // :459
    } else if (h->decim > 0) {
        DdcLaunch a = ddc_launch_of(h);
        a.x = in;
        a.out = out;
        a.pipe = h->ddc.flat && h->L >= 4;
        a.few = h->ddc.few;
        a.carry_in = h->ddc.d_carry[h->ddc.parity];
        a.carry_out = h->ddc.d_carry[h->ddc.parity ^ 1];
        a.sh.idx0 = h->ddc.idx;
        a.sh.M = h->ddc.M;
        a.sh.nblk = (int)(h->L / h->ddc.M);
        a.sh.nch = h->ddc.nch_max;
        a.sh.xlast = h->L - 4;
        if (a.pipe && h->ddc.pad > 0) {
            // the last sub-block of a block reads `pad` samples past it (zero taps);
            // behind the last block that would leave the caller's buffer
            HIPCHK(h, hipMemcpyAsync(h->ddc.d_stage, in, (size_t)h->L * sizeof(float2),
                                     hipMemcpyDeviceToDevice, st));
            a.x = h->ddc.d_stage;
            a.sh.xlast = h->L + h->ddc.pad - 4;
        }
        finish_shape(a.sh);
        if (record_begin(h, st, &stop)) return -1;
        HIPCHK(h, gsdr::launch_ddc(h->ddc.F, h->ddc.K, a, st, stop));
        h->ddc.parity ^= 1;
        ret = (long long)h->N * (h->L / h->ddc.M);               // :459
    } else {
        DdcLaunch a = ddc_launch_of(h);
        a.x = in;
        a.out = out;
        a.sh.idx0 = h->ddc.idx;
        a.sh.M = h->ddc.K;
        a.sh.total = h->L;
        a.sh.nblk = (int)((h->L + h->ddc.K - 1) / h->ddc.K);
        long long nch = h->ddc.target_waves / h->ddc.TW;
        if (nch < 1) nch = 1;
        if (nch > a.sh.nblk) nch = a.sh.nblk;
        a.sh.nch = (int)nch;
        finish_shape(a.sh);
        if (record_begin(h, st, &stop)) return -1;
        HIPCHK(h, gsdr::launch_mix(h->ddc.K, a, h->sw.mix_few, st));
        if (stop) HIPCHK(h, hipEventRecord(stop, st));
        ret = (long long)h->N * h->L;                        // :457
    }
    h->ddc.idx = (h->ddc.idx + (unsigned long long)h->L) % h->ddc.nco_rate;  // :437-440
    return (int)ret;
}

// ref: :59-119
int setup_direct(gsdr_demod *h, const gsdr_param_c *p) {
    const gsdr::Switches &sw = h->sw;
    if (p->rate <= 0) return refuse(h, "rate must be positive");
    if (!(p->n_freq >= h->N && p->freq)) return refuse(h, "DIRECT needs one frequency per wave_type entry");
    const std::vector<long long> tone(p->freq, p->freq + h->N);
    if (h->decim <= 0) {
        // undecimated: only the NCO tables are needed
        h->ddc.F = 1;
        h->ddc.M = 1;
        h->window.assign(1, 1.f);
        if (setup_ddc_common(h, 1, 1, (unsigned)p->rate, tone, 1, /*allow_flat=*/false)) return -1;
        h->kernel_name = gsdr::mix_kernel_name(h->N, h->ddc.TW, h->L, h->ddc.K, sw.mix_few);
        h->capacity = (long long)h->N * h->L;
        return 0;
    }
    if (h->L % h->decim != 0) return refuse(h, "buffer_len must be a multiple of decim (ref: fir.cu:20)");
    if (p->pf_average < 1 || p->pf_average > kMaxF) return refuse(h, "pf_average must be in [1,8] for DIRECT with decimation");
    if (h->decim > 0x7fffffffLL / p->pf_average) return refuse(h, "decim*pf_average overflows");
    const int F = (int)p->pf_average, M = (int)h->decim;
    h->window.resize((size_t)M * F);
    // ref: :99 taps, cut-off 0.75/(2*decim) narrowed to float
    gsdr_make_sinc_window(M * F, (float)(0.75 / (M * 2)), h->window.data());
    if (setup_ddc_common(h, F, M, (unsigned)p->rate, tone, (int)(h->L / M))) return -1;
    if (h->ddc.flat && h->ddc.pad > 0 && h->ddc.d_stage.alloc_zeroed((size_t)h->L + h->ddc.pad) != hipSuccess)
        return refuse(h, "staging allocation failed");
    h->kernel_name = h->ddc.flat ? gsdr::ddc_flat_kernel_name() : gsdr::ddc_kernel_name();
    for (auto &c : h->ddc.d_carry)
        if (c.alloc_zeroed((size_t)(F > 1 ? F - 1 : 1) * h->ddc.Npad) != hipSuccess) return refuse(h, "carry allocation failed");
    const gsdr::DdcEngine engine = gsdr::ddc_direct_engine(h->decim, h->N, M, F, h->L, sw);
    h->ddc.few = engine == gsdr::DdcEngine::Few;
    if (h->ddc.few) h->kernel_name = gsdr::ddc_few_kernel_name();
    if (engine == gsdr::DdcEngine::Mfma && setup_mfma(h, /*direct=*/true, tone, h->L / M, (long long)(F - 1) * M + h->L)) return -1;
    if (!h->mx.on && autotune_chunks(h, (int)(h->L / M))) return -1;
    h->capacity = (long long)h->N * (h->L / M);
    return 0;
}

void describe_mfma(const gsdr_demod *h, std::string &s) {
    s += ", \"row_tiles_per_workgroup\": " + std::to_string(h->mx.on ? h->mx.last_rt : 0);
    // every other handle reports what the four-product loop's row says
    const gsdr::ProductLoop &pr = h->mx.on && h->mx.loop ? *h->mx.loop : *gsdr::product_loop(gsdr::MfmaKernel::AsmRing16P);
    s += ", \"complex_mac\": " + std::to_string(pr.complex_mac);
    s += ", \"complex_mac_min_blocks\": " + std::to_string(gsdr::kMac3MinBlocks);
    s += ", \"rotation_blocks\": " + std::to_string(pr.rotation_blocks);
    s += ", \"rotation_min_blocks\": " + std::to_string(gsdr::kRot2MinBlocks);
    s += ", \"fold\": " + std::to_string(pr.fold);
    s += ", \"fold_min_blocks\": " + std::to_string(gsdr::kFoldMinBlocks);
    s += ", \"fold_products\": " + std::to_string(pr.fold_products);
    s += ", \"wave_tones\": " + std::to_string(pr.wave_tones);
    s += ", \"span_samples\": " + std::to_string(pr.image_blocks == 4 ? 128 : 64);
    s += ", \"span128_min_blocks\": " + std::to_string(gsdr::kSpan128MinBlocks);
}

}  // namespace rx
}  // namespace gsdr
