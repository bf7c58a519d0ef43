// demod_pfb.cpp -- TONES and NOISE: the polyphase filter bank through one of three engines -- a frame per workgroup
// inside the LDS (pfb_plan.h), the FFT stages through memory, or every bin as a tone of the DDC kernels
// (demod_ddc.cpp) -- and the mean of consecutive frames behind them.
//
// "ref:" citations name the reference's files, as in demod.cpp.
#include "demod_state.h"

namespace gsdr {
namespace rx {

namespace {

// What closes a TONES / NOISE call of cb frames: the host's frame bookkeeping moves on (:552 / :644) and the call's
// length is returned -- cb rows of every channel (:546 TONES; copy_size :638 NOISE: every bin).  windows: the engine
// keeps the raw windows (d_win), and the unconsumed samples of this one go to the front of the next call's
// (:504-509, :590-596); the LDS kernels keep none.
int close_pfb_call(gsdr_demod *h, int cb, bool windows) {
    if (windows) {
        h->pfb.prev_spare_begin = h->pfb.bh.spare_begin;
        h->pfb.prev_spare_samples = h->pfb.bh.spare_samples > 0 ? h->pfb.bh.spare_samples : 0;
    }
    h->pfb.win_seq++;
    gsdr_buffer_helper_update(&h->pfb.bh);
    return h->ddc.channels * cb;
}

// ref: process_pfb_spec (decim == 0), cpp/USRP_demodulator.cpp:568-649: polyphase filter, forward FFT of
// every complete frame, all bins kept.  Frame bookkeeping and the carry of the unconsumed samples
// are those of enqueue_pfb (the raw windows rotate, see there).
int enqueue_noise_fft(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st) {
    const int cb = h->pfb.bh.current_batch;
    float2 *win = h->pfb.d_win[h->pfb.win_seq % kStageSets];
    if (h->pfb.prev_spare_samples > 0)   // :590-596 of the previous call
        HIPCHK(h, hipMemcpyAsync(win, h->pfb.d_win[(h->pfb.win_seq + kStageSets - 1) % kStageSets] + h->pfb.prev_spare_begin,
                                 (size_t)h->pfb.prev_spare_samples * sizeof(float2), hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipMemcpyAsync(win + h->pfb.bh.new_0, in, (size_t)h->L * sizeof(float2), hipMemcpyDeviceToDevice, st));  // :573-577
    if (cb > 0) {
        hipEvent_t stop = nullptr;
        if (record_begin(h, st, &stop)) return -1;
        HIPCHK(h, gsdr::launch_pfb_filter(win, h->pfb.d_fft_win, h->pfb.nfft, h->pfb.taps, cb, h->pfb.d_fft_a, st));   // :580
        if (h->pfb.d_fft_c) {                                                                            // TONES: :531-540
            HIPCHK(h, gsdr::fft_forward(h->pfb.fft, h->pfb.d_fft_a, h->pfb.d_fft_c, h->pfb.d_fft_b, cb, st));
            HIPCHK(h, gsdr::launch_pfb_select(h->pfb.d_fft_c, h->pfb.nfft, cb, h->pfb.d_sel, h->ddc.channels, out, st));
        } else {
            HIPCHK(h, gsdr::fft_forward(h->pfb.fft, h->pfb.d_fft_a, out, h->pfb.d_fft_b, cb, st));               // :583
        }
        if (stop) HIPCHK(h, hipEventRecord(stop, st));
    }
    return close_pfb_call(h, cb, /*windows=*/true);
}

// ref: process_pfb (:486-565) and process_pfb_spec (:568-649), decim == 0: one launch, a frame per
// workgroup.  The logical raw_input is [what the previous call left over | the new buffer]; nothing is
// staged: the kernel reads both parts in place and writes this call's leftovers (:504-509, :590-596)
// into the other carry buffer.  h->kernel_name becomes the kernel launched.
int enqueue_pfb_lds(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st) {
    const int cb = h->pfb.bh.current_batch;
    const float2 *carry = h->pfb.d_carry[h->pfb.win_seq % kStageSets];
    float2 *carry_out = h->pfb.d_carry[(h->pfb.win_seq + 1) % kStageSets];
    const int spare_n = h->pfb.bh.spare_samples > 0 ? h->pfb.bh.spare_samples : 0;
    if (spare_n > h->pfb.nfft * h->pfb.taps) {
        h->err = "PFB carry larger than a window";
        return -1;
    }
    const int *sel = h->mode == GSDR_NOISE ? nullptr : h->pfb.d_sel;
    const long long wlen = (long long)h->pfb.bh.new_0 + h->L;
    const gsdr::FftPlan *blue = h->pfb.blue ? &h->pfb.fft : nullptr;
    const float2 *tw = h->pfb.blue ? h->pfb.fft.d_tw : h->pfb.d_tw;
    hipEvent_t stop = nullptr;
    if (record_begin(h, st, &stop)) return -1;
    HIPCHK(h, gsdr::launch_pfb_lds(carry, h->pfb.bh.new_0, in, h->pfb.d_fft_win, tw, h->pfb.nfft, h->pfb.taps, cb, sel, h->ddc.channels, out,
                                   carry_out, h->pfb.bh.spare_begin, spare_n, wlen, st, blue, h->sw, &h->kernel_name, &h->pfb.last));
    {
        const gsdr::PfbChoice &c = h->pfb.last;
        h->pfb.last_frames = cb;
        (c.cu ? h->pfb.calls_cu : h->pfb.calls_lds)++;
        if (c.cu && c.direct >= 0 && c.direct <= 5) h->pfb.calls_direct[c.direct]++;
        if (c.cu && c.teams) h->pfb.calls_teams++;
        if (c.G >= 2) h->pfb.calls_runs++;
        if (cb > 0 && c.G >= 1 && cb % c.G != 0) h->pfb.calls_short++;
    }
    if (stop) HIPCHK(h, hipEventRecord(stop, st));
    return close_pfb_call(h, cb, /*windows=*/false);      // the kernel has written the leftovers into the other carry buffer
}

}  // namespace

// ref: process_pfb (decim == 0 branch), cpp/USRP_demodulator.cpp:486-565
int enqueue_pfb(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st) {
    if (h->pfb.lds) return enqueue_pfb_lds(h, in, out, st);
    if (h->pfb.noise_fft) return enqueue_noise_fft(h, in, out, st);
    // :491-495  new buffer goes after the carried samples
    const int cb = h->pfb.bh.current_batch;
    float2 *win = h->pfb.d_win[h->pfb.win_seq % kStageSets];
    const float2 *spare = h->pfb.prev_spare_samples > 0
                              ? h->pfb.d_win[(h->pfb.win_seq + kStageSets - 1) % kStageSets] + h->pfb.prev_spare_begin
                              : nullptr;
    if (!(cb > 0 && h->mx.on)) {
        // :504-509 of the previous call (carry the unconsumed samples to the front), then :491-495
        if (spare)
            HIPCHK(h, hipMemcpyAsync(win, spare, (size_t)h->pfb.prev_spare_samples * sizeof(float2),
                                     hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemcpyAsync(win + h->pfb.bh.new_0, in, (size_t)h->L * sizeof(float2),
                                 hipMemcpyDeviceToDevice, st));
        if (record_staged(h, st)) return -1;
    }
    if (cb > 0 && h->mx.on) {
        if (enqueue_mfma(h, in, win, h->pfb.bh.new_0, (long long)(cb + h->ddc.F - 1) * h->ddc.M, cb, 0u, out, st, spare,
                         h->pfb.prev_spare_samples))
            return -1;
    } else if (cb > 0) {
        DdcLaunch a = ddc_launch_of(h);
        a.x = win;
        a.out = out;
        a.carry_in = nullptr;   // frames never reach back before raw_input[0]
        a.carry_out = nullptr;
        a.sh.idx0 = 0;          // raw_input[0] is always on the frame grid
        a.sh.M = h->ddc.M;
        a.sh.nblk = cb + h->ddc.F - 1;  // frame r spans blocks r .. r+F-1
        a.pipe = h->ddc.flat;
        a.sh.xlast = (long long)a.sh.nblk * h->ddc.M + h->ddc.pad - 4;  // a window is allocated twice as long
        a.sh.g_off = h->ddc.F - 1;      // DDC output G <-> frame r = G-(F-1)
        const int nch = pick_chunks(h, a.sh.nblk);
        a.sh.nch = nch;
        finish_shape(a.sh);
        hipEvent_t stop = nullptr;
        if (record_begin(h, st, &stop)) return -1;
        HIPCHK(h, gsdr::launch_ddc(h->ddc.F, h->ddc.K, a, st, stop));
    }
    return close_pfb_call(h, cb, /*windows=*/true);
}

// TONES / NOISE with gsdr_demod_set_frame_average(k > 1): the PFB writes its frames to the handle's frame buffer, and
// pfb_average_kernel behind it on the same stream writes the groups that complete to `out` and the sums of the open
// group to the other accumulator.  The bookkeeping is host integers, so the returned length is known at once.  The
// chain of accumulators is ordered like the raw-window carry: by the stream, and by join_streams when it changes.
int enqueue_pfb_average(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st) {
    const int cb = h->pfb.bh.current_batch;
    const size_t ev0 = h->prof.ev_used;
    if (enqueue_pfb(h, in, h->pfb.d_avg_frames, st) < 0) return -1;
    if (cb <= 0) return 0;
    const long long rows = ((long long)h->pfb.avg_count + cb) / h->pfb.avg_k;
    HIPCHK(h, gsdr::launch_pfb_average(h->pfb.d_avg_frames, cb, h->ddc.channels, h->pfb.avg_k, h->pfb.avg_kind, h->pfb.avg_count,
                                       h->pfb.d_avg_acc[h->pfb.avg_seq % 2], h->pfb.d_avg_acc[(h->pfb.avg_seq + 1) % 2], out, st));
    // the profile pair of this call (if it is a timed one) closes behind the averaging: recorded again, an event keeps the later point
    if (h->prof.ev_used > ev0) HIPCHK(h, hipEventRecord(h->prof.ev_pool[h->prof.ev_used - 1].second, st));
    h->pfb.avg_seq++;
    h->pfb.avg_count = (int)(((long long)h->pfb.avg_count + cb) % h->pfb.avg_k);
    return (int)(rows * h->ddc.channels);
}

namespace {

// TONES / NOISE, a frame per workgroup -- polyphase filter, transform inside the LDS, bin selection: the
// reference's own algorithm (:486-565, :568-649) at one read of the window and one write of the selected bins per
// buffer.  blue_m > 0: through Bluestein's identity at that padded length.
int setup_pfb_lds(gsdr_demod *h, bool noise, int F, const std::vector<long long> &tone, long long blue_m) {
    h->pfb.lds = true;
    h->pfb.blue = blue_m > 0;
    h->pfb.taps = F;
    std::vector<float2> tw((size_t)h->pfb.nfft);
    for (int k = 0; k < h->pfb.nfft; ++k) {
        const double a = -2.0 * M_PI * (double)k / (double)h->pfb.nfft;
        tw[(size_t)k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    const std::vector<int> sel(tone.begin(), tone.end());
    bool ok = h->pfb.d_tw.upload(tw) == hipSuccess && h->pfb.d_fft_win.upload(h->window) == hipSuccess &&
              (noise || h->pfb.d_sel.upload(sel) == hipSuccess);
    // Bluestein: the chirp, its transform and the twiddles of length m (fft_plan_build makes exactly these)
    if (ok && h->pfb.blue) ok = gsdr::fft_plan_build(h->pfb.fft, h->pfb.nfft) == 0 && h->pfb.fft.m == (int)blue_m;
    for (int i = 0; i < kStageSets && ok; ++i) ok = h->pfb.d_carry[i].alloc_zeroed((size_t)h->pfb.nfft * F + 8) == hipSuccess;
    if (!ok) return refuse(h, "PFB allocation failed");
    // the kernel of a call of L / nfft frames (each launch reports its own, enqueue_pfb_lds)
    h->kernel_name = gsdr::pfb_kernel_name(gsdr::pfb_choose(h->pfb.nfft, F, h->pfb.blue ? h->pfb.fft.m : 0, h->pfb.blue ? h->pfb.fft.n_radices : 0,
                                                            h->pfb.blue ? h->pfb.fft.radices : nullptr, (int)(h->L / h->pfb.nfft),
                                                            h->ddc.channels, device_cus(), h->sw));
    return 0;
}

// Frames the LDS kernel does not take: the polyphase filter and one launch per radix stage through memory (§4.5) --
// NOISE keeps every bin, TONES (tones_global) picks its bins out of a scratch spectrum.  For TONES this replaces one
// DDC per bin when the frame is long (above 8192 points a frame is a window of 32 768+ samples: the DDC rows become
// thousand-block loops on a handful of workgroups)
int setup_pfb_global(gsdr_demod *h, bool tones_global, int F, const std::vector<long long> &tone) {
    h->pfb.noise_fft = true;
    h->pfb.taps = F;
    h->kernel_name = gsdr::fft_kernel_name();
    if (tones_global) {
        const std::vector<int> sel(tone.begin(), tone.end());
        if (h->pfb.d_sel.upload(sel) != hipSuccess || h->pfb.d_fft_c.alloc((size_t)h->pfb.nfft * (size_t)h->pfb.batching) != hipSuccess)
            return refuse(h, "TONES allocation failed");
    }
    if (gsdr::fft_plan_build(h->pfb.fft, h->pfb.nfft) != 0) return refuse(h, "cannot plan an FFT of fft_tones points");
    const size_t len = (size_t)(h->pfb.fft.m > h->pfb.nfft ? h->pfb.fft.m : h->pfb.nfft) * (size_t)h->pfb.batching;
    bool ok = h->pfb.d_fft_a.alloc(len) == hipSuccess && h->pfb.d_fft_b.alloc(len) == hipSuccess &&
              h->pfb.d_fft_win.upload(h->window) == hipSuccess;
    for (int i = 0; i < kStageSets && ok; ++i) ok = h->pfb.d_win[i].alloc_zeroed((size_t)h->pfb.nfft * h->pfb.batching * 2) == hipSuccess;
    return ok ? 0 : refuse(h, "NOISE allocation failed");
}

// Every selected bin as a tone of the DDC kernels (GSDR_PFB_LDS=0 with GSDR_TONES_FFT=0 / GSDR_NOISE_FFT=0)
int setup_pfb_ddc(gsdr_demod *h, int F, const std::vector<long long> &tone) {
    const int rc = setup_ddc_common(h, F, h->pfb.nfft, (unsigned)h->pfb.nfft, tone, (int)(h->L / h->pfb.nfft) + F + 6);
    h->kernel_name = h->ddc.flat ? gsdr::ddc_flat_kernel_name() : gsdr::ddc_kernel_name();
    if (rc) return -1;
    // raw_input (:143) plus an equally long half of padding behind it, kStageSets times
    for (auto &w : h->pfb.d_win)
        if (w.alloc_zeroed((size_t)h->pfb.nfft * h->pfb.batching * 2) != hipSuccess) return refuse(h, "raw_input allocation failed");
    // every carried sample of the raw window must come from the previous buffer
    // (absmax covers this buffer and the one before)
    // and the padding behind the last window must stay inside the raw buffer's spare half
    if (h->sw.ddc_mfma && (long long)h->pfb.nfft * (F + 1) <= h->L && (long long)h->pfb.nfft * h->pfb.batching >= 40 &&
        setup_mfma(h, /*direct=*/false, tone, h->pfb.batching, 2LL * h->pfb.nfft * h->pfb.batching))
        return -1;
    if (!h->mx.on && autotune_chunks(h, (int)(h->L / h->pfb.nfft) + F - 1)) return -1;
    return 0;
}

}  // namespace

// TONES, ref: :121-175, :702-768; NOISE, ref: :264-313 (full spectrum: every FFT bin is a channel)
int setup_pfb(gsdr_demod *h, const gsdr_param_c *p) {
    const gsdr::Switches &sw = h->sw;
    const bool noise = (h->mode == GSDR_NOISE);
    if (p->rate <= 0) return refuse(h, "rate must be positive");
    if (p->fft_tones < 1) return refuse(h, "fft_tones must be >= 1");
    if (p->pf_average < 1 || p->pf_average > kMaxF) return refuse(h, "pf_average must be in [1,8] for TONES/NOISE");
    if (!(noise || (p->n_freq >= h->N && p->freq))) return refuse(h, "TONES needs one frequency per wave_type entry");
    if (h->decim > 0)
        return refuse(h, "TONES/NOISE with decim > 0 is not supported: the reference path is broken "
                         "(ref: kernels.cu:718-719,747,779, USRP_demodulator.cpp:172,516)");
    if ((long long)p->fft_tones * p->pf_average > 0x7fffffffLL) return refuse(h, "fft_tones*pf_average overflows");
    // NOISE: polyphase filter + batched FFT of every frame (fft_kernels.hip), any fft_tones.
    // GSDR_NOISE_FFT=0 evaluates every bin as a DDC tone instead (round 1's path: O(fft_tones)
    // per sample, kept for A/B runs and refused above 16384 bins)
    const bool noise_fft = noise && sw.noise_fft;
    if (noise && !noise_fft && p->fft_tones > 16384)
        return refuse(h, "NOISE without the FFT stage (GSDR_NOISE_FFT=0) supports fft_tones <= 16384");
    h->pfb.nfft = p->fft_tones;
    const int F = (int)p->pf_average;
    h->fcut = (float)(1. / (2 * h->pfb.nfft));                     // :131, :274
    h->window.resize((size_t)h->pfb.nfft * F);
    gsdr_make_sinc_window(h->pfb.nfft * F, h->fcut, h->window.data());  // :134, :277
    h->pfb.batching = gsdr_pfb_batching(h->L, h->pfb.nfft, F);         // :706
    const int n_ch = noise ? h->pfb.nfft : h->N;                   // channels of the DDC launch
    h->pfb.bins.resize(n_ch);
    if (noise) {
        for (int u = 0; u < n_ch; ++u) h->pfb.bins[u] = u;         // process_pfb_spec keeps every bin
    } else {
        gsdr_pfb_tone_bins(p->rate, h->pfb.nfft, p->freq, h->N, h->pfb.bins.data());  // :722-733
    }
    std::vector<long long> tone(n_ch);
    for (int u = 0; u < n_ch; ++u) tone[u] = h->pfb.bins[u] < 0 ? 0 : h->pfb.bins[u];
    // buffer_helper(n_tones, buffer_len, average, n_eff_tones): :159 / :301
    gsdr_buffer_helper_init(&h->pfb.bh, h->pfb.nfft, (int)h->L, F, n_ch);
    h->ddc.channels = n_ch;
    h->capacity = (long long)n_ch * h->pfb.batching;               // :147 / :288
    // The engine.  In the LDS: frames of up to 8192 points without a prime factor above 127;
    // GSDR_PFB_LDS=0, GSDR_TONES_FFT=0 (TONES only) or such a length leave TONES to the DDC
    // kernels (every selected bin as a tone) and NOISE to the global-memory FFT stages.
    int radices16[16];
    const bool direct_ok = gsdr::pfb_lds_plan(h->pfb.nfft, radices16, sw.pfb_radix8) >= 0;
    // a prime factor above 127 (or GSDR_PFB_BLUESTEIN=1: any length, for tests): Bluestein's identity inside
    // the workgroup, when a frame at the padded length m = 2^ceil(log2(2 nfft - 1)) fits the LDS
    const long long blue_m = gsdr::pfb_blue_length(h->pfb.nfft, F, sw.pfb_bluestein, sw);
    const bool blue_ok = blue_m > 0;
    if (sw.pfb_lds && (direct_ok || blue_ok) && (noise ? noise_fft : sw.tones_fft))
        return setup_pfb_lds(h, noise, F, tone, blue_ok ? blue_m : 0);
    const bool tones_global = !noise && sw.tones_fft;
    if (noise_fft || tones_global) return setup_pfb_global(h, tones_global, F, tone);
    return setup_pfb_ddc(h, F, tone);
}

void describe_pfb_lds(const gsdr_demod *h, std::string &s) {
    // the shape launch_pfb_lds chose for the last call (pfb_plan.h; frames -1: no call yet), and this handle's calls
    // so far by kernel, by the run kernel's filter (direct variant 0 - 5, 0: staged), with teams, with runs of
    // G >= 2 frames and with a last run short of G frames
    const gsdr::PfbChoice &c = h->pfb.last;
    auto n = [](unsigned long long v) { return std::to_string(v); };
    s += std::string(", \"pfb_last\": {\"kernel\": \"") + (h->pfb.last_frames < 0 ? "none" : gsdr::pfb_kernel_name(c)) + "\"";
    s += ", \"threads\": " + std::to_string(c.threads) + ", \"G\": " + std::to_string(c.G);
    s += ", \"direct\": " + std::to_string(c.direct) + ", \"dir_s\": " + std::to_string(c.dir_s);
    s += ", \"dir_gs\": " + std::to_string(c.dir_gs) + ", \"col\": " + std::to_string(c.col);
    s += ", \"teams\": " + std::to_string(c.teams) + ", \"twl\": " + std::to_string(c.twl);
    s += ", \"lds\": " + n(c.lds) + ", \"frames\": " + std::to_string(h->pfb.last_frames) + "}";
    s += ", \"pfb_calls\": {\"pfb_cu_kernel\": " + n(h->pfb.calls_cu) + ", \"pfb_lds_kernel\": " + n(h->pfb.calls_lds) + ", \"direct\": [";
    for (int v = 0; v < 6; ++v) s += (v ? ", " : "") + n(h->pfb.calls_direct[v]);
    s += "], \"teams\": " + n(h->pfb.calls_teams) + ", \"runs\": " + n(h->pfb.calls_runs) + ", \"short_last_run\": " + n(h->pfb.calls_short) + "}";
}

void describe_frame_average(const gsdr_demod *h, std::string &s) {
    s += ", \"frame_average\": " + std::to_string(h->pfb.avg_k);
    s += std::string(", \"frame_average_kind\": \"") + (h->pfb.avg_kind == GSDR_AVERAGE_POWER ? "power" : "complex") + "\"";
}

}  // namespace rx
}  // namespace gsdr

using namespace gsdr::rx;

extern "C" {

int gsdr_demod_set_frame_average(gsdr_demod *h, int k, int kind) {
    if (!h) return -1;
    if (h->mode != GSDR_TONES && h->mode != GSDR_NOISE) {
        h->err = "frame average: only TONES and NOISE handles have frames to average";
        return -1;
    }
    if (k < 1 || k > GSDR_FRAME_AVERAGE_MAX) {
        h->err = "frame average: k must be in [1, " + std::to_string(GSDR_FRAME_AVERAGE_MAX) + "]";
        return -1;
    }
    if (kind != GSDR_AVERAGE_COMPLEX && kind != GSDR_AVERAGE_POWER) {
        h->err = "frame average: kind must be GSDR_AVERAGE_COMPLEX (0) or GSDR_AVERAGE_POWER (1)";
        return -1;
    }
    if (h->pfb.win_seq > 0 || h->pl.count > 0) {
        h->err = "frame average: must be set before the first buffer goes through the handle";
        return -1;
    }
    if (h->device >= 0) HIPCHK(h, hipSetDevice(h->device));
    if (k > 1) {
        // everything the averaging needs, now (nothing is allocated by the first packets); kept when k changes again
        if (!h->pfb.d_avg_frames) HIPCHK(h, h->pfb.d_avg_frames.alloc((size_t)h->ddc.channels * (size_t)h->pfb.batching));
        for (auto &p : h->pfb.d_avg_acc) {
            if (!p) HIPCHK(h, p.alloc((size_t)h->ddc.channels));
            HIPCHK(h, hipMemset(p, 0, (size_t)h->ddc.channels * sizeof(float2)));
        }
    }
    const long long capacity = (long long)h->ddc.channels * ((h->pfb.batching + k - 1) / k);
    if (capacity > h->capacity) {
        // output staging that gsdr_demod_prepare sized for a larger k: nothing has used it yet, the entries make it anew
        h->host.d_out.reset();
        h->host.d_in.reset();                  // (the host entry allocates the two together)
        for (auto &sl : h->pl.slot) sl.d_out.reset();
    }
    h->pfb.avg_k = k;
    h->pfb.avg_kind = kind;
    h->pfb.avg_count = 0;
    h->capacity = capacity;
    return 0;
}

int gsdr_demod_frame_average(const gsdr_demod *h, int *kind) {
    if (kind) *kind = h ? h->pfb.avg_kind : GSDR_AVERAGE_COMPLEX;
    return h ? h->pfb.avg_k : 0;
}

int gsdr_frame_average_device(const gsdr_c64 *frames_dev, int n_frames, int n_ch, int k, int kind, int count,
                              const gsdr_c64 *acc_in_dev, gsdr_c64 *acc_out_dev, gsdr_c64 *out_dev, void *hip_stream) {
    const char *bad = nullptr;
    if (n_frames < 0 || n_ch < 1) bad = "n_frames must be >= 0 and n_ch >= 1";
    else if (k < 1 || k > GSDR_FRAME_AVERAGE_MAX) bad = "k must be in [1, 1048576]";
    else if (kind != GSDR_AVERAGE_COMPLEX && kind != GSDR_AVERAGE_POWER) bad = "kind must be GSDR_AVERAGE_COMPLEX or GSDR_AVERAGE_POWER";
    else if (count < 0 || count >= k) bad = "count must be in [0, k)";
    else if (!acc_out_dev || (n_frames > 0 && !frames_dev) || (count > 0 && !acc_in_dev) ||
             (((long long)count + n_frames) / k > 0 && !out_dev)) bad = "null buffer";
    else if (((uintptr_t)frames_dev | (uintptr_t)acc_in_dev | (uintptr_t)acc_out_dev | (uintptr_t)out_dev) & 7) bad = "pointers must be 8-byte aligned";
    if (bad) {
        gsdr::create_error() = std::string("gsdr_frame_average_device: ") + bad;
        return -1;
    }
    const hipError_t e = gsdr::launch_pfb_average(reinterpret_cast<const float2 *>(frames_dev), n_frames, n_ch, k, kind, count,
                                                  reinterpret_cast<const float2 *>(acc_in_dev), reinterpret_cast<float2 *>(acc_out_dev),
                                                  reinterpret_cast<float2 *>(out_dev), (hipStream_t)hip_stream);
    if (e != hipSuccess) {
        gsdr::create_error() = std::string("gsdr_frame_average_device: ") + hipGetErrorString(e);
        return -1;
    }
    return (int)(((long long)count + n_frames) / k);
}

int gsdr_demod_get_window(const gsdr_demod *h, float *w, int cap) {
    if (!h) return 0;
    const int n = (int)h->window.size();
    if (w)
        for (int i = 0; i < n && i < cap; ++i) w[i] = h->window[i];
    return n;
}

int gsdr_demod_get_bins(const gsdr_demod *h, int *bins, int cap) {
    if (!h) return 0;
    const int n = (int)h->pfb.bins.size();
    if (bins)
        for (int i = 0; i < n && i < cap; ++i) bins[i] = h->pfb.bins[i];
    return n;
}

}  // extern "C"
