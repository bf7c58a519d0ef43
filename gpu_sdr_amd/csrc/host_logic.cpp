// host_logic.cpp -- everything of the library that needs no GPU.  First the host-only pieces of the RX and TX paths:
// window/tap generation, the integer carry state machines, the tone->bin map, the chirp parameter derivation, the
// plans the launchers ask, and the host forms of the sc16 conversions and the frame average.  Then, the larger part,
// the six objects behind demodulated rows (trigger, welch, decim, sweep, resmap, stats: the stages), one section each:
// creation and its refusals, the bookkeeping and the host twin; what the sections share is in stage_state.h and just
// above the first of them.  No HIP here; everything is callable on a machine without a GPU (tests -m "not gpu").
//
// "ref:" citations are relative to /root/reference.
#include "../../include/gsdr.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "chirp_plan.h"
#include "ddc_plan.h"
#include "decim_state.h"
#include "pfb_plan.h"
#include "resmap_state.h"
#include "stage_state.h"
#include "stats_state.h"
#include "sweep_state.h"
#include "trigger_state.h"
#include "welch_state.h"

extern "C" void gsdr_stage_dev_close_(int device, gsdr::StageDev *dev) __attribute__((weak));   // stage_dev.cpp

namespace {
// ref: headers/kernels.cuh:34 -- the reference's float pi literal.
constexpr float kPiF = 3.14159265358979f;

using gsdr::stage_device_fault;
using gsdr::stage_refuse;

// gsdr_X_close of every stage: the device part first (the hook waits for the device), then the object
template <class Stage>
void stage_close(Stage *s) {
    if (!s) return;
    if (s->dev && gsdr_stage_dev_close_) gsdr_stage_dev_close_(s->device, s->dev);
    delete s;
}
}  // namespace

extern "C" {

int gsdr_abi_version(void) { return GSDR_ABI_VERSION; }

// ref: make_sinc_window, cpp/kernels.cu:258-310.
// Low-pass prototype 2fc*sinc(2*pi*fc*(i-c)) * hamming(i), unit DC gain.
// Quirks kept on purpose: the centre c = (length-1)/2 is an INTEGER division
// (:268), so even lengths are asymmetric; sinc and the hamming cosine are
// evaluated in float (nvcc picks the float overloads in host code), the
// hamming factor in double; the normalising sum is a float accumulator.
void gsdr_make_sinc_window(int length, float fc, float *w) {
    const int centre = (length - 1) / 2;
    const float gain = 2.f * fc;
    float sum = 0.f;
    for (int i = 0; i < length; ++i) {
        const int k = i - centre;
        float s = gain;
        if (k != 0) {
            const float a = 2.f * kPiF * fc * k;
            s = gain * sinf(a) / a;
        }
        const float c = cosf(2.f * kPiF * i / (length - 1));
        const float tap = static_cast<float>(s * (0.54 - 0.46 * c));
        w[i] = tap;
        sum += tap;
    }
    for (int i = 0; i < length; ++i) w[i] /= sum;
}

// ref: make_flat_window, cpp/kernels.cu:208-253.
// Zero on [0, side), 1/(length-side) on [side, length): the reference's
// trailing-zero loop (:223-226) is overwritten by its fill loop (:227-233).
void gsdr_make_flat_window(int length, int side, float *w) {
    float sum = 0.f;
    for (int i = 0; i < length; ++i) {
        w[i] = (i < side) ? 0.f : 1.f;
        if (i >= side) sum += 1.f;
    }
    for (int i = 0; i < length; ++i) w[i] /= sum;
}

// ---- TX tone comb: which spectrum the reference's tone_gen transforms --------
// ref: tone_gen, cpp/kernels.cu:617-635.  Tone i goes to index f if f > 0, else rate + f, of a
// zeroed vector of `rate` bins, by ASSIGNMENT: of tones that meet on one bin the last wins
// (they do not add).  An index outside [0, rate) -- a 0 Hz tone gives `rate` -- is written
// past the allocation there (undefined behaviour); the inverse FFT never sees that tone, so
// it is dropped here.  Output: the surviving tones as signed Hz (bin b > rate/2 -> b - rate,
// the same phasor) in first-seen bin order; returns their count.
int gsdr_tx_tone_bins(int rate, const int *freq, const float *ampl, int n, int *out_freq, float *out_ampl) {
    if (rate <= 0 || n < 0 || !freq || !ampl || !out_freq || !out_ampl) return -1;
    std::vector<long long> bins;
    int used = 0;
    for (int i = 0; i < n; ++i) {
        const long long idx = freq[i] > 0 ? (long long)freq[i] : (long long)rate + freq[i];
        if (idx < 0 || idx >= rate) continue;
        int k = 0;
        for (; k < used; ++k)
            if (bins[k] == idx) break;
        if (k == used) {
            bins.push_back(idx);
            ++used;
        }
        out_freq[k] = (int)(idx > rate / 2 ? idx - rate : idx);
        out_ampl[k] = ampl[i];
    }
    return used;
}

// ---- buffer_helper ---------------------------------------------------------
// ref: cpp/USRP_server_memory_management.cpp:104-156.  The batch count is the
// number of r >= 0 with r*n_tones + average*n_tones < eff_length (strict), the
// closed form of the reference's simulate_batching() loop (:145-156).
static int count_batches(const gsdr_buffer_helper *b) {
    const long long lim = (long long)b->eff_length - (long long)b->average * b->n_tones;
    if (lim <= 0) return 0;
    return (int)((lim + b->n_tones - 1) / b->n_tones);
}

static void refresh(gsdr_buffer_helper *b) {
    b->current_batch = count_batches(b);
    b->copy_size = b->n_eff_tones * b->current_batch;
    b->spare_samples = b->eff_length - b->current_batch * b->n_tones;
    b->spare_begin = b->eff_length - b->spare_samples;
}

void gsdr_buffer_helper_init(gsdr_buffer_helper *b, int n_tones, int buffer_len,
                             int average, int n_eff_tones) {
    b->n_tones = n_tones;
    b->buffer_len = buffer_len;
    b->average = average;
    b->n_eff_tones = n_eff_tones;
    b->eff_length = buffer_len;  // :114
    b->new_0 = 0;                // :121
    refresh(b);
}

void gsdr_buffer_helper_update(gsdr_buffer_helper *b) {
    b->new_0 = b->spare_samples;                      // :128
    b->eff_length = b->spare_samples + b->buffer_len; // :131
    refresh(b);
}

// ---- VNA_decimator_helper --------------------------------------------------
// ref: cpp/USRP_server_memory_management.cpp:30-56.
static void vna_refresh(gsdr_vna_helper *v) {
    v->valid_size = v->total_len / v->ppt;
    v->new0 = v->total_len - v->ppt * v->valid_size;
    v->spare_begin = v->total_len - v->new0;
}

void gsdr_vna_helper_init(gsdr_vna_helper *v, int ppt, int buffer_len) {
    v->ppt = ppt;
    v->buffer_len = buffer_len;
    v->total_len = buffer_len;
    vna_refresh(v);
}

void gsdr_vna_helper_update(gsdr_vna_helper *v) {
    v->total_len = v->buffer_len + v->new0;
    vna_refresh(v);
}

// ---- tone -> FFT bin -------------------------------------------------------
// ref: upload_multitone_parameters, cpp/USRP_demodulator.cpp:722-733.
// The reference scans every bin i and lets the LAST i whose open interval
// (c_i - bin, c_i + bin) contains the tone win, with c_i = i*bin - bin*(nfft/2)
// evaluated in double.  Only bins next to (f - c_0)/bin can match, so we test
// the same double predicate on a +-3 neighbourhood and keep the largest
// matching i: same result, O(n) instead of O(n * nfft).
void gsdr_pfb_tone_bins(int rate, int fft_tones, const int *freq, int n, int *bins) {
    const double bin = (double)rate / (double)fft_tones;
    const int half = fft_tones / 2;
    for (int u = 0; u < n; ++u) {
        bins[u] = -1;
        const double guess = ((double)freq[u] + bin * half) / bin;
        long long lo = (long long)std::floor(guess) - 3, hi = (long long)std::floor(guess) + 3;
        if (lo < 0) lo = 0;
        if (hi > fft_tones - 1) hi = fft_tones - 1;
        for (long long i = lo; i <= hi; ++i) {
            const double centre = (size_t)i * bin - bin * half;
            if ((freq[u] < centre + bin) && (freq[u] > centre - bin))
                bins[u] = (int)((i + half) % fft_tones);
        }
    }
}

// ref: cpp/USRP_demodulator.cpp:706 (the division and ceil are in float).
int gsdr_pfb_batching(long long buffer_len, int fft_tones, long long pf_average) {
    return (int)(std::ceil((float)buffer_len / (float)fft_tones) + pf_average + 5);
}

// ---- chirp parameters ------------------------------------------------------
// ref: cpp/USRP_demodulator.cpp:192-214, headers/kernels.cuh:58-64.
// The reference narrows doubles into `unsigned int chirpness` and `int f0`
// implicitly; for values outside the target range that is undefined in C++ and
// we pin what x86-64 does (cvttsd2si): wrap through 64 bits for chirpness,
// INT_MIN for f0.
void gsdr_chirp_derive(int rate, int freq0, int chirp_f, int swipe_s,
                       float chirp_t, gsdr_chirp_param *cp) {
    unsigned long long steps = (unsigned long long)(long long)swipe_s;  // :192
    if (steps < 1) steps = (unsigned long long)(chirp_t * rate);        // :193-196
    unsigned long long len = (unsigned long long)(chirp_t * rate / steps);  // :202, float maths
    if (len < 1) len = 1;                                               // :203-206
    const double two32m1 = std::pow(2, 32) - 1;
    const double slope = (two32m1 * (chirp_f - freq0) / ((double)steps - 1.)) / (double)rate;  // :210
    const double start = two32m1 * ((double)freq0 / (double)rate);                           // :214
    cp->num_steps = steps;
    cp->length = len;
    cp->chirpness = (slope > -9.2e18 && slope < 9.2e18) ? (unsigned int)(long long)slope : 0u;
    cp->f0 = (start > -2147483649.0 && start < 2147483648.0) ? (int)start : INT_MIN;
}

// ref: TX_buffer_generator, CHIRP case, cpp/USRP_buffer_generator.cpp:107-127.  The same derivation with one
// difference: when a step would be shorter than one sample the TX side also resets num_steps to chirp_t * rate
// (:115-119) BEFORE the slope is computed from it (:122); the RX side keeps the requested num_steps
// (cpp/USRP_demodulator.cpp:203-206).
void gsdr_chirp_derive_tx(int rate, int freq0, int chirp_f, int swipe_s,
                          float chirp_t, gsdr_chirp_param *cp) {
    unsigned long long steps = (unsigned long long)(long long)swipe_s;  // :107
    if (steps < 1) steps = (unsigned long long)(chirp_t * rate);        // :108-111
    unsigned long long len = (unsigned long long)(chirp_t * rate / steps);  // :117, float maths
    if (len < 1) {                                                      // :118-122
        len = 1;
        steps = (unsigned long long)(chirp_t * rate);
    }
    const double two32m1 = std::pow(2, 32) - 1;
    const double slope = (two32m1 * (chirp_f - freq0) / ((double)steps - 1.)) / (double)rate;  // :125
    const double start = two32m1 * ((double)freq0 / (double)rate);                           // :129
    cp->num_steps = steps;
    cp->length = len;
    cp->chirpness = (slope > -9.2e18 && slope < 9.2e18) ? (unsigned int)(long long)slope : 0u;
    cp->f0 = (start > -2147483649.0 && start < 2147483648.0) ? (int)start : INT_MIN;
}

// The lock-in form a CHIRP call takes (chirp_plan.h: the function the launchers themselves ask).
int gsdr_chirp_lockin_plan(unsigned long long num_steps, unsigned long long length, long long ppt,
                           unsigned long long index0, int valid, int chirps, int split, int partial_cap, int *parts,
                           int *per_part) {
    if (num_steps < 1 || length < 1 || num_steps > 0x7fffffffffffffffULL / length || ppt < 1 || ppt > INT_MAX || valid < 1 || chirps < 1 ||
        chirps > GSDR_MULTI_CHIRP_MAX || partial_cap < 0)
        return -1;
    const gsdr::ChirpPlan p =
        gsdr::chirp_lockin_plan(gsdr::chirp_plan_fits_32(num_steps, length, num_steps * length), length, ppt, index0, valid,
                                chirps, split != 0, partial_cap);
    if (parts) *parts = (int)p.parts;
    if (per_part) *per_part = (int)p.per_part;
    return p.form;
}

// The kernel and shape a TONES / NOISE call takes inside the LDS (pfb_plan.h: the function launch_pfb_lds itself asks).
int gsdr_pfb_plan(const gsdr_pfb_plan_in *in, gsdr_pfb_plan_out *out) {
    if (!in || !out) return -1;
    if (in->nfft < 1 || in->nfft > gsdr::kPfbLdsMaxN || in->avg < 1 || in->frames < 0 || in->n_out < 1 || in->cus < 1 || in->blue_m < 0)
        return -1;
    gsdr::Switches sw;
    sw.pfb_cu = in->pfb_cu; sw.pfb_direct = in->pfb_direct != 0; sw.pfb_col = in->pfb_col; sw.pfb_cu_nt = in->pfb_cu_nt;
    sw.pfb_teams = in->pfb_teams != 0; sw.pfb_radix8 = in->pfb_radix8 != 0; sw.pfb_fr = in->pfb_fr; sw.pfb_wide = in->pfb_wide;
    int r[32], nr;
    if (in->blue_m > 0) {
        long long m = 1;
        while (m < 2LL * in->nfft - 1) m <<= 1;
        if (m != in->blue_m || m > gsdr::kPfbLdsMaxN || !gsdr::pfb_cu_fits(in->nfft, in->avg, in->blue_m, sw)) return -1;
        nr = gsdr::fft_radices(in->blue_m, r, 32);
    } else {
        nr = gsdr::pfb_lds_plan(in->nfft, r, sw.pfb_radix8);
        if (nr < 0) return -1;
    }
    const gsdr::PfbChoice c = gsdr::pfb_choose(in->nfft, in->avg, in->blue_m, nr, r, in->frames, in->n_out, in->cus, sw);
    if (in->blue_m > 0 && !c.cu) return -1;                // only the run kernel knows Bluestein's identity
    *out = gsdr_pfb_plan_out{};
    out->cu = c.cu; out->threads = c.threads; out->G = c.G; out->twl = c.twl; out->lds = (int)c.lds;
    out->b_off = c.b_off; out->b_len = c.b_len; out->col = c.col; out->direct = c.direct; out->dir_s = c.dir_s;
    out->dir_gs = c.dir_gs; out->teams = c.teams;
    out->len = in->blue_m > 0 ? in->blue_m : in->nfft;
    out->n_radices = nr;
    for (int i = 0; i < nr && i < 16; ++i) out->radices[i] = r[i];
    return 0;
}

int gsdr_pfb_plan_many(const gsdr_pfb_plan_in *in, int count, gsdr_pfb_plan_out *out) {
    if (count < 0 || (count > 0 && (!in || !out))) return -1;
    for (int i = 0; i < count; ++i)
        if (gsdr_pfb_plan(in + i, out + i) != 0) return -1;
    return 0;
}

int gsdr_pfb_blue_length(int nfft, int avg, int pfb_bluestein, int pfb_direct, int pfb_radix8) {
    if (nfft < 1 || avg < 1) return 0;
    gsdr::Switches sw;
    sw.pfb_direct = pfb_direct != 0;
    sw.pfb_radix8 = pfb_radix8 != 0;
    return gsdr::pfb_blue_length(nfft, avg, pfb_bluestein, sw);
}

// The engine of a DIRECT handle and the shape of one of its launches (ddc_plan.h: the functions the handle itself asks,
// in the order setup_direct, setup_mfma and enqueue_mfma ask them).
int gsdr_ddc_plan(const gsdr_ddc_plan_in *in, gsdr_ddc_plan_out *out) {
    if (!in || !out) return -1;
    if (in->rate < 1 || in->tones < 1 || in->buffer_len < 1 || in->cus < 1 || in->rows < 0) return -1;
    const bool decimated = in->decim > 0;
    if (decimated && (in->buffer_len % in->decim != 0 || in->pf_average < 1 || in->pf_average > gsdr::kMaxF ||
                      in->decim > 0x7fffffffLL / in->pf_average))
        return -1;
    const long long L = in->buffer_len;
    const int N = in->tones, M = decimated ? (int)in->decim : 1, F = decimated ? (int)in->pf_average : 1;
    const long long max_rows = decimated ? L / M : 1;
    if (max_rows > 0x7fffffffLL || in->rows > max_rows) return -1;
    const long long rows = in->rows > 0 ? in->rows : max_rows;
    const bool overlap = in->overlapped != 0;
    gsdr::Switches sw;
    sw.ddc_mfma = in->ddc_mfma != 0; sw.ddc_few = in->ddc_few != 0; sw.ddc_pipe = in->ddc_pipe != 0; sw.ddc_k = in->ddc_k;
    sw.ddc_waves = in->ddc_waves; sw.ddc_nch = in->ddc_nch; sw.mfma_asm = in->mfma_asm; sw.mfma_tt = in->mfma_tt;
    sw.mfma_pk = in->mfma_pk; sw.mfma_w = in->mfma_w; sw.mfma_rt = in->mfma_rt; sw.mfma_w8 = in->mfma_w8 != 0;
    sw.mfma_prec = in->mfma_prec; sw.mfma_3m = in->mfma_3m; sw.mfma_3m_rot = in->mfma_3m_rot; sw.mfma_fold = in->mfma_fold;
    sw.mfma_fold_products = in->mfma_fold_products; sw.mfma_wave_tones = in->mfma_wave_tones; sw.mfma_span = in->mfma_span;
    *out = gsdr_ddc_plan_out{};
    out->complex_mac_min_blocks = (int)gsdr::kMac3MinBlocks;
    out->rotation_min_blocks = (int)gsdr::kRot2MinBlocks;
    out->fold_min_blocks = (int)gsdr::kFoldMinBlocks;
    out->span128_min_blocks = (int)gsdr::kSpan128MinBlocks;
    const int simds = in->cus * 4;
    const gsdr::DdcEngine engine = gsdr::ddc_direct_engine(in->decim, N, M, F, L, sw);
    out->engine = (int)engine;
    if (engine != gsdr::DdcEngine::Mfma) {
        const bool flat = engine == gsdr::DdcEngine::Flat;
        const gsdr::DdcBlocking b = gsdr::ddc_blocking(flat, M, sw);
        const int TW = (N + 63) / 64;
        out->K = b.K; out->pad = b.pad; out->R = b.R;
        out->target_waves = gsdr::ddc_target_waves(simds, flat, sw);
        out->tails_nch = gsdr::ddc_tails_nch(F, (int)max_rows, out->target_waves, TW, sw.ddc_nch);
        out->chunks_want = (int)((long long)(1.3 * out->target_waves) / TW);
        out->chunks = gsdr::pick_chunks((int)rows, 1.3, out->target_waves, TW, F, out->tails_nch, sw.ddc_nch);
        return 0;
    }
    const gsdr::MfmaTile tile = gsdr::mfma_tile(sw);
    const int nk8 = (M * F + 7) / 8, ntg = ((N + 31) / 32 + tile.TT - 1) / tile.TT, ntq = (ntg + tile.W - 1) / tile.W;
    const long long nhi = (nk8 + 3) / 4, ngt = (rows + 31) / 32;
    const bool images = tile.kind == gsdr::MfmaKernel::AsmRing16 && gsdr::prec_pays(simds, (max_rows + 31) / 32, ntq, nk8, /*overlap=*/true, sw);
    const gsdr::ProductRule rule = images ? gsdr::product_rule(nhi, max_rows, ntg, sw) : gsdr::ProductRule{};
    const bool one_loop = rule.mac3;                     // every loop of the family but AsmRing16P belongs to a handle
    const gsdr::ProductDescribe d = gsdr::product_describe(rule);
    out->complex_mac = d.complex_mac; out->rotation_blocks = d.rotation_blocks; out->fold = d.fold;
    out->fold_products = d.fold_products; out->wave_tones = d.wave_tones; out->span_samples = d.span_samples;
    out->images = images;
    out->row_tiles_per_workgroup = gsdr::mfma_row_tiles(one_loop, overlap, nk8, ngt, ntq, sw);
    const gsdr::MfmaKernel kind = one_loop ? gsdr::product_loop_chosen(rule)
                                           : gsdr::mfma_launch_kernel(tile.kind, images, out->row_tiles_per_workgroup, simds, ngt, ntq, ntg, nk8, overlap, sw);
    out->preconverted = one_loop || kind == gsdr::MfmaKernel::AsmRing16P;
    out->eight_waves = kind == gsdr::MfmaKernel::AsmRing16W8;
    return 0;
}

// sc16 input widened on the host: an exact int16 -> float conversion and one IEEE multiply per component, what
// widen_sc16_kernel (ddc_kernels.hip) computes on the device, bit for bit.
void gsdr_widen_sc16_host(const gsdr_sc16 *in, gsdr_c64 *out, long long n, float scale) {
    for (long long k = 0; k < n; ++k) {
        out[k].x = (float)in[k].i * scale;
        out[k].y = (float)in[k].q * scale;
    }
}

// Mean of k consecutive frames per channel on the host, the arithmetic of include/gsdr.h operation for operation: what
// pfb_average_kernel (fft_kernels.hip) computes on the device, bit for bit.  Every sum and product is stored to a float
// before it is used again, and the function is compiled without contraction, so no compiler fuses a product into a sum.
// (Its refusal goes where the stages' go: gsdr_note_error_, stage_state.h.)
#if defined(__clang__)
#define GSDR_NO_CONTRACT
#elif defined(__GNUC__)
#define GSDR_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define GSDR_NO_CONTRACT
#endif

GSDR_NO_CONTRACT
int gsdr_frame_average_host(const gsdr_c64 *frames, int n_frames, int n_ch, int k, int kind, int count,
                            const gsdr_c64 *acc_in, gsdr_c64 *acc_out, gsdr_c64 *out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const char *bad = nullptr;
    if (n_frames < 0 || n_ch < 1) bad = "gsdr_frame_average: n_frames must be >= 0 and n_ch >= 1";
    else if (k < 1 || k > GSDR_FRAME_AVERAGE_MAX) bad = "gsdr_frame_average: k must be in [1, 1048576]";
    else if (kind != GSDR_AVERAGE_COMPLEX && kind != GSDR_AVERAGE_POWER) bad = "gsdr_frame_average: kind must be GSDR_AVERAGE_COMPLEX or GSDR_AVERAGE_POWER";
    else if (count < 0 || count >= k) bad = "gsdr_frame_average: count must be in [0, k)";
    else if (!acc_out || (n_frames > 0 && !frames) || (count > 0 && !acc_in)) bad = "gsdr_frame_average: null buffer";
    const long long rows = bad ? 0 : ((long long)count + n_frames) / k;
    if (!bad && rows > 0 && !out) bad = "gsdr_frame_average: null buffer";
    if (bad) {
        if (gsdr_note_error_) gsdr_note_error_(bad);
        return -1;
    }
    const float inv_k = 1.0f / (float)k;
    std::vector<gsdr_c64> acc((size_t)n_ch);
    int have = count;                                  // frames summed in acc
    for (int c = 0; c < n_ch; ++c) acc[(size_t)c] = count > 0 ? acc_in[c] : gsdr_c64{0.f, 0.f};
    long long row = 0;
    for (int f = 0; f < n_frames; ++f) {
        const gsdr_c64 *fr = frames + (size_t)f * (size_t)n_ch;
        for (int c = 0; c < n_ch; ++c) {
            gsdr_c64 t = fr[c];
            if (kind == GSDR_AVERAGE_POWER) {
                const float rr = t.x * t.x;
                const float ii = t.y * t.y;
                t.x = rr + ii;
                t.y = 0.f;
            }
            if (have == 0) {
                acc[(size_t)c] = t;
            } else {
                const float sx = acc[(size_t)c].x + t.x;
                const float sy = acc[(size_t)c].y + t.y;
                acc[(size_t)c].x = sx;
                acc[(size_t)c].y = sy;
            }
        }
        if (++have == k) {
            gsdr_c64 *o = out + (size_t)row * (size_t)n_ch;
            for (int c = 0; c < n_ch; ++c) {
                o[c].x = acc[(size_t)c].x * inv_k;
                o[c].y = acc[(size_t)c].y * inv_k;
            }
            ++row;
            have = 0;
        }
    }
    for (int c = 0; c < n_ch; ++c) acc_out[c] = have > 0 ? acc[(size_t)c] : gsdr_c64{0.f, 0.f};
    return (int)rows;
}

// sc16 output narrowed on the host, the arithmetic of include/gsdr.h step for step: what narrow_component
// (ddc_device.h) computes on the device, bit for bit.  The range is tested on the rounded FLOAT and the conversion
// only sees a value it can represent (converting a NaN or an out-of-range float is undefined behaviour).
// std::nearbyintf rounds in the current rounding mode: to nearest, ties to even, unless the caller changed it.
namespace {
GSDR_NO_CONTRACT
inline int16_t narrow_one_host(float c, float gain, long long &clipped) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float v = c * gain;
    if (v != v) {
        ++clipped;
        return 0;
    }
    const float r = std::nearbyintf(v);
    if (r > 32767.0f) {
        ++clipped;
        return 32767;
    }
    if (r < -32768.0f) {
        ++clipped;
        return -32768;
    }
    return (int16_t)(int)r;
}
}  // namespace

long long gsdr_narrow_sc16_host(const gsdr_c64 *in, gsdr_sc16 *out, long long n, float gain) {
    long long clipped = 0;
    for (long long k = 0; k < n; ++k) {
        out[k].i = narrow_one_host(in[k].x, gain, clipped);
        out[k].q = narrow_one_host(in[k].y, gain, clipped);
    }
    return clipped;
}

// ---- trigger: creation, bookkeeping and the host twin (the contract: include/gsdr.h, "trigger on the device") --------
// The host twin streams like the device path does -- it carries the last pre + post - 1 rows, the records of the last
// post - 1 rows and the last hitting row, and never recomputes a record -- so that set_levels between feeds means the
// same on both.  trigger_hits_kernel / trigger_select_kernel / trigger_capture_kernel (trigger_kernels.hip) give the
// same bits.
int gsdr_trigger_dev_create_(gsdr_trigger *t, const gsdr_trigger_level *levels) __attribute__((weak));
int gsdr_trigger_dev_set_levels_(gsdr_trigger *t, const gsdr_trigger_level *levels, void *hip_stream) __attribute__((weak));

namespace {
GSDR_NO_CONTRACT
inline gsdr_trigger_rec trigger_row_host(const gsdr_c64 *row, const gsdr_trigger_level *lv, int n_ch) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    gsdr_trigger_rec rec{0, 0, 0.f, 0};
    for (int c = 0; c < n_ch; ++c) {
        const float t0 = row[c].x - lv[c].bx;
        const float t1 = row[c].y - lv[c].by;
        const float p0 = t0 * lv[c].dx;
        const float p1 = t1 * lv[c].dy;
        const float q = p0 + p1;
        const bool up = q > lv[c].hi;
        const bool dn = !up && q < lv[c].lo;
        if (!(up || dn)) continue;
        if (rec.n_hit == 0) {
            rec.channel = c;
            rec.side = up ? 1 : -1;
            rec.q = q;
        }
        ++rec.n_hit;
    }
    return rec;
}
}  // namespace

gsdr_trigger *gsdr_trigger_create(int n_ch, int max_rows, int pre, int post, int holdoff, int max_events,
                                  const gsdr_trigger_level *levels, int device_index) {
    const char *const me = "gsdr_trigger_create";
    std::string bad;
    if (n_ch < 1 || n_ch > (1 << 20)) bad = "n_ch must be in [1, 1048576]";
    else if (max_rows < 1 || max_rows > (1 << 20)) bad = "max_rows must be in [1, 1048576]";
    else if (pre < 0) bad = "pre must be >= 0";
    else if (post < 1) bad = "post must be >= 1";
    else if ((long long)pre + post > 65536) bad = "pre + post must be <= 65536";
    else if (holdoff < 0 || holdoff > (1 << 30)) bad = "holdoff must be in [0, 1073741824]";
    else if (max_events < 1 || max_events > (1 << 20)) bad = "max_events must be in [1, 1048576]";
    else if (!levels) bad = "levels must not be NULL";
    else bad = stage_device_fault(device_index, "GSDR_TRIGGER_HOST", gsdr_trigger_dev_create_ != nullptr);
    if (!bad.empty()) {
        stage_refuse(me, bad);
        return nullptr;
    }
    gsdr_trigger *t = new (std::nothrow) gsdr_trigger();
    if (!t) {
        stage_refuse(me, "out of memory");
        return nullptr;
    }
    t->n_ch = n_ch, t->max_rows = max_rows, t->pre = pre, t->post = post, t->holdoff = holdoff, t->max_events = max_events;
    t->device = device_index;
    if (device_index != GSDR_TRIGGER_HOST) {
        if (gsdr_trigger_dev_create_(t, levels) != 0) {       // has noted why
            delete t;
            return nullptr;
        }
        return t;
    }
    try {
        t->levels.assign(levels, levels + n_ch);
        t->carry.assign((size_t)(pre + post - 1) * (size_t)n_ch, gsdr_c64{0.f, 0.f});
        t->recs.assign((size_t)(post - 1), gsdr_trigger_rec{0, 0, 0.f, 0});
        t->trig.assign((size_t)(post - 1), 0);
    } catch (const std::bad_alloc &) {
        delete t;
        stage_refuse(me, "pre + post and n_ch: no host memory for the carried rows");
        return nullptr;
    }
    return t;
}

int gsdr_trigger_set_levels(gsdr_trigger *t, const gsdr_trigger_level *levels, void *hip_stream) {
    if (!t || !levels) return stage_refuse("gsdr_trigger_set_levels", "null argument");
    if (t->device != GSDR_TRIGGER_HOST) return gsdr_trigger_dev_set_levels_(t, levels, hip_stream);
    t->levels.assign(levels, levels + t->n_ch);
    return 0;
}

int gsdr_trigger_reset(gsdr_trigger *t) {
    if (!t) return stage_refuse("gsdr_trigger_reset", "null object");
    // the device path reads `total` on the host and takes nothing from the carry of a stream that has just begun
    t->total = 0;
    t->last_hit = -1;
    for (auto &r : t->recs) r = gsdr_trigger_rec{0, 0, 0.f, 0};
    for (auto &f : t->trig) f = 0;
    return 0;
}

long long gsdr_trigger_rows(const gsdr_trigger *t) { return t ? t->total : 0; }

void gsdr_trigger_close(gsdr_trigger *t) { stage_close(t); }

int gsdr_trigger_feed_host(gsdr_trigger *t, const gsdr_c64 *rows, int n_rows, gsdr_trigger_event *events,
                           gsdr_c64 *snippets, int *n_dropped) {
    const char *const me = "gsdr_trigger_feed_host";
    if (!t) return stage_refuse(me, "null object");
    if (t->device != GSDR_TRIGGER_HOST)
        return stage_refuse(me, "a device object takes gsdr_trigger_feed or gsdr_trigger_feed_device");
    if (n_rows < 0 || n_rows > t->max_rows) return stage_refuse(me, "n_rows must be in [0, max_rows]");
    if (n_dropped) *n_dropped = 0;
    if (n_rows == 0) return 0;
    if (!rows || !events || !snippets) return stage_refuse(me, "null buffer");
    const size_t n_ch = (size_t)t->n_ch, n = (size_t)n_rows;
    const size_t P = (size_t)(t->post - 1), K = (size_t)(t->pre + t->post - 1), S = (size_t)(t->pre + t->post);
    const long long R0 = t->total, base = R0 - (long long)P;     // window entry j is stream row base + j
    std::vector<gsdr_trigger_rec> wrec;
    std::vector<unsigned char> wtrig;
    try {
        wrec.resize(P + n);
        wtrig.assign(P + n, 0);
    } catch (const std::bad_alloc &) {
        return stage_refuse(me, "out of memory");
    }
    for (size_t j = 0; j < P; ++j) wrec[j] = t->recs[j], wtrig[j] = t->trig[j];
    for (size_t i = 0; i < n; ++i) {
        const gsdr_trigger_rec rec = trigger_row_host(rows + i * n_ch, t->levels.data(), t->n_ch);
        wrec[P + i] = rec;
        if (rec.n_hit > 0) {
            const long long r = R0 + (long long)i;
            wtrig[P + i] = (t->last_hit < 0 || r - t->last_hit > t->holdoff) ? 1 : 0;
            t->last_hit = r;
        }
    }
    int n_events = 0, dropped = 0;
    for (size_t j = 0; j < n; ++j) {
        const long long r = base + (long long)j;
        if (!wtrig[j] || r < t->pre) continue;
        if (n_events >= t->max_events) {
            ++dropped;
            continue;
        }
        events[n_events] = gsdr_trigger_event{r, wrec[j].channel, wrec[j].side, wrec[j].q, wrec[j].n_hit};
        gsdr_c64 *dst = snippets + (size_t)n_events * S * n_ch;
        for (size_t k = 0; k < S; ++k) {
            const long long rel = r - t->pre + (long long)k - R0;     // in [-K, n)
            const gsdr_c64 *src = rel >= 0 ? rows + (size_t)rel * n_ch : t->carry.data() + (size_t)((long long)K + rel) * n_ch;
            std::memcpy(dst + k * n_ch, src, n_ch * sizeof(gsdr_c64));
        }
        ++n_events;
    }
    if (K > 0) {
        if (n >= K) {
            std::memcpy(t->carry.data(), rows + (n - K) * n_ch, K * n_ch * sizeof(gsdr_c64));
        } else {
            std::memmove(t->carry.data(), t->carry.data() + n * n_ch, (K - n) * n_ch * sizeof(gsdr_c64));
            std::memcpy(t->carry.data() + (K - n) * n_ch, rows, n * n_ch * sizeof(gsdr_c64));
        }
    }
    for (size_t j = 0; j < P; ++j) t->recs[j] = wrec[n + j], t->trig[j] = wtrig[n + j];
    t->total += n_rows;
    if (n_dropped) *n_dropped = dropped;
    return n_events;
}

// ---- welch: creation, bookkeeping and the host twin (the contract: include/gsdr.h, "Welch spectra on the device") ----
// The host twin is the estimator's statement in code: double throughout, a plain radix-2 transform, one segment at a
// time in stream order.  welch_append_kernel / welch_segment_kernel / welch_accumulate_kernel (welch_kernels.hip) run
// the float32 pipeline of the contract; they agree with this to the float32 transform's error, not bit for bit.
int gsdr_welch_dev_create_(gsdr_welch *w) __attribute__((weak));
int gsdr_welch_dev_reset_(gsdr_welch *w) __attribute__((weak));

namespace {
int welch_count(long long n_seg) { return n_seg > INT_MAX ? INT_MAX : (int)n_seg; }

// in-place radix-2 forward transform of N = 2 * tw.size() / 2 points; tw: (cos, -sin)(2 pi k / N), k < N / 2
void welch_fft_host(std::vector<double> &re, std::vector<double> &im, const std::vector<double> &tw) {
    const size_t N = re.size();
    for (size_t i = 1, j = 0; i < N; ++i) {
        size_t bit = N >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) {
            std::swap(re[i], re[j]);
            std::swap(im[i], im[j]);
        }
    }
    for (size_t len = 2; len <= N; len <<= 1) {
        const size_t stride = N / len;
        for (size_t i = 0; i < N; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const double wr = tw[2 * k * stride], wi = tw[2 * k * stride + 1];
                const size_t a = i + k, b = i + k + len / 2;
                const double tr = re[b] * wr - im[b] * wi, ti = re[b] * wi + im[b] * wr;
                re[b] = re[a] - tr;
                im[b] = im[a] - ti;
                re[a] += tr;
                im[a] += ti;
            }
    }
}

// segment s of channel c out of the pending rows: detrend, window, transform, accumulate, mean
void welch_segment_host(gsdr_welch *w, long long s, int c, std::vector<double> &re, std::vector<double> &im) {
    const int N = w->nperseg, K1 = N / 2 + 1;
    const size_t n_ch = (size_t)w->n_ch;
    const double *x = w->pending.data() + ((size_t)(s * w->step - w->pending_base) * n_ch + (size_t)c) * 2;
    const double mid = 0.5 * (double)(N - 1);
    double sr = 0.0, si = 0.0, tr = 0.0, ti = 0.0, mr = 0.0, mi = 0.0;
    for (int n = 0; n < N; ++n) {
        const double xr = x[(size_t)n * n_ch * 2], xi = x[(size_t)n * n_ch * 2 + 1], t = (double)n - mid;
        sr += xr, si += xi;
        tr += xr * t, ti += xi * t;
        if (n < w->step) mr += xr, mi += xi;
    }
    const double tt = (double)N * ((double)N * (double)N - 1.0) / 12.0;          // sum t_n^2
    double m_r = sr / N, m_i = si / N, b_r = tr / tt, b_i = ti / tt;
    if (w->detrend != GSDR_WELCH_DETREND_LINEAR) b_r = b_i = 0.0;
    for (int n = 0; n < N; ++n) {
        const double xr = x[(size_t)n * n_ch * 2], xi = x[(size_t)n * n_ch * 2 + 1], t = (double)n - mid;
        const bool raw = w->detrend == GSDR_WELCH_DETREND_NONE;
        const double win = (double)w->window[(size_t)n];
        re[(size_t)n] = (raw ? xr : xr - (m_r + b_r * t)) * win;
        im[(size_t)n] = (raw ? xi : xi - (m_i + b_i * t)) * win;
    }
    welch_fft_host(re, im, w->tw);
    double *acc = w->acc.data() + (size_t)c * 3 * (size_t)K1;
    for (int k = 0; k < K1; ++k) {
        const size_t km = (size_t)((N - k) & (N - 1));
        const double zr = re[(size_t)k], zi = im[(size_t)k], ur = re[km], ui = -im[km];       // Zm = conj Z[N - k]
        const double Xr = 0.5 * (zr + ur), Xi = 0.5 * (zi + ui);
        const double Yr = 0.5 * (zi - ui), Yi = -0.5 * (zr - ur);                             // (Z - Zm) / (2i)
        acc[k] += Xr * Xr + Xi * Xi;
        acc[K1 + k] += Yr * Yr + Yi * Yi;
        acc[2 * K1 + k] += Xr * Yr + Xi * Yi;
    }
    w->msum[(size_t)c * 2] += mr;
    w->msum[(size_t)c * 2 + 1] += mi;
}
}  // namespace

gsdr_welch *gsdr_welch_create(int n_ch, int max_rows, int nperseg, int step, int detrend, const float *window, int device_index) {
    const char *const me = "gsdr_welch_create";
    std::string bad;
    if (n_ch < 1 || n_ch > (1 << 20)) bad = "n_ch must be in [1, 1048576]";
    else if (max_rows < 1 || max_rows > (1 << 20)) bad = "max_rows must be in [1, 1048576]";
    else if (nperseg < 16 || nperseg > 8192 || (nperseg & (nperseg - 1))) bad = "nperseg must be a power of two in [16, 8192]";
    else if (step < nperseg / 8 || step > nperseg) bad = "step must be in [nperseg / 8, nperseg]";
    else if (detrend != GSDR_WELCH_DETREND_NONE && detrend != GSDR_WELCH_DETREND_CONSTANT && detrend != GSDR_WELCH_DETREND_LINEAR)
        bad = "detrend must be GSDR_WELCH_DETREND_NONE, _CONSTANT or _LINEAR";
    else bad = stage_device_fault(device_index, "GSDR_WELCH_HOST", gsdr_welch_dev_create_ != nullptr);
    if (!bad.empty()) {
        stage_refuse(me, bad);
        return nullptr;
    }
    gsdr_welch *w = new (std::nothrow) gsdr_welch();
    if (!w) {
        stage_refuse(me, "out of memory");
        return nullptr;
    }
    w->n_ch = n_ch, w->max_rows = max_rows, w->nperseg = nperseg, w->step = step, w->detrend = detrend;
    w->device = device_index;
    try {
        w->window.resize((size_t)nperseg);
        for (int n = 0; n < nperseg; ++n)
            w->window[(size_t)n] = window ? window[n] : (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)n / (double)nperseg));
        for (float v : w->window) w->sum_w2 += (double)v * (double)v;
        if (device_index == GSDR_WELCH_HOST) {
            w->acc.assign((size_t)n_ch * 3 * (size_t)(nperseg / 2 + 1), 0.0);
            w->msum.assign((size_t)n_ch * 2, 0.0);
            w->tw.resize((size_t)nperseg);
            for (int k = 0; k < nperseg / 2; ++k) {
                const double a = 2.0 * M_PI * (double)k / (double)nperseg;
                w->tw[2 * (size_t)k] = std::cos(a), w->tw[2 * (size_t)k + 1] = -std::sin(a);
            }
        }
    } catch (const std::bad_alloc &) {
        delete w;
        stage_refuse(me, "n_ch and nperseg: no host memory for the accumulators");
        return nullptr;
    }
    if (device_index != GSDR_WELCH_HOST && gsdr_welch_dev_create_(w) != 0) {       // has noted why
        delete w;
        return nullptr;
    }
    return w;
}

int gsdr_welch_reset(gsdr_welch *w) {
    if (!w) return stage_refuse("gsdr_welch_reset", "null object");
    if (w->dev && gsdr_welch_dev_reset_ && gsdr_welch_dev_reset_(w) != 0) return -1;
    w->total = 0;
    w->pending.clear();
    w->pending_base = 0;
    for (auto &v : w->acc) v = 0.0;
    for (auto &v : w->msum) v = 0.0;
    return 0;
}

long long gsdr_welch_rows(const gsdr_welch *w) { return w ? w->total : 0; }

long long gsdr_welch_segments(const gsdr_welch *w) { return w ? gsdr_welch_segments_of(w->total, w->nperseg, w->step) : 0; }

void gsdr_welch_close(gsdr_welch *w) { stage_close(w); }

int gsdr_welch_feed_host(gsdr_welch *w, const gsdr_c64 *rows, int n_rows) {
    const char *const me = "gsdr_welch_feed_host";
    if (!w) return stage_refuse(me, "null object");
    if (w->device != GSDR_WELCH_HOST) return stage_refuse(me, "a device object takes gsdr_welch_feed_device");
    if (n_rows < 0 || n_rows > w->max_rows) return stage_refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows) return stage_refuse(me, "null buffer: rows");
    const size_t n_ch = (size_t)w->n_ch, n = (size_t)n_rows;
    std::vector<double> re, im;
    try {
        const size_t at = w->pending.size();
        w->pending.resize(at + n * n_ch * 2);
        for (size_t i = 0; i < n * n_ch; ++i) w->pending[at + 2 * i] = (double)rows[i].x, w->pending[at + 2 * i + 1] = (double)rows[i].y;
        re.resize((size_t)w->nperseg), im.resize((size_t)w->nperseg);
    } catch (const std::bad_alloc &) {
        return stage_refuse(me, "out of memory");
    }
    const long long s0 = gsdr_welch_segments_of(w->total, w->nperseg, w->step);
    w->total += n_rows;
    const long long s1 = gsdr_welch_segments_of(w->total, w->nperseg, w->step);
    for (long long s = s0; s < s1; ++s)
        for (int c = 0; c < w->n_ch; ++c) welch_segment_host(w, s, c, re, im);
    // rows in front of the next segment are done with
    const long long keep_from = std::min(s1 * (long long)w->step, w->total);
    if (keep_from > w->pending_base) {
        w->pending.erase(w->pending.begin(), w->pending.begin() + (std::ptrdiff_t)((size_t)(keep_from - w->pending_base) * n_ch * 2));
        w->pending_base = keep_from;
    }
    return 0;
}

int gsdr_welch_read_host(gsdr_welch *w, int mode, const gsdr_c64 *gain, double fs, double *psd, double *mean) {
    const char *const me = "gsdr_welch_read_host";
    if (!w) return stage_refuse(me, "null object");
    if (w->device != GSDR_WELCH_HOST) return stage_refuse(me, "a device object takes gsdr_welch_read or gsdr_welch_read_device");
    if (mode < GSDR_WELCH_RAW || mode > GSDR_WELCH_GAIN) return stage_refuse(me, "mode must be GSDR_WELCH_RAW, _ROTATE, _DBC or _GAIN");
    if (!(fs > 0.0) || !std::isfinite(fs)) return stage_refuse(me, "fs must be finite and > 0");
    if (mode == GSDR_WELCH_GAIN && !gain) return stage_refuse(me, "gain must not be NULL with GSDR_WELCH_GAIN");
    if (!psd) return stage_refuse(me, "null buffer: psd");
    const long long n_seg = gsdr_welch_segments_of(w->total, w->nperseg, w->step);
    if (n_seg == 0) return 0;
    const int N = w->nperseg, K1 = N / 2 + 1;
    const double rows_in = (double)n_seg * (double)w->step, scale = 1.0 / (fs * w->sum_w2 * (double)n_seg);
    for (int c = 0; c < w->n_ch; ++c) {
        const double mr = w->msum[(size_t)c * 2] / rows_in, mi = w->msum[(size_t)c * 2 + 1] / rows_in;
        if (mean) mean[(size_t)c * 2] = mr, mean[(size_t)c * 2 + 1] = mi;
        double gr = 1.0, gi = 0.0;
        const double m2 = mr * mr + mi * mi;
        if (mode == GSDR_WELCH_GAIN) gr = (double)gain[c].x, gi = (double)gain[c].y;
        else if (mode != GSDR_WELCH_RAW && std::isfinite(m2) && m2 > 0.0) {
            const double d = mode == GSDR_WELCH_ROTATE ? std::sqrt(m2) : m2;         // |m| / m = conj m / |m|, 1 / m = conj m / |m|^2
            gr = mr / d, gi = -mi / d;
        }
        const double *acc = w->acc.data() + (size_t)c * 3 * (size_t)K1;
        double *out = psd + (size_t)c * 2 * (size_t)K1;
        for (int k = 0; k < K1; ++k) {
            const double f = (k > 0 && k < N / 2) ? 2.0 : 1.0;
            const double a0 = acc[k], a1 = acc[K1 + k], a2 = acc[2 * K1 + k];
            out[k] = (gr * gr * a0 + gi * gi * a1 - 2.0 * gr * gi * a2) * f * scale;
            out[K1 + k] = (gi * gi * a0 + gr * gr * a1 + 2.0 * gr * gi * a2) * f * scale;
        }
    }
    return welch_count(n_seg);
}

// ---- decim: creation, the default taps, the count law and the host twin (the contract: include/gsdr.h, "FIR
// decimation on the device"; the blocks and the ring: decim_state.h) -------------------------------------------------
// The host twin keeps the same ring of chunk sums as the device and walks the rows in stream order; every chain of
// fused multiply-adds and every addition is the one decim_partial_kernel / decim_combine_kernel (decim_kernels.hip)
// make, so the bits are the same.
int gsdr_decim_dev_create_(gsdr_decim *d) __attribute__((weak));

namespace {
// output row of block k (complete) out of the ring: the chunk sums oldest first
GSDR_NO_CONTRACT
void decim_emit_host(const gsdr_decim *d, long long k, gsdr_c64 *out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const size_t n_ch = (size_t)d->n_ch, F = (size_t)d->F;
    for (size_t c = 0; c < n_ch; ++c) {
        float sx = 0.f, sy = 0.f;
        for (int j = d->F - 1; j >= 0; --j) {
            const long long kb = k - j;
            gsdr_c64 p{0.f, 0.f};
            if (kb >= 0) p = d->ring[((size_t)(kb % d->ring_blocks) * F + (size_t)j) * n_ch + c];
            if (j == d->F - 1) {
                sx = p.x, sy = p.y;
            } else {
                const float tx = sx + p.x, ty = sy + p.y;
                sx = tx, sy = ty;
            }
        }
        out[c].x = sx, out[c].y = sy;
    }
}
}  // namespace

int gsdr_decim_default_taps(int q, float *w) {
    if (q < 2 || q > 4096 || !w) return -1;
    const int T = 20 * q + 1, mid = 10 * q;
    std::vector<double> h((size_t)T);
    for (int n = 0; n <= mid; ++n) {
        const int m = n - mid;
        const double x = M_PI * (double)m / (double)q;
        const double s = m == 0 ? 1.0 : std::sin(x) / x;
        const double win = 0.54 - 0.46 * std::cos(2.0 * M_PI * (double)n / (double)(T - 1));
        h[(size_t)n] = h[(size_t)(T - 1 - n)] = s / (double)q * win;
    }
    double sum = 0.0;
    for (double v : h) sum += v;
    for (int n = 0; n < T; ++n) w[n] = (float)(h[(size_t)n] / sum);
    return T;
}

gsdr_decim *gsdr_decim_create(int n_ch, int max_rows, int q, int n_taps, const float *taps, long long offset, int device_index) {
    const char *const me = "gsdr_decim_create";
    std::string bad;
    if (n_ch < 1 || n_ch > (1 << 20)) bad = "n_ch must be in [1, 1048576]";
    else if (max_rows < 1 || max_rows > (1 << 20)) bad = "max_rows must be in [1, 1048576]";
    else if (q < 1 || q > 4096) bad = "q must be in [1, 4096]";
    else if (!taps && n_taps != 0) bad = "taps must not be NULL with n_taps != 0 (NULL and 0 select the default taps)";
    else if (!taps && q < 2) bad = "q must be >= 2 for the default taps (taps == NULL)";
    else if (taps && (n_taps < 1 || n_taps > 64 * q)) bad = "n_taps must be in [1, 64 q]";
    else if (offset < 0 || offset > (1LL << 30)) bad = "offset must be in [0, 1073741824]";
    else bad = stage_device_fault(device_index, "GSDR_DECIM_HOST", gsdr_decim_dev_create_ != nullptr);
    if (bad.empty() && taps)
        for (int t = 0; t < n_taps; ++t)
            if (!std::isfinite(taps[t])) {
                bad = "taps must all be finite";
                break;
            }
    if (!bad.empty()) {
        stage_refuse(me, bad);
        return nullptr;
    }
    gsdr_decim *d = new (std::nothrow) gsdr_decim();
    if (!d) {
        stage_refuse(me, "out of memory");
        return nullptr;
    }
    const int T = taps ? n_taps : 20 * q + 1;
    d->n_ch = n_ch, d->max_rows = max_rows, d->q = q, d->n_taps = T, d->offset = offset, d->device = device_index;
    d->F = (T + q - 1) / q;
    d->ring_blocks = (long long)(max_rows - 1) / q + 2 + d->F;
    const unsigned long long ring_bytes = (unsigned long long)d->ring_blocks * (unsigned long long)d->F * (unsigned long long)n_ch * sizeof(gsdr_c64);
    try {
        d->taps.resize((size_t)T);
        if (taps) std::copy(taps, taps + T, d->taps.begin());
        else gsdr_decim_default_taps(q, d->taps.data());
        if (device_index == GSDR_DECIM_HOST) {
            if (ring_bytes > (unsigned long long)PTRDIFF_MAX) throw std::bad_alloc();
            d->ring.assign((size_t)(ring_bytes / sizeof(gsdr_c64)), gsdr_c64{0.f, 0.f});
        }
    } catch (const std::bad_alloc &) {
        delete d;
        stage_refuse(me, "n_ch, max_rows, q and n_taps: no host memory for the carried chunk sums (" + std::to_string(ring_bytes >> 20) + " MiB)");
        return nullptr;
    }
    if (device_index != GSDR_DECIM_HOST && gsdr_decim_dev_create_(d) != 0) {       // has noted why
        delete d;
        return nullptr;
    }
    return d;
}

int gsdr_decim_next_rows(const gsdr_decim *d, int n_rows) {
    if (!d) return 0;
    if (n_rows < 0 || n_rows > d->max_rows) return stage_refuse("gsdr_decim_next_rows", "n_rows must be in [0, max_rows]");
    return (int)(gsdr_decim_out_of(d->total + n_rows, d->offset, d->q) - gsdr_decim_out_of(d->total, d->offset, d->q));
}

long long gsdr_decim_out_capacity(const gsdr_decim *d) { return d ? (long long)(d->max_rows - 1) / d->q + 1 : 0; }

int gsdr_decim_get_taps(const gsdr_decim *d, float *w, int cap) {
    if (!d) return 0;
    if (w && cap > 0) std::copy(d->taps.begin(), d->taps.begin() + std::min(cap, d->n_taps), w);
    return d->n_taps;
}

int gsdr_decim_reset(gsdr_decim *d) {
    if (!d) return stage_refuse("gsdr_decim_reset", "null object");
    // the ring needs no clearing: a block's sums start at +0 with its first row, and no output reads a block before row 0
    d->total = 0;
    return 0;
}

long long gsdr_decim_rows(const gsdr_decim *d) { return d ? d->total : 0; }

long long gsdr_decim_rows_out(const gsdr_decim *d) { return d ? gsdr_decim_out_of(d->total, d->offset, d->q) : 0; }

void gsdr_decim_close(gsdr_decim *d) { stage_close(d); }

int gsdr_decim_feed_host(gsdr_decim *d, const gsdr_c64 *rows, int n_rows, gsdr_c64 *out) {
    const char *const me = "gsdr_decim_feed_host";
    if (!d) return stage_refuse(me, "null object");
    if (d->device != GSDR_DECIM_HOST) return stage_refuse(me, "a device object takes gsdr_decim_feed or gsdr_decim_feed_device");
    if (n_rows < 0 || n_rows > d->max_rows) return stage_refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows) return stage_refuse(me, "null buffer: rows");
    const int emitted = (int)(gsdr_decim_out_of(d->total + n_rows, d->offset, d->q) - gsdr_decim_out_of(d->total, d->offset, d->q));
    if (emitted > 0 && !out) return stage_refuse(me, "null buffer: out");
    const size_t n_ch = (size_t)d->n_ch, F = (size_t)d->F;
    const long long q = d->q, r0 = gsdr_decim_r0(d->offset, d->q), shift = d->offset / q;
    const int T = d->n_taps;
    const float *h = d->taps.data();
    int at = 0;
    for (int i = 0; i < n_rows; ++i) {
        const long long R = d->total + i, k = (R - r0) / q;
        const int pos = (int)(R - r0 - k * q);                                 // the row's place in its block
        gsdr_c64 *blk = d->ring.data() + (size_t)(k % d->ring_blocks) * F * n_ch;
        if (pos == 0 || R == 0) std::fill(blk, blk + F * n_ch, gsdr_c64{0.f, 0.f});
        const gsdr_c64 *x = rows + (size_t)i * n_ch;
        for (int j = 0; j < d->F; ++j) {
            const long long t = (long long)T - (long long)(j + 1) * q + pos;
            if (t < 0) continue;
            const float w = h[t];
            gsdr_c64 *a = blk + (size_t)j * n_ch;
            for (size_t c = 0; c < n_ch; ++c) {
                a[c].x = std::fmaf(w, x[c].x, a[c].x);
                a[c].y = std::fmaf(w, x[c].y, a[c].y);
            }
        }
        if (pos == q - 1 && k - shift >= 0) decim_emit_host(d, k, out + (size_t)at++ * n_ch);
    }
    d->total += n_rows;
    return emitted;
}

// ---- sweep: creation, the counts, the host twin and the two helpers (the contract: include/gsdr.h, "VNA sweep
// accumulator on the device"; the fold: sweep_state.h) ---------------------------------------------------------------
// The host twin walks the rows in stream order; every addition, the division, the fma of the variance and the block
// order of the slope are the ones sweep_kernels.hip makes, so the bits are the same.
int gsdr_sweep_dev_create_(gsdr_sweep *s) __attribute__((weak));
int gsdr_sweep_dev_reset_(gsdr_sweep *s) __attribute__((weak));
int gsdr_sweep_dev_slope_(gsdr_sweep *s, double *d_host, void *hip_stream) __attribute__((weak));

namespace {
long long sweep_rows_of(const gsdr_sweep *s, long long p) {
    return gsdr_sweep_rows_of(gsdr_sweep_edge_of(s->first_row, s->n_points, s->group),
                              gsdr_sweep_edge_of(s->first_row + s->total, s->n_points, s->group), p, s->group);
}

// the float32 mean of (p, c) as a read returns it
GSDR_NO_CONTRACT
gsdr_c64 sweep_mean_host(const gsdr_sweep *s, long long p, int c) {
    const long long cnt = sweep_rows_of(s, p);
    if (cnt <= 0) return gsdr_c64{0.f, 0.f};
    const double *a = s->acc.data() + ((size_t)p * (size_t)s->n_ch + (size_t)c) * 4;
    const double n = (double)cnt;
    return gsdr_c64{(float)(a[0] / n), (float)(a[1] / n)};
}

float sweep_var_host(double sum, double q, double n) {
    const double v = std::fma(-sum, sum / n, q) / (n - 1.0);
    return (float)(v < 0.0 ? 0.0 : v);                             // a NaN is not < 0: it stays
}
}  // namespace

gsdr_sweep *gsdr_sweep_create(int n_ch, long long n_points, long long group, long long first_row, int device_index) {
    const char *const me = "gsdr_sweep_create";
    std::string bad;
    if (n_ch < 1 || n_ch > (1 << 20)) bad = "n_ch must be in [1, 1048576]";
    else if (n_points < 1 || n_points > (1LL << 24)) bad = "n_points must be in [1, 16777216]";
    else if (n_points * (long long)n_ch > (1LL << 25)) bad = "n_points * n_ch must be <= 33554432 (32 bytes each)";
    else if (group < 1 || group > (1LL << 30)) bad = "group must be in [1, 1073741824]";
    else if (first_row < 0 || first_row > (1LL << 62)) bad = "first_row must be in [0, 2^62]";
    else bad = stage_device_fault(device_index, "GSDR_SWEEP_HOST", gsdr_sweep_dev_create_ != nullptr);
    if (!bad.empty()) {
        stage_refuse(me, bad);
        return nullptr;
    }
    gsdr_sweep *s = new (std::nothrow) gsdr_sweep();
    if (!s) {
        stage_refuse(me, "out of memory");
        return nullptr;
    }
    s->n_ch = n_ch, s->n_points = n_points, s->group = group, s->first_row = first_row, s->device = device_index;
    const size_t cells = (size_t)n_points * (size_t)n_ch;
    if (device_index == GSDR_SWEEP_HOST) {
        try {
            s->acc.assign(cells * 4, 0.0);
        } catch (const std::bad_alloc &) {
            delete s;
            stage_refuse(me, "n_ch and n_points: no host memory for the accumulators (" + std::to_string((cells * 32) >> 20) + " MiB)");
            return nullptr;
        }
    } else if (gsdr_sweep_dev_create_(s) != 0) {                   // has noted why
        delete s;
        return nullptr;
    }
    return s;
}

void gsdr_sweep_close(gsdr_sweep *s) { stage_close(s); }

int gsdr_sweep_reset(gsdr_sweep *s, long long first_row) {
    const char *const me = "gsdr_sweep_reset";
    if (!s) return stage_refuse(me, "null object");
    if (first_row < 0 || first_row > (1LL << 62)) return stage_refuse(me, "first_row must be in [0, 2^62]");
    if (s->dev) {
        if (!gsdr_sweep_dev_reset_ || gsdr_sweep_dev_reset_(s) != 0) return -1;      // has noted why
    } else {
        std::fill(s->acc.begin(), s->acc.end(), 0.0);
    }
    s->first_row = first_row, s->total = 0;
    return 0;
}

long long gsdr_sweep_rows(const gsdr_sweep *s) { return s ? s->total : 0; }

long long gsdr_sweep_sweeps(const gsdr_sweep *s) {
    return s ? gsdr_sweep_min_rows(s->first_row, s->total, s->n_points, s->group) / s->group : 0;
}

long long gsdr_sweep_point_rows(const gsdr_sweep *s, long long p) { return s && p >= 0 && p < s->n_points ? sweep_rows_of(s, p) : 0; }

GSDR_NO_CONTRACT
int gsdr_sweep_feed_host(gsdr_sweep *s, const gsdr_c64 *rows, int n_rows) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const char *const me = "gsdr_sweep_feed_host";
    if (!s) return stage_refuse(me, "null object");
    if (s->device != GSDR_SWEEP_HOST) return stage_refuse(me, "a device object takes gsdr_sweep_feed_device");
    if (n_rows < 0 || n_rows > GSDR_SWEEP_MAX_FEED) return stage_refuse(me, "n_rows must be in [0, 16777216]");
    if (n_rows == 0) return 0;
    if (s->total > GSDR_SWEEP_MAX_ROWS - n_rows) return stage_refuse(me, "n_rows: the stream would pass 2^61 rows");
    if (!rows) return stage_refuse(me, "null buffer: rows");
    const size_t n_ch = (size_t)s->n_ch;
    const long long R = s->first_row + s->total;
    long long p = (R / s->group) % s->n_points, in = R % s->group;          // the point of the row and its place in the group
    for (int i = 0; i < n_rows; ++i) {
        double *a = s->acc.data() + (size_t)p * n_ch * 4;
        const gsdr_c64 *x = rows + (size_t)i * n_ch;
        for (size_t c = 0; c < n_ch; ++c) {
            const double re = (double)x[c].x, im = (double)x[c].y;
            const double rr = re * re, ii = im * im;                       // exact: 48 bits
            a[4 * c + 0] = a[4 * c + 0] + re;
            a[4 * c + 1] = a[4 * c + 1] + im;
            a[4 * c + 2] = a[4 * c + 2] + rr;
            a[4 * c + 3] = a[4 * c + 3] + ii;
        }
        if (++in == s->group) {
            in = 0;
            if (++p == s->n_points) p = 0;
        }
    }
    s->total += n_rows;
    return 0;
}

GSDR_NO_CONTRACT
int gsdr_sweep_read_host(gsdr_sweep *s, gsdr_c64 *mean, gsdr_c64 *var) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const char *const me = "gsdr_sweep_read_host";
    if (!s) return stage_refuse(me, "null object");
    if (s->device != GSDR_SWEEP_HOST) return stage_refuse(me, "a device object takes gsdr_sweep_read or gsdr_sweep_read_device");
    if (!mean) return stage_refuse(me, "null buffer: mean");
    const gsdr_sweep_edge ea = gsdr_sweep_edge_of(s->first_row, s->n_points, s->group),
                          eb = gsdr_sweep_edge_of(s->first_row + s->total, s->n_points, s->group);
    const size_t n_ch = (size_t)s->n_ch;
    for (long long p = 0; p < s->n_points; ++p) {
        const long long cnt = gsdr_sweep_rows_of(ea, eb, p, s->group);
        const double n = (double)cnt;
        for (size_t c = 0; c < n_ch; ++c) {
            const size_t at = (size_t)p * n_ch + c;
            const double *a = s->acc.data() + at * 4;
            gsdr_c64 m{0.f, 0.f}, v{0.f, 0.f};
            if (cnt > 0) {
                m = gsdr_c64{(float)(a[0] / n), (float)(a[1] / n)};
                if (var && cnt > 1) v = gsdr_c64{sweep_var_host(a[0], a[2], n), sweep_var_host(a[1], a[3], n)};
            }
            mean[at] = m;
            if (var) var[at] = v;
        }
    }
    return 0;
}

GSDR_NO_CONTRACT
int gsdr_sweep_slope(gsdr_sweep *s, double *d_host, void *hip_stream) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const char *const me = "gsdr_sweep_slope";
    if (!s) return stage_refuse(me, "null object");
    if (!d_host) return stage_refuse(me, "null buffer: d_host");
    if (s->dev) return gsdr_sweep_dev_slope_ ? gsdr_sweep_dev_slope_(s, d_host, hip_stream) : stage_refuse(me, "no device part in this build");
    const long long terms = s->n_points - 1, blocks = gsdr_sweep_slope_blocks(s->n_points);
    for (int c = 0; c < s->n_ch; ++c) {
        double sx = 0.0, sy = 0.0;
        for (long long b = 0; b < blocks; ++b) {
            const long long first = b * kSweepSlopeBlock, last = std::min(first + kSweepSlopeBlock, terms);
            double dx = 0.0, dy = 0.0;
            if (first < last) {
                gsdr_c64 m0 = sweep_mean_host(s, first, c);
                for (long long p = first; p < last; ++p) {
                    const gsdr_c64 m1 = sweep_mean_host(s, p + 1, c);
                    const double ar = (double)m1.x, ai = (double)m1.y, br = (double)m0.x, bi = (double)m0.y;
                    const double rr = ar * br, ii = ai * bi, ir = ai * br, ri = ar * bi;      // exact
                    const double tx = rr + ii, ty = ir - ri;
                    dx = dx + tx, dy = dy + ty;
                    m0 = m1;
                }
            }
            if (b == 0) sx = dx, sy = dy;
            else sx = sx + dx, sy = sy + dy;
        }
        d_host[2 * c] = sx, d_host[2 * c + 1] = sy;
    }
    return 0;
}

int gsdr_sweep_shape_for_chirp(const gsdr_chirp_param *cp, long long decim, long long *n_points, long long *group) {
    const char *const me = "gsdr_sweep_shape_for_chirp";
    if (!cp || !n_points || !group) return stage_refuse(me, "null pointer");
    if (decim < 0) return stage_refuse(me, "decim must be >= 0");
    if (cp->num_steps < 1 || cp->length < 1 || cp->num_steps > (1ULL << 62) / cp->length) return stage_refuse(me, "cp: num_steps and length must be >= 1, their product <= 2^62");
    long long np = 0, g = 0;
    if (decim == 0) {
        if (cp->num_steps > (1ULL << 24) || cp->length > (1ULL << 30)) return stage_refuse(me, "cp: num_steps > 2^24 or length > 2^30 (the limits of gsdr_sweep_create)");
        np = (long long)cp->num_steps, g = (long long)cp->length;
    } else {
        const unsigned long long period = cp->num_steps * cp->length;
        if ((unsigned long long)decim > period / cp->length) return stage_refuse(me, "decim: a row of length * decim samples is longer than the period");
        const unsigned long long ppt = cp->length * (unsigned long long)decim;
        if (period % ppt != 0) return stage_refuse(me, "decim: length * decim does not divide the period num_steps * length, the points do not repeat from sweep to sweep");
        if (period / ppt > (1ULL << 24)) return stage_refuse(me, "cp, decim: more than 2^24 points");
        np = (long long)(period / ppt), g = 1;
    }
    *n_points = np, *group = g;
    return 0;
}

GSDR_NO_CONTRACT
int gsdr_vna_axis(double rate, double freq0, double chirp_f, double swipe_s, long long n_points, double rf, double *f) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const char *const me = "gsdr_vna_axis";
    if (!f) return stage_refuse(me, "null buffer: f");
    if (!(swipe_s >= 2.0)) return stage_refuse(me, "swipe_s must be >= 2");
    if (n_points < 1) return stage_refuse(me, "n_points must be >= 1");
    if (!(rate > 0.0)) return stage_refuse(me, "rate must be > 0");
    const double two32m1 = 4294967295.0;
    const double df = std::trunc(two32m1 * (chirp_f - freq0) / (swipe_s - 1.0) / rate);
    const double stop = freq0 + df * (swipe_s - 1.0) * rate / two32m1;
    // numpy.linspace: arange(n) * step + start, the last point set to stop
    const double step = n_points > 1 ? (stop - freq0) / (double)(n_points - 1) : 0.0;
    for (long long i = 0; i < n_points; ++i) {
        const double at = (double)i * step;
        const double y = at + freq0;
        f[i] = rf + y;
    }
    if (n_points > 1) f[n_points - 1] = rf + stop;
    return 0;
}

// ---- resmap: the constants, creation, the offsets and the host twin (the contract: include/gsdr.h, "resonator map on
// the device"; the per-sample law: gsdr_resmap_sample, resmap_state.h) --------------------------------------------------
// The twin calls the function resmap_kernel (resmap_kernels.hip) calls, on the same tables: the bits are the same.
int gsdr_resmap_dev_create_(gsdr_resmap *r) __attribute__((weak));
int gsdr_resmap_dev_set_offsets_(gsdr_resmap *r, void *hip_stream) __attribute__((weak));

GSDR_NO_CONTRACT
int gsdr_resmap_constants(double f_tone, double f0, double A, double phi, double D, double Qe_re, double Qe_im, double *constants) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const char *const me = "gsdr_resmap_constants";
    const char *bad = nullptr;
    if (!std::isfinite(f_tone)) bad = "f_tone must be finite";
    else if (!std::isfinite(f0) || !(f0 > 0.0)) bad = "f0 must be finite and > 0 (MHz)";
    else if (!std::isfinite(A) || !(A > 0.0)) bad = "A must be finite and > 0";
    else if (!std::isfinite(phi)) bad = "phi must be finite";
    else if (!std::isfinite(D)) bad = "D must be finite";
    else if (!std::isfinite(Qe_re)) bad = "Qe_re must be finite";
    else if (!std::isfinite(Qe_im)) bad = "Qe_im must be finite";
    else if (Qe_re == 0.0 && Qe_im == 0.0) bad = "Qe_re and Qe_im: Qe must not be 0";
    else if (!constants) bad = "constants must not be NULL";
    if (bad) return stage_refuse(me, bad);
    const double f0_hz = f0 * 1e6;
    const double df = f_tone - f0_hz;
    const double slope = 1e-6 * D;
    const double cable = slope * df;
    const double theta = cable + phi;
    const double arg = 2.0 * M_PI * theta;
    const double nr = A * std::cos(arg), ni = A * std::sin(arg);
    const double nr2 = nr * nr, ni2 = ni * ni;
    const double nn = nr2 + ni2;
    const double qr2 = Qe_re * Qe_re, qi2 = Qe_im * Qe_im;
    const double qq = qr2 + qi2;
    const double rr = nr * Qe_re, ii = ni * Qe_im, ir = ni * Qe_re, ri = nr * Qe_im;
    const double kr_num = rr + ii, ki_num = ir - ri;
    constants[0] = nr;
    constants[1] = ni;
    constants[2] = nr / nn;
    constants[3] = -ni / nn;
    constants[4] = kr_num / qq;
    constants[5] = ki_num / qq;
    constants[6] = f0_hz / 2.0;
    return 0;
}

gsdr_resmap *gsdr_resmap_create(int n_ch, int max_rows, int n_out, const int *channels, const double *constants, int kind, int device_index) {
    const char *const me = "gsdr_resmap_create";
    std::string bad;
    if (n_ch < 1 || n_ch > (1 << 20)) bad = "n_ch must be in [1, 1048576]";
    else if (max_rows < 1 || max_rows > (1 << 20)) bad = "max_rows must be in [1, 1048576]";
    else if (n_out < 1 || n_out > (1 << 20)) bad = "n_out must be in [1, 1048576]";
    else if (!channels && n_out != n_ch) bad = "channels must not be NULL with n_out != n_ch (NULL is the identity)";
    else if (!constants) bad = "constants must not be NULL";
    else if (kind != GSDR_RESMAP_CAL && kind != GSDR_RESMAP_X_DQR && kind != GSDR_RESMAP_X_QR) bad = "kind must be GSDR_RESMAP_CAL, GSDR_RESMAP_X_DQR or GSDR_RESMAP_X_QR";
    else bad = stage_device_fault(device_index, "GSDR_RESMAP_HOST", gsdr_resmap_dev_create_ != nullptr);
    if (bad.empty() && channels)
        for (int k = 0; k < n_out; ++k)
            if (channels[k] < 0 || channels[k] >= n_ch) {
                bad = "channels must all be in [0, n_ch)";
                break;
            }
    if (bad.empty())
        for (size_t i = 0; i < (size_t)n_out * GSDR_RESMAP_NCONST; ++i)
            if (!std::isfinite(constants[i])) {
                bad = "constants must all be finite";
                break;
            }
    if (!bad.empty()) {
        stage_refuse(me, bad);
        return nullptr;
    }
    gsdr_resmap *r = new (std::nothrow) gsdr_resmap();
    if (!r) {
        stage_refuse(me, "out of memory");
        return nullptr;
    }
    r->n_ch = n_ch, r->max_rows = max_rows, r->n_out = n_out, r->kind = kind, r->device = device_index;
    try {
        r->channels.resize((size_t)n_out);
        r->cols.resize((size_t)n_out);
        r->offsets.assign(2 * (size_t)n_out, 0.0);
    } catch (const std::bad_alloc &) {
        delete r;
        stage_refuse(me, "n_out: no host memory for the tables (" + std::to_string(((size_t)n_out * 84) >> 20) + " MiB)");
        return nullptr;
    }
    r->identity = n_out == n_ch;
    for (int k = 0; k < n_out; ++k) {
        r->channels[(size_t)k] = channels ? channels[k] : k;
        r->identity = r->identity && r->channels[(size_t)k] == k;
        const double *c = constants + (size_t)k * GSDR_RESMAP_NCONST;
        r->cols[(size_t)k] = gsdr_resmap_col{c[0], c[1], c[2], c[3], c[4], c[5], c[6], 0.0};
    }
    if (device_index != GSDR_RESMAP_HOST && gsdr_resmap_dev_create_(r) != 0) {     // has noted why
        delete r;
        return nullptr;
    }
    return r;
}

void gsdr_resmap_close(gsdr_resmap *r) { stage_close(r); }

int gsdr_resmap_set_offsets(gsdr_resmap *r, const double *xy, void *hip_stream) {
    const char *const me = "gsdr_resmap_set_offsets";
    if (!r) return stage_refuse(me, "null object");
    if (xy)
        for (size_t i = 0; i < 2 * (size_t)r->n_out; ++i)
            if (!std::isfinite(xy[i])) return stage_refuse(me, "xy must all be finite");
    if (xy) std::copy(xy, xy + 2 * (size_t)r->n_out, r->offsets.begin());
    else std::fill(r->offsets.begin(), r->offsets.end(), 0.0);
    if (!r->dev) return 0;
    return gsdr_resmap_dev_set_offsets_ ? gsdr_resmap_dev_set_offsets_(r, hip_stream) : stage_refuse(me, "no device part in this build");
}

int gsdr_resmap_n_out(const gsdr_resmap *r) { return r ? r->n_out : 0; }

int gsdr_resmap_kind(const gsdr_resmap *r) { return r ? r->kind : 0; }

int gsdr_resmap_get_constants(const gsdr_resmap *r, double *constants, int cap) {
    if (!r) return 0;
    for (int k = 0; constants && k < std::min(cap, r->n_out); ++k) {
        const gsdr_resmap_col &c = r->cols[(size_t)k];
        const double v[GSDR_RESMAP_NCONST] = {c.nr, c.ni, c.gr, c.gi, c.kr, c.ki, c.hf0};
        std::copy(v, v + GSDR_RESMAP_NCONST, constants + (size_t)k * GSDR_RESMAP_NCONST);
    }
    return r->n_out;
}

int gsdr_resmap_get_offsets(const gsdr_resmap *r, double *xy, int cap) {
    if (!r) return 0;
    if (xy && cap > 0) std::copy(r->offsets.begin(), r->offsets.begin() + 2 * (std::ptrdiff_t)std::min(cap, r->n_out), xy);
    return r->n_out;
}

int gsdr_resmap_get_channels(const gsdr_resmap *r, int *channels, int cap) {
    if (!r) return 0;
    if (channels && cap > 0) std::copy(r->channels.begin(), r->channels.begin() + std::min(cap, r->n_out), channels);
    return r->n_out;
}

int gsdr_resmap_feed_host(gsdr_resmap *r, const gsdr_c64 *rows, int n_rows, gsdr_c64 *out) {
    const char *const me = "gsdr_resmap_feed_host";
    if (!r) return stage_refuse(me, "null object");
    if (r->device != GSDR_RESMAP_HOST) return stage_refuse(me, "a device object takes gsdr_resmap_feed or gsdr_resmap_feed_device");
    if (n_rows < 0 || n_rows > r->max_rows) return stage_refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows) return stage_refuse(me, "null buffer: rows");
    if (!out) return stage_refuse(me, "null buffer: out");
    const size_t n_ch = (size_t)r->n_ch, n_out = (size_t)r->n_out;
    if (!(rows == out && r->identity)) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(rows), b = reinterpret_cast<uintptr_t>(out);
        const uintptr_t na = (uintptr_t)n_rows * n_ch * sizeof(gsdr_c64), nb = (uintptr_t)n_rows * n_out * sizeof(gsdr_c64);
        if (a < b + nb && b < a + na) return stage_refuse(me, "out overlaps rows (out == rows is allowed with the identity channel list only)");
    }
    for (size_t i = 0; i < (size_t)n_rows; ++i) {
        const gsdr_c64 *x = rows + i * n_ch;
        gsdr_c64 *y = out + i * n_out;
        for (size_t k = 0; k < n_out; ++k) {
            const gsdr_c64 s = x[(size_t)r->channels[k]];
            gsdr_resmap_sample(r->kind, r->cols[k], r->offsets[2 * k], r->offsets[2 * k + 1], s.x, s.y, y[k].x, y[k].y);
        }
    }
    return n_rows;
}

// ---- stats: creation, the axes, the host twin, the quantiles and the levels (the contract: include/gsdr.h, "row
// statistics on the device"; the laws: stats_state.h) -------------------------------------------------------------------
// The twin calls the functions stats_feed_kernel and stats_read_kernel (stats_kernels.hip) call, walks every chain in
// stream order and joins the chains by the halving tree as it is written in the header: the bits are the same.  The
// levels are made HERE for both kinds of object, from the summaries and the medians a read returns: one text, one sqrt.
int gsdr_stats_dev_create_(gsdr_stats *s) __attribute__((weak));
int gsdr_stats_dev_reset_(gsdr_stats *s, int upload) __attribute__((weak));
int gsdr_stats_dev_fetch_(gsdr_stats *s, const char *entry, gsdr_stats_summary *summary, const double *pr, int n_p, double *quantiles,
                          unsigned long long *counts, void *hip_stream) __attribute__((weak));

}  // extern "C"

namespace {
// "" or what is wrong with the axes; the tables' entries into out
GSDR_NO_CONTRACT
std::string stats_axes_of(const gsdr_trigger_level *axes, int n_ch, int n_bins, std::vector<gsdr_stats_axis> &out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    out.resize((size_t)n_ch);
    for (int c = 0; c < n_ch; ++c) {
        const gsdr_trigger_level &a = axes[c];
        if (!std::isfinite(a.lo) || !std::isfinite(a.hi) || !(a.lo < a.hi)) return "axes: lo < hi, both finite, is required of every channel (channel " + std::to_string(c) + ")";
        const double lo = (double)a.lo, hi = (double)a.hi;
        const double sum = lo + hi, range = hi - lo;
        out[(size_t)c] = gsdr_stats_axis{a.bx, a.by, a.dx, a.dy, a.lo, a.hi, 0.5 * sum, (double)n_bins / range, range / (double)n_bins};
    }
    return std::string();
}

// the host twin's read of channel c: the summary and, where out is not null, the n_p quantiles
GSDR_NO_CONTRACT
gsdr_stats_summary stats_channel_host(const gsdr_stats *s, int c, std::vector<gsdr_stats_chain> &tree, const double *pr, int n_p, double *out) {
    const size_t n_ch = (size_t)s->n_ch;
    const unsigned long long *cnt = s->counts.data() + (size_t)c * (size_t)(s->n_bins + 3);
    for (int j = 0; j < s->lanes; ++j) tree[(size_t)j] = s->chains[(size_t)j * n_ch + (size_t)c];
    for (int h = s->lanes / 2; h >= 1; h /= 2)
        for (int j = 0; j < h; ++j) tree[(size_t)j] = gsdr_stats_chain_join(tree[(size_t)j], tree[(size_t)(j + h)]);
    unsigned long long bins = 0;
    for (int b = 0; b < s->n_bins; ++b) bins += cnt[1 + b];
    const gsdr_stats_axis &ax = s->axes[(size_t)c];
    const unsigned long long under = cnt[0], over = cnt[s->n_bins + 1];
    const gsdr_stats_summary sum = gsdr_stats_summarise(tree[0], ax.p, under, bins, over, cnt[s->n_bins + 2]);
    for (int ip = 0; out && ip < n_p; ++ip) {
        double &o = out[ip];
        if (sum.n == 0) {
            o = std::nan("");
            continue;
        }
        const unsigned long long rank = gsdr_stats_rank(pr[ip], sum.n);
        o = under >= rank ? -HUGE_VAL : HUGE_VAL;                  // a rank that no bin holds lies in `over`
        unsigned long long C = under;
        for (int b = 0; under < rank && b < s->n_bins; ++b) {
            const unsigned long long h = cnt[1 + b];
            if (rank <= C + h) {
                o = gsdr_stats_in_bin(ax, b, rank, C, h);
                break;
            }
            C += h;
        }
    }
    return sum;
}

// fl32 of a finite or infinite double as IEEE rounds it to nearest, without a conversion that is out of range in C++
float stats_fl32(double v) {
    const double a = std::fabs(v);
    if (a <= 3.4028234663852886e38) return (float)v;              // FLT_MAX
    const float r = a >= 3.4028235677973366e38 ? HUGE_VALF : 3.402823466e+38f;      // from 2^128 - 2^103 on: the tie goes to even
    return v < 0.0 ? -r : r;
}

// the summaries, the quantiles and the counters of either kind of object (each output may be null)
int stats_fetch(gsdr_stats *s, const char *me, gsdr_stats_summary *summary, const double *pr, int n_p, double *quantiles, unsigned long long *counts,
                void *hip_stream) {
    if (s->dev) {
        if (!gsdr_stats_dev_fetch_) return stage_refuse(me, "no device part in this build");
        return gsdr_stats_dev_fetch_(s, me, summary, pr, n_p, quantiles, counts, hip_stream);
    }
    if (summary || quantiles) {
        std::vector<gsdr_stats_chain> tree;
        try {
            tree.resize((size_t)s->lanes);
        } catch (const std::bad_alloc &) {
            return stage_refuse(me, "out of memory");
        }
        for (int c = 0; c < s->n_ch; ++c) {
            const gsdr_stats_summary sum = stats_channel_host(s, c, tree, pr, n_p, quantiles ? quantiles + (size_t)c * (size_t)n_p : nullptr);
            if (summary) summary[c] = sum;
        }
    }
    if (counts) std::copy(s->counts.begin(), s->counts.end(), counts);
    return 0;
}
}  // namespace

extern "C" {

gsdr_stats *gsdr_stats_create(int n_ch, int max_rows, int n_bins, int lanes, const gsdr_trigger_level *axes, int device_index) {
    const char *const me = "gsdr_stats_create";
    std::string bad;
    std::vector<gsdr_stats_axis> table;
    if (n_ch < 1 || n_ch > (1 << 20)) bad = "n_ch must be in [1, 1048576]";
    else if (max_rows < 1 || max_rows > (1 << 20)) bad = "max_rows must be in [1, 1048576]";
    else if (n_bins < 1 || n_bins > GSDR_STATS_MAX_BINS) bad = "n_bins must be in [1, 4096]";
    else if (lanes < 0 || lanes > GSDR_STATS_MAX_LANES || (lanes & (lanes - 1)) != 0) bad = "lanes must be 0 or a power of two in [1, 32768]";
    else if (!axes) bad = "axes must not be NULL";
    else bad = stage_device_fault(device_index, "GSDR_STATS_HOST", gsdr_stats_dev_create_ != nullptr);
    gsdr_stats *s = nullptr;
    try {
        if (bad.empty()) bad = stats_axes_of(axes, n_ch, n_bins, table);
        if (bad.empty()) s = new gsdr_stats();
    } catch (const std::bad_alloc &) {
        bad = "n_ch: no host memory for the axes";
    }
    if (!bad.empty()) {
        stage_refuse(me, bad);
        return nullptr;
    }
    s->n_ch = n_ch, s->max_rows = max_rows, s->n_bins = n_bins, s->device = device_index;
    s->lanes = lanes ? lanes : gsdr_stats_lanes_rule(n_ch, max_rows);
    s->axes.swap(table);
    const size_t chains = (size_t)s->lanes * (size_t)n_ch, counters = (size_t)n_ch * (size_t)(n_bins + 3);
    if (device_index == GSDR_STATS_HOST) {
        try {
            s->chains.assign(chains, gsdr_stats_chain{0.0, 0.0, HUGE_VALF, -HUGE_VALF});
            s->counts.assign(counters, 0ULL);
        } catch (const std::bad_alloc &) {
            delete s;
            stage_refuse(me, "n_ch, lanes and n_bins: no host memory for the chains and the counters (" + std::to_string((chains * 24 + counters * 8) >> 20) + " MiB)");
            return nullptr;
        }
    } else if (gsdr_stats_dev_create_(s) != 0) {                   // has noted why
        delete s;
        return nullptr;
    }
    return s;
}

void gsdr_stats_close(gsdr_stats *s) { stage_close(s); }

long long gsdr_stats_rows(const gsdr_stats *s) { return s ? s->total : 0; }

int gsdr_stats_lanes(const gsdr_stats *s) { return s ? s->lanes : 0; }

int gsdr_stats_n_bins(const gsdr_stats *s) { return s ? s->n_bins : 0; }

// The launch of a feed (stats_state.h: the function launch_stats_feed itself asks).
int gsdr_stats_plan(int n_ch, int n_bins, int lanes, int out[4]) {
    if (!out || !gsdr::stats_shape_ok(n_ch, n_bins, lanes)) return -1;
    const gsdr::StatsPlan p = gsdr::stats_plan_of(n_ch, n_bins, lanes);
    out[0] = p.tile, out[1] = p.tiles, out[2] = p.splits, out[3] = (int)p.lds_bytes;
    return 0;
}

int gsdr_stats_reset(gsdr_stats *s, const gsdr_trigger_level *axes) {
    const char *const me = "gsdr_stats_reset";
    if (!s) return stage_refuse(me, "null object");
    if (axes) {
        std::vector<gsdr_stats_axis> table;
        std::string bad;
        try {
            bad = stats_axes_of(axes, s->n_ch, s->n_bins, table);
        } catch (const std::bad_alloc &) {
            bad = "out of memory";
        }
        if (!bad.empty()) return stage_refuse(me, bad);
        s->axes.swap(table);
    }
    if (s->dev) {
        if (!gsdr_stats_dev_reset_ || gsdr_stats_dev_reset_(s, axes != nullptr) != 0) return -1;      // has noted why
    } else {
        std::fill(s->chains.begin(), s->chains.end(), gsdr_stats_chain{0.0, 0.0, HUGE_VALF, -HUGE_VALF});
        std::fill(s->counts.begin(), s->counts.end(), 0ULL);
    }
    s->total = 0;
    return 0;
}

GSDR_NO_CONTRACT
int gsdr_stats_feed_host(gsdr_stats *s, const gsdr_c64 *rows, int n_rows) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const char *const me = "gsdr_stats_feed_host";
    if (!s) return stage_refuse(me, "null object");
    if (s->device != GSDR_STATS_HOST) return stage_refuse(me, "a device object takes gsdr_stats_feed_device");
    if (n_rows < 0 || n_rows > s->max_rows) return stage_refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows) return stage_refuse(me, "null buffer: rows");
    const size_t n_ch = (size_t)s->n_ch, nb3 = (size_t)(s->n_bins + 3);
    for (int i = 0; i < n_rows; ++i) {
        const size_t j = (size_t)((s->total + i) % s->lanes);
        const gsdr_c64 *x = rows + (size_t)i * n_ch;
        gsdr_stats_chain *ch = s->chains.data() + j * n_ch;
        for (size_t c = 0; c < n_ch; ++c) {
            float q;
            const int slot = gsdr_stats_sample(s->axes[c], s->n_bins, x[c].x, x[c].y, q);
            ++s->counts[c * nb3 + (size_t)slot];
            if (slot != s->n_bins + 2) gsdr_stats_chain_add(ch[c], s->axes[c].p, q);
        }
    }
    s->total += n_rows;
    return 0;
}

int gsdr_stats_read_host(gsdr_stats *s, gsdr_stats_summary *summary) {
    const char *const me = "gsdr_stats_read_host";
    if (!s) return stage_refuse(me, "null object");
    if (s->device != GSDR_STATS_HOST) return stage_refuse(me, "a device object takes gsdr_stats_read or gsdr_stats_read_device");
    if (!summary) return stage_refuse(me, "null buffer: summary");
    return stats_fetch(s, me, summary, nullptr, 0, nullptr, nullptr, nullptr);
}

int gsdr_stats_counts(gsdr_stats *s, unsigned long long *counts_host, void *hip_stream) {
    const char *const me = "gsdr_stats_counts";
    if (!s) return stage_refuse(me, "null object");
    if (!counts_host) return stage_refuse(me, "null buffer: counts_host");
    return stats_fetch(s, me, nullptr, nullptr, 0, nullptr, counts_host, hip_stream);
}

int gsdr_stats_quantiles(gsdr_stats *s, const double *pr, int n_p, double *out_host, void *hip_stream) {
    const char *const me = "gsdr_stats_quantiles";
    if (!s) return stage_refuse(me, "null object");
    if (n_p < 1 || n_p > GSDR_STATS_MAX_QUANTILES) return stage_refuse(me, "n_p must be in [1, 16]");
    if (!pr) return stage_refuse(me, "null buffer: pr");
    if (!out_host) return stage_refuse(me, "null buffer: out_host");
    for (int i = 0; i < n_p; ++i)
        if (!(pr[i] > 0.0 && pr[i] <= 1.0)) return stage_refuse(me, "pr must all be in (0, 1]");
    return stats_fetch(s, me, nullptr, pr, n_p, out_host, nullptr, hip_stream);
}

GSDR_NO_CONTRACT
int gsdr_stats_levels(gsdr_stats *s, int centre, double nsigma, const unsigned char *on, gsdr_trigger_level *out_host, void *hip_stream) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const char *const me = "gsdr_stats_levels";
    if (!s) return stage_refuse(me, "null object");
    if (centre != GSDR_STATS_CENTRE_MEAN && centre != GSDR_STATS_CENTRE_MEDIAN) return stage_refuse(me, "centre must be GSDR_STATS_CENTRE_MEAN or GSDR_STATS_CENTRE_MEDIAN");
    if (!std::isfinite(nsigma) || nsigma < 0.0) return stage_refuse(me, "nsigma must be finite and >= 0");
    if (!out_host) return stage_refuse(me, "null buffer: out_host");
    std::vector<gsdr_stats_summary> sum;
    std::vector<double> med;
    try {
        sum.resize((size_t)s->n_ch);
        med.resize((size_t)s->n_ch);
    } catch (const std::bad_alloc &) {
        return stage_refuse(me, "out of memory");
    }
    const double half = 0.5;
    const bool median = centre == GSDR_STATS_CENTRE_MEDIAN;
    if (stats_fetch(s, me, sum.data(), &half, 1, median ? med.data() : nullptr, nullptr, hip_stream) != 0) return -1;
    for (int c = 0; c < s->n_ch; ++c) {
        const gsdr_stats_axis &ax = s->axes[(size_t)c];
        const double mid = median ? med[(size_t)c] : sum[(size_t)c].mean;
        const double sigma = std::sqrt(sum[(size_t)c].var);
        gsdr_trigger_level lv{ax.bx, ax.by, ax.dx, ax.dy, -HUGE_VALF, HUGE_VALF};
        if (!(on && on[c] == 0) && sum[(size_t)c].n >= 2 && std::isfinite(mid) && std::isfinite(sigma)) {
            const double span = nsigma * sigma;
            const double lo = mid - span, hi = mid + span;
            lv.lo = stats_fl32(lo), lv.hi = stats_fl32(hi);
        }
        out_host[c] = lv;
    }
    return 0;
}

}  // extern "C"
