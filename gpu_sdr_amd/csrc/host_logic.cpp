// host_logic.cpp -- the host-only pieces of the RX and TX paths: window/tap generation, the integer carry state
// machines, the tone->bin map, the chirp parameter derivation, the plans the launchers ask, and the host forms of the
// sc16 conversions and the frame average.  No HIP here; everything is callable on a machine without a GPU (tests -m
// "not gpu").  The objects behind demodulated rows have a host file each (X_host.cpp; stage_state.h).
//
// "ref:" citations are relative to /root/reference.
#include "../../include/gsdr.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "chirp_plan.h"
#include "ddc_plan.h"
#include "pfb_plan.h"
#include "stage_state.h"

namespace {
// ref: headers/kernels.cuh:34 -- the reference's float pi literal.
constexpr float kPiF = 3.14159265358979f;
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
// (Its refusal goes where the stages' go, and the two macros are theirs: gsdr_note_error_, stage_state.h.)
GSDR_NO_CONTRACT
int gsdr_frame_average_host(const gsdr_c64 *frames, int n_frames, int n_ch, int k, int kind, int count,
                            const gsdr_c64 *acc_in, gsdr_c64 *acc_out, gsdr_c64 *out) {
    GSDR_NO_CONTRACT_BODY
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
    GSDR_NO_CONTRACT_BODY
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

}  // extern "C"
