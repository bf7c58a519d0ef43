// welch_host.cpp -- the Welch accumulator's creation, bookkeeping and host twin (the contract: include/gsdr.h, "Welch
// spectra on the device").  The host twin is the estimator's statement in code: double throughout, a plain radix-2
// transform, one segment at a time in stream order.  welch_append_kernel / welch_segment_kernel /
// welch_accumulate_kernel (welch_kernels.hip) run the float32 pipeline of the contract; they agree with this to the
// float32 transform's error, not bit for bit.  No HIP here.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "stage_host.h"
#include "welch_state.h"

extern "C" {

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
    std::string bad;
    if (n_ch < 1 || n_ch > (1 << 20)) bad = "n_ch must be in [1, 1048576]";
    else if (max_rows < 1 || max_rows > (1 << 20)) bad = "max_rows must be in [1, 1048576]";
    else if (nperseg < 16 || nperseg > 8192 || (nperseg & (nperseg - 1))) bad = "nperseg must be a power of two in [16, 8192]";
    else if (step < nperseg / 8 || step > nperseg) bad = "step must be in [nperseg / 8, nperseg]";
    else if (detrend != GSDR_WELCH_DETREND_NONE && detrend != GSDR_WELCH_DETREND_CONSTANT && detrend != GSDR_WELCH_DETREND_LINEAR)
        bad = "detrend must be GSDR_WELCH_DETREND_NONE, _CONSTANT or _LINEAR";
    else bad = stage_device_fault(device_index, "GSDR_WELCH_HOST", gsdr_welch_dev_create_ != nullptr);
    return stage_create<gsdr_welch>(
        "gsdr_welch_create", bad, device_index, "n_ch and nperseg: no host memory for the accumulators",
        [&](gsdr_welch &w) {
            w.n_ch = n_ch, w.max_rows = max_rows, w.nperseg = nperseg, w.step = step, w.detrend = detrend;
            w.window.resize((size_t)nperseg);
            for (int n = 0; n < nperseg; ++n)
                w.window[(size_t)n] = window ? window[n] : (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)n / (double)nperseg));
            for (float v : w.window) w.sum_w2 += (double)v * (double)v;
            if (device_index != GSDR_WELCH_HOST) return;
            w.acc.assign((size_t)n_ch * 3 * (size_t)(nperseg / 2 + 1), 0.0);
            w.msum.assign((size_t)n_ch * 2, 0.0);
            w.tw.resize((size_t)nperseg);
            for (int k = 0; k < nperseg / 2; ++k) {
                const double a = 2.0 * M_PI * (double)k / (double)nperseg;
                w.tw[2 * (size_t)k] = std::cos(a), w.tw[2 * (size_t)k + 1] = -std::sin(a);
            }
        },
        gsdr_welch_dev_create_);
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
    if (const char *why = stage_host_fault(w, "a device object takes gsdr_welch_feed_device")) return stage_refuse(me, why);
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
    if (const char *why = stage_host_fault(w, "a device object takes gsdr_welch_read or gsdr_welch_read_device")) return stage_refuse(me, why);
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

}  // extern "C"
