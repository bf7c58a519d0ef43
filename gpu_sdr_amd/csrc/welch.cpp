// welch.cpp -- the device part of a welch object (the contract: include/gsdr.h, "Welch spectra on the device"): what
// it owns on the GPU and the sequencing of a feed and of a read.  Creation, the refusals of the arguments and the host
// twin are in welch_host.cpp, the kernels in welch_kernels.hip, the frame of every stage in stage_dev.h.
//
// A feed is three launches on the caller's stream (one when it completes no segment) and no host synchronisation.  What
// the HOST has to know of the stream is only the number of rows fed: from it follow the ring position of the feed, the
// segments it completes and where the first of them starts.  Nothing is read back.
#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "stage_dev.h"
#include "welch_kernels.h"

namespace gsdr {

struct WelchDev : StageDev {
    DevBuf<float2> hist;                     // [n_ch][H], H = nperseg - 1 + max_rows: the ring
    DevBuf<float> window;                    // nperseg
    DevBuf<float2> tw;                       // w_N^k, k < N, built in double as the PFB's table
    DevBuf<float> stage;                     // [max_segs][n_ch][3][K1]: a feed's segment spectra
    DevBuf<double> stage_mean;               // [max_segs][n_ch][2]
    DevBuf<double> acc;                      // [n_ch][3][K1]
    DevBuf<double> msum;                     // [n_ch][2]
    DevBuf<float> psd;                       // [n_ch][2][K1]: what gsdr_welch_read reads into
    DevBuf<float2> mean, gain;               // [n_ch] each, for gsdr_welch_read
    unsigned H = 0;
    long long max_segs = 0;
};

}  // namespace gsdr

using gsdr::refuse;
using gsdr::result;
using gsdr::set_device;
using gsdr::WelchDev;

namespace {

int count(long long n_seg) { return n_seg > INT_MAX ? INT_MAX : (int)n_seg; }

// nullptr or why a device entry cannot take this object
const char *object_fault(const gsdr_welch *w) {
    return gsdr::object_fault(w, "a host object (GSDR_WELCH_HOST) takes gsdr_welch_feed_host / gsdr_welch_read_host");
}

// psd and / or mean on st; the checks of the arguments are the callers'
hipError_t enqueue_read(const gsdr_welch *w, int mode, const float2 *gain_dev, double fs, float *psd_dev, float2 *mean_dev,
                        long long n_seg, hipStream_t st) {
    const WelchDev *d = static_cast<const WelchDev *>(w->dev);
    gsdr::WelchRead r{};
    r.n_ch = w->n_ch, r.nperseg = w->nperseg, r.mode = mode;
    r.rows_in = (double)n_seg * (double)w->step;
    r.scale = 1.0 / (fs * w->sum_w2 * (double)n_seg);
    r.acc = d->acc, r.msum = d->msum, r.gain = gain_dev, r.psd = psd_dev, r.mean = mean_dev;
    return gsdr::launch_welch_read(r, st);
}

const char *read_fault(int mode, const void *gain, double fs) {
    if (mode < GSDR_WELCH_RAW || mode > GSDR_WELCH_GAIN) return "mode must be GSDR_WELCH_RAW, _ROTATE, _DBC or _GAIN";
    if (!(fs > 0.0) || !std::isfinite(fs)) return "fs must be finite and > 0";
    if (mode == GSDR_WELCH_GAIN && !gain) return "gain must not be NULL with GSDR_WELCH_GAIN";
    return nullptr;
}

}  // namespace

extern "C" {

int gsdr_welch_dev_create_(gsdr_welch *w) {
    const char *const me = "gsdr_welch_create";
    const size_t N = (size_t)w->nperseg, K1 = N / 2 + 1, n_ch = (size_t)w->n_ch;
    const size_t H = N - 1 + (size_t)w->max_rows;
    const size_t max_segs = (size_t)w->max_rows / (size_t)w->step + 1;
    const size_t bytes = n_ch * H * sizeof(float2) + max_segs * n_ch * (3 * K1 * sizeof(float) + 2 * sizeof(double)) +
                         n_ch * (3 * K1 * sizeof(double) + 2 * sizeof(double) + 2 * K1 * sizeof(float) + 2 * sizeof(float2));
    const std::string asked = "(n_ch, max_rows, nperseg, step: " + std::to_string(bytes >> 20) + " MiB)";
    // a bound like those of welch_host.cpp (it is here for `asked`): decided before the device is touched
    if (max_segs * n_ch > (size_t)INT_MAX) return refuse(me, "n_ch x (max_rows / step + 1) segments per feed exceed 2^31 - 1 " + asked);
    std::vector<float2> tw(N);
    for (size_t k = 0; k < N; ++k) {
        const double a = -2.0 * M_PI * (double)k / (double)N;
        tw[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    return gsdr::create_dev<WelchDev>(w, me, asked, [&](WelchDev &d) {
        d.H = (unsigned)H, d.max_segs = (long long)max_segs;
        return d.hist.alloc(n_ch * H) == hipSuccess && d.window.upload(w->window) == hipSuccess && d.tw.upload(tw) == hipSuccess &&
               d.stage.alloc(max_segs * n_ch * 3 * K1) == hipSuccess && d.stage_mean.alloc(max_segs * n_ch * 2) == hipSuccess &&
               d.acc.alloc_zeroed(n_ch * 3 * K1) == hipSuccess && d.msum.alloc_zeroed(n_ch * 2) == hipSuccess &&
               d.psd.alloc(n_ch * 2 * K1) == hipSuccess && d.mean.alloc(n_ch) == hipSuccess && d.gain.alloc(n_ch) == hipSuccess;
    });
}

int gsdr_welch_dev_reset_(gsdr_welch *w) {
    const char *const me = "gsdr_welch_reset";
    if (!set_device(w)) return refuse(me, "hipSetDevice failed");
    WelchDev *d = static_cast<WelchDev *>(w->dev);
    const size_t K1 = (size_t)w->nperseg / 2 + 1, n_ch = (size_t)w->n_ch;
    // the ring needs no clearing: a young stream reads only rows it has written
    return result(me, gsdr::zero_behind_all({{d->acc, n_ch * 3 * K1 * sizeof(double)}, {d->msum, n_ch * 2 * sizeof(double)}}));
}

int gsdr_welch_feed_device(gsdr_welch *w, const gsdr_c64 *rows_dev, int n_rows, void *hip_stream) {
    const char *const me = "gsdr_welch_feed_device";
    if (const char *bad = object_fault(w)) return refuse(me, bad);
    if (n_rows < 0 || n_rows > w->max_rows) return refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows_dev) return refuse(me, "null buffer: rows_dev");
    if (!set_device(w)) return refuse(me, "hipSetDevice failed");
    WelchDev *d = static_cast<WelchDev *>(w->dev);
    const long long s0 = gsdr_welch_segments_of(w->total, w->nperseg, w->step);
    const long long s1 = gsdr_welch_segments_of(w->total + n_rows, w->nperseg, w->step);
    gsdr::WelchFeed f{};
    f.rows = reinterpret_cast<const float2 *>(rows_dev);
    f.n = n_rows, f.n_ch = w->n_ch, f.nperseg = w->nperseg, f.step = w->step, f.detrend = w->detrend;
    f.hist = d->hist, f.H = d->H;
    f.row_pos = (unsigned)(w->total % (long long)d->H);
    f.seg_pos = (unsigned)((s0 * (long long)w->step) % (long long)d->H);
    f.n_segs = (int)(s1 - s0);                       // <= max_rows / step + 1: the staging holds them
    f.window = d->window, f.tw = d->tw, f.stage = d->stage, f.stage_mean = d->stage_mean, f.acc = d->acc, f.msum = d->msum;
    if ((long long)f.n_segs > d->max_segs) return refuse(me, "internal: more segments than the staging holds");
    const hipError_t e = gsdr::launch_welch_feed(f, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return result(me, e);
    w->total += n_rows;
    return 0;
}

int gsdr_welch_read_device(gsdr_welch *w, int mode, const gsdr_c64 *gain_dev, double fs, float *psd_dev, void *hip_stream) {
    const char *const me = "gsdr_welch_read_device";
    if (const char *bad = object_fault(w)) return refuse(me, bad);
    if (const char *bad = read_fault(mode, gain_dev, fs)) return refuse(me, bad);
    if (!psd_dev) return refuse(me, "null buffer: psd_dev");
    const long long n_seg = gsdr_welch_segments_of(w->total, w->nperseg, w->step);
    if (n_seg == 0) return 0;
    if (!set_device(w)) return refuse(me, "hipSetDevice failed");
    const hipError_t e = enqueue_read(w, mode, reinterpret_cast<const float2 *>(gain_dev), fs, psd_dev, nullptr, n_seg,
                                      static_cast<hipStream_t>(hip_stream));
    return result(me, e, count(n_seg));
}

int gsdr_welch_mean_device(gsdr_welch *w, gsdr_c64 *mean_dev, void *hip_stream) {
    const char *const me = "gsdr_welch_mean_device";
    if (const char *bad = object_fault(w)) return refuse(me, bad);
    if (!mean_dev) return refuse(me, "null buffer: mean_dev");
    const long long n_seg = gsdr_welch_segments_of(w->total, w->nperseg, w->step);
    if (n_seg == 0) return 0;
    if (!set_device(w)) return refuse(me, "hipSetDevice failed");
    const hipError_t e = enqueue_read(w, GSDR_WELCH_RAW, nullptr, 1.0, nullptr, reinterpret_cast<float2 *>(mean_dev), n_seg,
                                      static_cast<hipStream_t>(hip_stream));
    return result(me, e, count(n_seg));
}

int gsdr_welch_read(gsdr_welch *w, int mode, const gsdr_c64 *gain_host, double fs, float *psd_host, gsdr_c64 *mean_host,
                    void *hip_stream) {
    const char *const me = "gsdr_welch_read";
    if (const char *bad = object_fault(w)) return refuse(me, bad);
    if (const char *bad = read_fault(mode, gain_host, fs)) return refuse(me, bad);
    if (!psd_host) return refuse(me, "null buffer: psd_host");
    const long long n_seg = gsdr_welch_segments_of(w->total, w->nperseg, w->step);
    if (n_seg == 0) return 0;
    if (!set_device(w)) return refuse(me, "hipSetDevice failed");
    WelchDev *d = static_cast<WelchDev *>(w->dev);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const size_t n_ch = (size_t)w->n_ch, K1 = (size_t)w->nperseg / 2 + 1;
    hipError_t e = hipSuccess;
    if (mode == GSDR_WELCH_GAIN) {
        // the source is the caller's pageable or pinned memory: wait for the copy, the caller may reuse it at once
        e = hipMemcpyAsync(d->gain, gain_host, n_ch * sizeof(gsdr_c64), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e == hipSuccess) e = enqueue_read(w, mode, d->gain, fs, d->psd, d->mean, n_seg, st);
    e = gsdr::fetch(e, st, {{psd_host, d->psd, n_ch * 2 * K1 * sizeof(float)}, {mean_host, d->mean, n_ch * sizeof(gsdr_c64)}});
    return result(me, e, count(n_seg));
}

}  // extern "C"
