// sweep_host.cpp -- the VNA sweep accumulator's creation, counts, host twin and two helpers (the contract:
// include/gsdr.h, "VNA sweep accumulator on the device"; the fold: sweep_state.h).  The host twin walks the rows in
// stream order; every addition, the division, the fma of the variance and the block order of the slope are the ones
// sweep_kernels.hip makes, so the bits are the same.  No HIP here.
#include <algorithm>
#include <cmath>
#include <vector>

#include "stage_host.h"
#include "sweep_state.h"

extern "C" {

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
    std::string bad;
    if (n_ch < 1 || n_ch > (1 << 20)) bad = "n_ch must be in [1, 1048576]";
    else if (n_points < 1 || n_points > (1LL << 24)) bad = "n_points must be in [1, 16777216]";
    else if (n_points * (long long)n_ch > (1LL << 25)) bad = "n_points * n_ch must be <= 33554432 (32 bytes each)";
    else if (group < 1 || group > (1LL << 30)) bad = "group must be in [1, 1073741824]";
    else if (first_row < 0 || first_row > (1LL << 62)) bad = "first_row must be in [0, 2^62]";
    else bad = stage_device_fault(device_index, "GSDR_SWEEP_HOST", gsdr_sweep_dev_create_ != nullptr);
    const size_t cells = (size_t)n_points * (size_t)n_ch;
    return stage_create<gsdr_sweep>(
        "gsdr_sweep_create", bad, device_index, "n_ch and n_points: no host memory for the accumulators (" + std::to_string((cells * 32) >> 20) + " MiB)",
        [&](gsdr_sweep &s) {
            s.n_ch = n_ch, s.n_points = n_points, s.group = group, s.first_row = first_row;
            if (device_index == GSDR_SWEEP_HOST) s.acc.assign(cells * 4, 0.0);
        },
        gsdr_sweep_dev_create_);
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
    GSDR_NO_CONTRACT_BODY
    const char *const me = "gsdr_sweep_feed_host";
    if (const char *why = stage_host_fault(s, "a device object takes gsdr_sweep_feed_device")) return stage_refuse(me, why);
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
    GSDR_NO_CONTRACT_BODY
    const char *const me = "gsdr_sweep_read_host";
    if (const char *why = stage_host_fault(s, "a device object takes gsdr_sweep_read or gsdr_sweep_read_device")) return stage_refuse(me, why);
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
    GSDR_NO_CONTRACT_BODY
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
    GSDR_NO_CONTRACT_BODY
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

}  // extern "C"
