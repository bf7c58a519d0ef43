// stats_host.cpp -- the row statistics' creation, axes, host twin, quantiles and levels (the contract: include/gsdr.h,
// "row statistics on the device"; the laws: stats_state.h).  The twin calls the functions stats_feed_kernel and
// stats_read_kernel (stats_kernels.hip) call, walks every chain in stream order and joins the chains by the halving
// tree as it is written in the header: the bits are the same.  The levels are made HERE for both kinds of object, from
// the summaries and the medians a read returns: one text, one sqrt.  No HIP here.
#include <algorithm>
#include <cmath>
#include <vector>

#include "stage_host.h"
#include "stats_state.h"

extern "C" {
int gsdr_stats_dev_create_(gsdr_stats *s) __attribute__((weak));
int gsdr_stats_dev_reset_(gsdr_stats *s, int upload) __attribute__((weak));
int gsdr_stats_dev_fetch_(gsdr_stats *s, const char *entry, gsdr_stats_summary *summary, const double *pr, int n_p, double *quantiles,
                          unsigned long long *counts, void *hip_stream) __attribute__((weak));
}

namespace {
// "" or what is wrong with the axes; the tables' entries into out
GSDR_NO_CONTRACT
std::string stats_axes_of(const gsdr_trigger_level *axes, int n_ch, int n_bins, std::vector<gsdr_stats_axis> &out) {
    GSDR_NO_CONTRACT_BODY
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
    std::string bad;
    std::vector<gsdr_stats_axis> table;
    if (n_ch < 1 || n_ch > (1 << 20)) bad = "n_ch must be in [1, 1048576]";
    else if (max_rows < 1 || max_rows > (1 << 20)) bad = "max_rows must be in [1, 1048576]";
    else if (n_bins < 1 || n_bins > GSDR_STATS_MAX_BINS) bad = "n_bins must be in [1, 4096]";
    else if (lanes < 0 || lanes > GSDR_STATS_MAX_LANES || (lanes & (lanes - 1)) != 0) bad = "lanes must be 0 or a power of two in [1, 32768]";
    else if (!axes) bad = "axes must not be NULL";
    else bad = stage_device_fault(device_index, "GSDR_STATS_HOST", gsdr_stats_dev_create_ != nullptr);
    try {
        if (bad.empty()) bad = stats_axes_of(axes, n_ch, n_bins, table);
    } catch (const std::bad_alloc &) {
        bad = "n_ch: no host memory for the axes";
    }
    const int n_lanes = lanes ? lanes : gsdr_stats_lanes_rule(n_ch, max_rows);
    const size_t chains = (size_t)n_lanes * (size_t)n_ch, counters = (size_t)n_ch * ((size_t)n_bins + 3);
    return stage_create<gsdr_stats>(
        "gsdr_stats_create", bad, device_index,
        "n_ch, lanes and n_bins: no host memory for the chains and the counters (" + std::to_string((chains * 24 + counters * 8) >> 20) + " MiB)",
        [&](gsdr_stats &s) {
            s.n_ch = n_ch, s.max_rows = max_rows, s.n_bins = n_bins, s.lanes = n_lanes;
            s.axes.swap(table);
            if (device_index != GSDR_STATS_HOST) return;
            s.chains.assign(chains, gsdr_stats_chain{0.0, 0.0, HUGE_VALF, -HUGE_VALF});
            s.counts.assign(counters, 0ULL);
        },
        gsdr_stats_dev_create_);
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
    GSDR_NO_CONTRACT_BODY
    const char *const me = "gsdr_stats_feed_host";
    if (const char *why = stage_host_fault(s, "a device object takes gsdr_stats_feed_device")) return stage_refuse(me, why);
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
    if (const char *why = stage_host_fault(s, "a device object takes gsdr_stats_read or gsdr_stats_read_device")) return stage_refuse(me, why);
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
    GSDR_NO_CONTRACT_BODY
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
