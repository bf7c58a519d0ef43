// stats_state.h -- the row statistics (include/gsdr.h, "row statistics on the device") as stats_host.cpp, stats.cpp and
// stats_kernels.hip share them: the object, a channel's axis as the tables hold it, a chain, and THE LAWS -- the
// per-sample law, the combination of two chains, the summary and the quantile -- as inline host-and-device functions
// that the kernels and the host twin both include: there is one text of the arithmetic -- and the launch rule of a feed
// (stats_plan_of), which the launcher and gsdr_stats_plan both ask.  stats_host.cpp owns creation,
// the refusals, the lanes rule, the levels and the host twin; stats.cpp hangs the device part on `dev` through the hooks
// below (its release: stage_state.h).  No HIP here: stats_host.cpp is built without stats.cpp by a host compiler
// (tests/test_stats_sanitizers.py), where the hooks are absent and only host objects exist.
//
// No law below has a product that feeds an addition in one expression: every product is stored first, and contraction
// is off wherever these functions are compiled (the pragma for clang, GSDR_STATS_NO_CONTRACT for gcc).
#ifndef GSDR_STATS_STATE_H
#define GSDR_STATS_STATE_H

#include <vector>

#include "../../include/gsdr.h"
#include "stage_state.h"

#define GSDR_STATS_HD GSDR_STAGE_HD

// one channel's axis, 48 bytes: what the device table and the twin hold
struct gsdr_stats_axis {
    float bx, by, dx, dy, lo, hi;
    double p, inv_w, w;                       // the pivot, n_bins / (hi - lo), (hi - lo) / n_bins
};
static_assert(sizeof(gsdr_stats_axis) == 48, "an axis of the table is 6 floats and 3 doubles");

// one chain of one channel
struct gsdr_stats_chain {
    double S, Q;
    float mn, mx;
};

// The chain table keeps min and max as their bit patterns XOR those of +Inf and -Inf: a zeroed table is a table of
// empty chains (S = Q = +0, min = +Inf, max = -Inf), which is all a reset has to write.
constexpr unsigned kStatsMinEmpty = 0x7f800000u, kStatsMaxEmpty = 0xff800000u;

constexpr int kStatsChainTarget = 65536;      // chains x channels the lanes rule aims at: 256 per compute unit

static_assert(sizeof(gsdr_stats_summary) == 64, "a summary is 64 bytes");

struct gsdr_stats {
    int n_ch = 0, max_rows = 0, n_bins = 0, lanes = 0;
    long long total = 0;                      // rows fed since creation / reset
    int device = GSDR_STATS_HOST;
    std::vector<gsdr_stats_axis> axes;        // [n_ch]
    std::vector<gsdr_stats_chain> chains;     // host twin: [lanes][n_ch]
    std::vector<unsigned long long> counts;   // host twin: [n_ch][n_bins + 3]
    gsdr::StageDev *dev = nullptr;            // gsdr::StatsDev (stats.cpp)
};

// lanes == 0 of gsdr_stats_create: the smallest power of two that gives kStatsChainTarget chains over all channels, but
// no more chains than a feed of max_rows rows can give a row each, and at most GSDR_STATS_MAX_LANES
inline int gsdr_stats_lanes_rule(int n_ch, int max_rows) {
    int lanes = 1;
    while (lanes < GSDR_STATS_MAX_LANES && (long long)lanes * n_ch < kStatsChainTarget && 2 * lanes <= max_rows) lanes *= 2;
    return lanes;
}

// THE LAUNCH RULE of a feed (stats_kernels.hip launches what it says and decides nothing itself; gsdr_stats_plan gives
// the same answer without a GPU; tests/test_stats_host.py pins it at its edges).  A workgroup of 256 threads owns `tile`
// channels by 256 / tile chains and counts the bins in an LDS table [tile][n_bins + 3] of 32-bit counters; the grid is
// tiles x splits.
namespace gsdr {

constexpr int kStatsMaxTile = 32;        // channels of a workgroup: 256 bytes of a row per wave-instruction
constexpr unsigned kStatsMaxLds = 65536; // bytes of the table a workgroup may ask for
constexpr int kStatsMaxSplits = 65535;   // the grid's y

struct StatsPlan {
    int tile, tiles, splits;
    unsigned lds_bytes;                  // tile x (n_bins + 3) counters of 32 bits
};

// what gsdr_stats_create accepts of the three (a lanes of 0 has become the rule's value by then)
inline bool stats_shape_ok(int n_ch, int n_bins, int lanes) {
    return n_ch >= 1 && n_ch <= (1 << 20) && n_bins >= 1 && n_bins <= GSDR_STATS_MAX_BINS && lanes >= 1 && lanes <= GSDR_STATS_MAX_LANES &&
           (lanes & (lanes - 1)) == 0;
}

inline StatsPlan stats_plan_of(int n_ch, int n_bins, int lanes) {
    StatsPlan p{};
    const unsigned per_channel = (unsigned)(n_bins + 3) * (unsigned)sizeof(unsigned);     // <= 16396
    p.tile = 1;
    // as many channels as the table has room for, no more than there are, at most kStatsMaxTile
    while (2 * p.tile <= kStatsMaxTile && (unsigned)(2 * p.tile) * per_channel <= kStatsMaxLds && 2 * p.tile <= n_ch) p.tile *= 2;
    p.tiles = (n_ch + p.tile - 1) / p.tile;
    const int chains = 256 / p.tile;
    p.splits = (lanes + chains - 1) / chains;
    p.lds_bytes = (unsigned)p.tile * per_channel;
    return p;
}

}  // namespace gsdr

GSDR_STATS_HD bool gsdr_stats_finite(float q) { return __builtin_fabsf(q) <= 3.402823466e+38f; }

// The per-sample law: q, and the counter of counts[c] the sample belongs to (n_bins + 2: bad).
GSDR_STATS_HD int gsdr_stats_sample(const gsdr_stats_axis &a, int n_bins, float x, float y, float &q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    q = gsdr_stage_project(a.bx, a.by, a.dx, a.dy, x, y);
    if (!gsdr_stats_finite(q)) return n_bins + 2;
    if (q < a.lo) return 0;
    const double off = (double)q - (double)a.lo;
    const double pos = off * a.inv_w;
    const double k = __builtin_floor(pos);
    return k >= (double)n_bins ? n_bins + 1 : 1 + (int)k;
}

// a finite q enters its chain
GSDR_STATS_HD void gsdr_stats_chain_add(gsdr_stats_chain &s, double p, float q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double d = (double)q - p;
    const double dd = d * d;
    s.S = s.S + d;
    s.Q = s.Q + dd;
    s.mn = q < s.mn ? q : s.mn;
    s.mx = q > s.mx ? q : s.mx;
}

// s[j] (+) s[j + h] of the halving tree: a is the earlier
GSDR_STATS_HD gsdr_stats_chain gsdr_stats_chain_join(const gsdr_stats_chain &a, const gsdr_stats_chain &b) {
    gsdr_stats_chain r;
    r.S = a.S + b.S;
    r.Q = a.Q + b.Q;
    r.mn = b.mn < a.mn ? b.mn : a.mn;
    r.mx = b.mx > a.mx ? b.mx : a.mx;
    return r;
}

// the summary of one channel from its joined chains and its counters; `bins` is the sum of the n_bins bins
GSDR_STATS_HD gsdr_stats_summary gsdr_stats_summarise(const gsdr_stats_chain &s, double p, unsigned long long under, unsigned long long bins,
                                                       unsigned long long over, unsigned long long bad) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    gsdr_stats_summary o;
    o.n = under + bins + over, o.bad = bad, o.under = under, o.over = over;
    const double nan = __builtin_nan("");
    o.mean = nan, o.var = nan;
    o.min = s.mn, o.max = s.mx;
    for (int i = 0; i < 8; ++i) o.reserved[i] = 0;
    if (o.n >= 1) {
        const double n = (double)o.n;
        const double m = s.S / n;
        o.mean = p + m;
        if (o.n >= 2) {
            const double sm = s.S * m;
            const double num = s.Q - sm;
            const double v = num / (n - 1.0);
            o.var = v < 0.0 ? 0.0 : v;                 // a NaN is not < 0: it stays
        }
    }
    return o;
}

// the rank of quantile pr among n >= 1 samples
GSDR_STATS_HD unsigned long long gsdr_stats_rank(double pr, unsigned long long n) {
    const double t = __builtin_ceil(pr * (double)n);
    return t < 1.0 ? 1ULL : (unsigned long long)t;
}

// the quantile of rank t that falls into bin k, which holds h >= 1 samples behind C below it (C < t <= C + h)
GSDR_STATS_HD double gsdr_stats_in_bin(const gsdr_stats_axis &a, int k, unsigned long long t, unsigned long long C, unsigned long long h) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double up = (double)(t - C) - 0.5;
    const double frac = up / (double)h;
    const double at = (double)k + frac;
    const double span = at * a.w;
    return (double)a.lo + span;
}

extern "C" {
// stats.cpp; weak in stats_host.cpp.  _create_: allocates, zeroes and uploads s->axes, 0 or -1 with the message noted;
// called after every bound has been checked.  _reset_: waits for the device, zeroes the chains and the counters,
// uploads s->axes where `upload` is set, waits.  _fetch_: on the stream a read with the n_p quantiles pr, waits and
// copies what is asked for (each of the three may be NULL).
int gsdr_stats_dev_create_(gsdr_stats *s);
int gsdr_stats_dev_reset_(gsdr_stats *s, int upload);
int gsdr_stats_dev_fetch_(gsdr_stats *s, const char *entry, gsdr_stats_summary *summary, const double *pr, int n_p, double *quantiles,
                          unsigned long long *counts, void *hip_stream);
}

#endif
