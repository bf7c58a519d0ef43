// stats_kernels.h -- launch interface of the row statistics' kernels (internal; the contract: include/gsdr.h, "row
// statistics on the device"; the laws: stats_state.h; the design: DESIGN.md section 4.14).
#pragma once
#include <hip/hip_runtime.h>

#include "stats_state.h"

namespace gsdr {

// The chain table of an object, [lanes][n_ch] in each of its four arrays (one allocation of 24 bytes per chain).
struct StatsChains {
    double *S, *Q;
    unsigned *mn, *mx;                   // bit patterns XOR kStatsMinEmpty / kStatsMaxEmpty (stats_state.h)
};

inline StatsChains stats_chains_at(void *base, size_t chains) {
    StatsChains t;
    t.S = static_cast<double *>(base), t.Q = t.S + chains;
    t.mn = reinterpret_cast<unsigned *>(t.Q + chains), t.mx = t.mn + chains;
    return t;
}

// One feed of n_rows >= 1 rows, stream rows [row0, row0 + n_rows).
struct StatsFeed {
    const float2 *rows;                  // [n_rows][n_ch], this feed
    const gsdr_stats_axis *axes;         // [n_ch]
    StatsChains chains;
    unsigned long long *counts;          // [n_ch][n_bins + 3]
    int n_rows, n_ch, n_bins, lanes;
    long long row0;
};

// stats_feed_kernel on st, in the shape stats_plan_of (stats_state.h) gives: `tile` channels by 256 / tile chains per
// workgroup, a grid of tiles x splits, lds_bytes of dynamic LDS
hipError_t launch_stats_feed(const StatsFeed &f, hipStream_t st);

// A read: the summaries and, with n_p > 0, the quantiles quant[n_ch][n_p].  Either output may be null.
struct StatsRead {
    const gsdr_stats_axis *axes;
    StatsChains chains;
    const unsigned long long *counts;
    int n_ch, n_bins, lanes;
    gsdr_stats_summary *summary;         // [n_ch]
    double *quant;                       // [n_ch][n_p]
    int n_p;
    double pr[GSDR_STATS_MAX_QUANTILES];
};

// stats_read_kernel on st
hipError_t launch_stats_read(const StatsRead &r, hipStream_t st);

}  // namespace gsdr
