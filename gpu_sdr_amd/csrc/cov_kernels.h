// cov_kernels.h -- launch interface of the channel covariance's kernels (internal; the contract: include/gsdr.h, "channel
// covariance on the device"; the laws: cov_state.h; the design: DESIGN.md section 4.15).
#pragma once
#include <hip/hip_runtime.h>

#include "cov_state.h"

namespace gsdr {

// The sums of an object on the device.  S is [lanes][n_var].  G is [lanes][pairs][tile][tile]: the pair (I >= J) of tiles
// at I (I + 1) / 2 + J holds the cell (I tile + il, J tile + jl) at il tile + jl -- whole squares, so that a workgroup of
// the accumulate pass loads and stores one contiguous block; of a diagonal pair only jl <= il is ever read.
inline size_t cov_g_doubles(const CovPlan &p) { return (size_t)p.lanes * (size_t)p.pairs * (size_t)p.tile * (size_t)p.tile; }

// One feed of n_rows >= 1 rows, stream rows [row0, row0 + n_rows).
struct CovFeed {
    const float2 *rows;                  // [n_rows][n_ch], this feed
    const gsdr_cov_axis *axes;           // [n_var]
    double *D;                           // [max_rows][n_var]: the projected rows of this feed
    double *S, *G;
    int n_rows, n_ch, n_var, lanes;
    long long row0;
};

// cov_project_kernel and cov_accumulate_kernel on st, in the shapes cov_plan_of (cov_state.h) gives
hipError_t launch_cov_feed(const CovFeed &f, hipStream_t st);

// A read of `kind` after n rows: out[n_var][n_var] and, where not null, mean[n_var].
struct CovRead {
    const gsdr_cov_axis *axes;
    const double *S, *G;
    int n_var, lanes, kind;
    long long n;
    double *out, *mean;
};

// cov_read_kernel on st
hipError_t launch_cov_read(const CovRead &r, hipStream_t st);

}  // namespace gsdr
