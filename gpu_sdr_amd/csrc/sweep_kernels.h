// sweep_kernels.h -- launch interface of the VNA sweep accumulator's kernels (internal; the contract: include/gsdr.h,
// "VNA sweep accumulator on the device"; the fold: sweep_state.h; the design: DESIGN.md section 4.12).
#pragma once
#include <hip/hip_runtime.h>

#include "sweep_state.h"

namespace gsdr {

// One feed of n >= 1 rows, stream rows [row0, row0 + n).
struct SweepFeed {
    const float2 *rows;                  // [n][n_ch], this feed
    double *acc;                         // [n_points][n_ch][4]
    int n, n_ch;
    long long n_points, group;
    long long row0;                      // stream number of the feed's first row
};

// sweep_accumulate_kernel on st
hipError_t launch_sweep_feed(const SweepFeed &f, hipStream_t st);

// What a read and the slope need: the accumulators and the two ends of the stream so far.
struct SweepRead {
    const double *acc;
    int n_ch;
    long long n_points, group;
    gsdr_sweep_edge a, b;                // of first_row and of first_row + total
};

// sweep_read_kernel on st: mean[n_points][n_ch] and, where var is not null, var[n_points][n_ch]
hipError_t launch_sweep_read(const SweepRead &r, float2 *mean, float2 *var, hipStream_t st);

// sweep_slope_block_kernel, then sweep_slope_combine_kernel on st: blocks[gsdr_sweep_slope_blocks(n_points)][n_ch] is
// scratch, d[n_ch] complex128 the result
hipError_t launch_sweep_slope(const SweepRead &r, double2 *blocks, double2 *d, hipStream_t st);

}  // namespace gsdr
