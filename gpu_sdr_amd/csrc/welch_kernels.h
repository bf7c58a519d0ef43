// welch_kernels.h -- launch interface of the Welch kernels (internal; the contract: include/gsdr.h, "Welch spectra on
// the device"; the design: DESIGN.md section 4.10).
#pragma once
#include <hip/hip_runtime.h>

#include "welch_state.h"

namespace gsdr {

// One feed of n >= 1 rows.  The HISTORY is a ring of H = nperseg - 1 + max_rows samples per channel, channel-major:
// stream row r of channel c sits at hist[c * H + r % H].  A feed overwrites only rows older than any segment still
// to come, so no kernel reads what another workgroup of the same launch writes.
struct WelchFeed {
    const float2 *rows;                  // [n][n_ch], this feed
    int n, n_ch, nperseg, step, detrend;
    float2 *hist;                        // [n_ch][H]
    unsigned H;
    unsigned row_pos;                    // ring position of rows[0]: total % H
    unsigned seg_pos;                    // ring position of the first row of the first segment this feed completes
    int n_segs;                          // segments this feed completes (may be 0: only the append runs)
    const float *window;                 // nperseg
    const float2 *tw;                    // w_N^k, k < N
    float *stage;                        // [n_segs][n_ch][3][N/2+1]: this feed's segment spectra
    double *stage_mean;                  // [n_segs][n_ch][2]
    double *acc;                         // [n_ch][3][N/2+1]
    double *msum;                        // [n_ch][2]
};

// welch_append_kernel, then (n_segs > 0) welch_segment_kernel and welch_accumulate_kernel on st, in that order
hipError_t launch_welch_feed(const WelchFeed &f, hipStream_t st);

struct WelchRead {
    int n_ch, nperseg, mode;
    double rows_in;                      // n_seg * step
    double scale;                        // 1 / (fs * sum w^2 * n_seg)
    const double *acc, *msum;
    const float2 *gain;                  // GSDR_WELCH_GAIN
    float *psd;                          // [n_ch][2][N/2+1], or nullptr
    float2 *mean;                        // [n_ch], or nullptr
};

// welch_read_kernel: psd and / or mean from the accumulators
hipError_t launch_welch_read(const WelchRead &r, hipStream_t st);

}  // namespace gsdr
