// decim_kernels.h -- launch interface of the FIR decimation kernels (internal; the contract: include/gsdr.h, "FIR
// decimation on the device"; the blocks and the ring: decim_state.h; the design: DESIGN.md section 4.11).
#pragma once
#include <hip/hip_runtime.h>

#include "decim_state.h"

namespace gsdr {

constexpr int kDecimTapsPad = 8;         // floats behind the taps that decim_partial_kernel may load

// One feed of n >= 1 rows, stream rows [first_row, first_row + n).
struct DecimFeed {
    const float2 *rows;                  // [n][n_ch], this feed
    float2 *out;                         // [n_emit][n_ch]
    float2 *ring;                        // [ring_blocks][F][n_ch]: chunk sums per block
    const float *taps;                   // [F q + kDecimTapsPad]: tap t at taps[t + F q - T]; the padding in front and
                                         // behind is loaded but never multiplied
    int n, n_ch, q, T, F;
    unsigned ring_blocks;
    long long first_row;                 // rows fed before this feed
    long long r0;                        // first row of block 0: offset % q + 1 - q
    int n_emit;                          // output rows this feed completes (may be 0: only the partial sums run)
    long long k_out;                     // block of the first of them
};

// decim_partial_kernel, then (n_emit > 0) decim_combine_kernel on st, in that order
hipError_t launch_decim_feed(const DecimFeed &f, hipStream_t st);

// chunks per thread decim_partial_kernel takes for F chunks per output (1, 3 or 7)
int decim_chunks_per_thread(int F);

}  // namespace gsdr
