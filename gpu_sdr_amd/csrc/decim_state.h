// decim_state.h -- the FIR decimator (include/gsdr.h, "FIR decimation on the device") as decim_host.cpp and decim.cpp
// share it.  decim_host.cpp owns creation, the refusals, the default taps, the count law and the host twin; decim.cpp
// hangs the device part on `dev` through the hook below (its release: stage_state.h).  No HIP here: decim_host.cpp is built without decim.cpp by a host
// compiler (tests/test_decim_sanitizers.py), where the hooks are absent and only host objects exist.
//
// Blocks.  The contract's block B is the q rows that end on row B q + p.  Both sides count blocks from the one that
// holds stream row 0: k = B + p/q >= 0, whose first row is k q + r0 with r0 = p % q + 1 - q in (-q, 0].  Output o is
// complete with block k = o + p/q, and takes chunk j from block k - j (a block k - j < 0 lies before the stream: +0).
// The RING holds the chunk sums of the last ring_blocks blocks, [k % ring_blocks][j][channel]: the open block's
// unfinished sums and the finished ones of every block an output still to come needs.
#ifndef GSDR_DECIM_STATE_H
#define GSDR_DECIM_STATE_H

#include <vector>

#include "../../include/gsdr.h"
#include "stage_state.h"

struct gsdr_decim {
    int n_ch = 0, max_rows = 0, q = 0, n_taps = 0;
    int F = 0;                                // chunks per output: ceil(n_taps / q)
    long long offset = 0;
    int device = GSDR_DECIM_HOST;
    long long total = 0;                      // rows fed since creation / reset
    long long ring_blocks = 0;                // (max_rows - 1)/q + 2 + F
    std::vector<float> taps;
    std::vector<gsdr_c64> ring;               // host twin: [ring_blocks][F][n_ch]
    gsdr::StageDev *dev = nullptr;            // gsdr::DecimDev (decim.cpp)
};

// output rows complete after `total` rows
inline long long gsdr_decim_out_of(long long total, long long offset, int q) {
    return total <= offset ? 0 : (total - 1 - offset) / q + 1;
}
// first row of block 0 (see above); the block of row r >= 0 is (r - r0) / q
inline long long gsdr_decim_r0(long long offset, int q) { return offset % q + 1 - q; }

extern "C" {
// decim.cpp; weak in decim_host.cpp.  _create_: allocates and uploads, 0 or -1 with the message noted; it is called
// after every bound has been checked.
int gsdr_decim_dev_create_(gsdr_decim *d);
}

#endif
