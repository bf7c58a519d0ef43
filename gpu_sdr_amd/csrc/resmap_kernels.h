// resmap_kernels.h -- launch interface of the resonator-map kernel (internal; the contract: include/gsdr.h, "resonator
// map on the device"; the law: resmap_state.h; the design: DESIGN.md section 4.13).
#pragma once
#include <hip/hip_runtime.h>

#include "resmap_state.h"

namespace gsdr {

// One feed of n_rows >= 1 rows.
struct ResmapFeed {
    const float2 *rows;                  // [n_rows][n_ch]
    float2 *out;                         // [n_rows][n_out]; may be rows where channels is nullptr
    const gsdr_resmap_col *cols;         // [n_out]
    const double2 *offs;                 // [n_out]: (x0, y0)
    const int *channels;                 // [n_out], each in [0, n_ch); nullptr: the identity (n_out == n_ch)
    int n_rows, n_ch, n_out, kind;
};

// How lanes reach memory in one call; decided per call from the pointers and the counts (resmap_lanes_of).
enum ResmapLanes {
    kResmapSingle = 0,                   // a lane maps one sample: 8 bytes in, 8 bytes out
    kResmapPairOut = 1,                  // a lane maps two adjacent output columns: two 8-byte loads, one 16-byte store
    kResmapPair = 2,                     // identity list: one 16-byte load, one 16-byte store
};

struct ResmapPlan {
    int lanes;                           // ResmapLanes
    unsigned units;                      // column units per row: n_out, or n_out / 2 where a lane maps a pair
    unsigned row_step;                   // rows between two samples of one lane: the launch has units x row_step lanes
    unsigned blocks;                     // of 256
};

// the plan of a feed (no launch, no device call)
ResmapPlan resmap_plan_of(const ResmapFeed &f);

// resmap_kernel on st
hipError_t launch_resmap_feed(const ResmapFeed &f, hipStream_t st);

}  // namespace gsdr
