// trigger_kernels.h -- launch interface of the trigger kernels (internal; the contract: include/gsdr.h, "trigger on the
// device"; the design: DESIGN.md section 4.9).
#pragma once
#include <hip/hip_runtime.h>

#include "trigger_state.h"

namespace gsdr {

// One feed of n >= 1 rows.  The WINDOW of a feed is the records of the last P = post - 1 rows before it followed by
// those of its n rows: entry j is stream row R0 - P + j.  flags: bit 0 the row hits, bit 1 it is a trigger.
struct TriggerFeed {
    const float2 *rows;                  // [n][n_ch], this feed
    int n, n_ch, pre, post, holdoff, max_events;
    long long R0;                        // stream row of rows[0]
    int n_prev;                          // rows of the feed before (its window has P + n_prev entries)
    int rec_valid;                       // carried records that exist: min(R0, P)
    const float *levels;                 // [n_ch][6]
    const gsdr_trigger_rec *rec_in;      // window of the feed before
    const unsigned char *flag_in;
    gsdr_trigger_rec *rec_out;           // window of this feed, P + n entries
    unsigned char *flag_out;
    long long *last_hit;                 // the last hitting row before the window's new rows; read when R0 > 0, then updated
    const float2 *carry_in;              // [K][n_ch], K = pre + post - 1: rows R0 - K .. R0 - 1
    float2 *carry_out;                   // the same for the next feed
    gsdr_trigger_event *events;          // out, max_events
    float2 *snippets;                    // out, max_events x (pre + post) x n_ch
    int *counts;                         // out, {n_events, n_dropped}
};

// trigger_hits_kernel, trigger_select_kernel, trigger_capture_kernel on st, in that order
hipError_t launch_trigger_feed(const TriggerFeed &f, hipStream_t st);

}  // namespace gsdr
