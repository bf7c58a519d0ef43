// sweep_state.h -- the VNA sweep accumulator (include/gsdr.h, "VNA sweep accumulator on the device") as sweep_host.cpp,
// sweep.cpp and sweep_kernels.hip share it: the closed forms of the fold.  sweep_host.cpp owns creation, the refusals,
// the counts and the host twin; sweep.cpp hangs the device part on `dev` through the hooks below (its release: stage_state.h).  No HIP here:
// sweep_host.cpp is built without sweep.cpp by a host compiler (tests/test_sweep_sanitizers.py), where the hooks are absent and
// only host objects exist.
//
// The fold.  Stream row r lies in GROUP r / group, and group G belongs to point G mod n_points.  One PASS is
// W = n_points * group rows (<= 2^54).  Every count below is a difference of "rows of point p in [0, x)", which needs
// x / W and x mod W only: the host divides once, the read kernel gets both and compares.
#ifndef GSDR_SWEEP_STATE_H
#define GSDR_SWEEP_STATE_H

#include <vector>

#include "../../include/gsdr.h"
#include "stage_state.h"

#if defined(__HIPCC__)
#define GSDR_SWEEP_HD __host__ __device__ inline
#else
#define GSDR_SWEEP_HD inline
#endif

struct gsdr_sweep {
    int n_ch = 0;
    long long n_points = 0, group = 0;
    long long first_row = 0;                  // stream number of the first row fed since creation / reset
    long long total = 0;                      // rows fed since creation / reset
    int device = GSDR_SWEEP_HOST;
    std::vector<double> acc;                  // host twin: [n_points][n_ch][S.re, S.im, Q.re, Q.im]
    gsdr::StageDev *dev = nullptr;            // gsdr::SweepDev (sweep.cpp)
};

constexpr long long kSweepSlopeBlock = 256;   // consecutive terms of the phase slope that are summed into one block sum

// x as passes and rest: what the counts need of an end of the stream
struct gsdr_sweep_edge {
    long long passes, rest;                   // x / W, x mod W
};

inline gsdr_sweep_edge gsdr_sweep_edge_of(long long x, long long n_points, long long group) {
    const long long W = n_points * group;
    return gsdr_sweep_edge{x / W, x % W};
}

// rows of point p among stream rows [0, x)
GSDR_SWEEP_HD long long gsdr_sweep_rows_below(gsdr_sweep_edge x, long long p, long long group) {
    const long long in = x.rest - p * group;
    return x.passes * group + (in < 0 ? 0 : (in > group ? group : in));
}

// n[p]: rows of point p among stream rows [a, b)
GSDR_SWEEP_HD long long gsdr_sweep_rows_of(gsdr_sweep_edge a, gsdr_sweep_edge b, long long p, long long group) {
    return gsdr_sweep_rows_below(b, p, group) - gsdr_sweep_rows_below(a, p, group);
}

// min over p of n[p]: n[.] is constant between the points the two ends lie in, so the points around them and the two
// outermost are all that can hold the minimum
inline long long gsdr_sweep_min_rows(long long first_row, long long total, long long n_points, long long group) {
    const gsdr_sweep_edge a = gsdr_sweep_edge_of(first_row, n_points, group), b = gsdr_sweep_edge_of(first_row + total, n_points, group);
    const long long pa = a.rest / group, pb = b.rest / group;
    const long long at[8] = {0, n_points - 1, pa - 1, pa, pa + 1, pb - 1, pb, pb + 1};
    long long least = -1;
    for (long long p : at) {
        if (p < 0 || p >= n_points) continue;
        const long long n = gsdr_sweep_rows_of(a, b, p, group);
        if (least < 0 || n < least) least = n;
    }
    return least;
}

// What a feed of n >= 1 rows, stream rows [R, R + n), touches: the groups [g0, g1], on min(g1 - g0 + 1, n_points)
// points from p0 on (cyclically).  Slot t of the feed takes the groups g0 + t, g0 + t + n_points, ... up to g1, in that
// order: each accumulator has one owner and sees its rows in stream order.  rel0 is the feed row on which group g0
// begins, in (-group, 0].
struct gsdr_sweep_span {
    long long touched, p0, rel0;
};

inline gsdr_sweep_span gsdr_sweep_span_of(long long R, long long n, long long n_points, long long group) {
    const long long g0 = R / group, g1 = (R + n - 1) / group, ng = g1 - g0 + 1;
    return gsdr_sweep_span{ng < n_points ? ng : n_points, g0 % n_points, g0 * group - R};
}

// block sums of the phase slope over n_points - 1 terms (one block, of +0, where there is no term)
inline long long gsdr_sweep_slope_blocks(long long n_points) {
    return n_points < 2 ? 1 : (n_points - 1 + kSweepSlopeBlock - 1) / kSweepSlopeBlock;
}

extern "C" {
// sweep.cpp; weak in sweep_host.cpp.  _create_: allocates and zeroes, 0 or -1 with the message noted; it is called
// after every bound has been checked.  _reset_: waits for the device and zeroes the accumulators.  _slope_: the slope
// kernels on the stream, waits, copies n_ch complex128.
int gsdr_sweep_dev_create_(gsdr_sweep *s);
int gsdr_sweep_dev_reset_(gsdr_sweep *s);
int gsdr_sweep_dev_slope_(gsdr_sweep *s, double *d_host, void *hip_stream);
}

#endif
