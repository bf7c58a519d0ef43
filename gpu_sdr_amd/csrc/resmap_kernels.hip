// resmap_kernels.hip -- the resonator map on demodulated rows (the contract: include/gsdr.h, "resonator map on the
// device"; the law: gsdr_resmap_sample, resmap_state.h; the design: DESIGN.md section 4.13).  One launch per feed:
//   resmap_kernel<KIND, LANES>  a lane owns one COLUMN UNIT -- one output column, or two adjacent ones where this
//                               call's output pointer is 16-byte aligned and n_out is even -- and walks rows.  The
//                               launch has units x row_step lanes, the unit running fastest: lane g takes unit
//                               g mod units and the rows g / units, + row_step, + 2 row_step, ...  A lane therefore keeps
//                               its columns: their constants and offsets come out of the tables once, before the loop,
//                               and stay in registers.  Adjacent lanes hold adjacent units of one row, then the next
//                               row: with the identity list a wave reads and writes one contiguous run whatever the
//                               row length -- 2 048 columns (a wave inside one row) or 4 (a wave across 32 rows).
//                               With a channel list the stores stay contiguous and the loads gather.
//                               kResmapRowsInFlight rows are loaded before the first is mapped: the two divisions of a
//                               sample are long chains, the loads behind them would wait.
// The lanes' form is chosen per call (resmap_plan_of): 16-byte loads need the identity list, an even n_ch and a 16-byte
// aligned rows_dev; 16-byte stores an even n_out and a 16-byte aligned out_dev; anything else takes 8 bytes a sample.
// All index arithmetic is 64-bit.  In place (out == rows, identity): a lane loads the rows of a turn before it stores
// them, and no other lane touches them.  Compiler-scheduled and GSDR_NO_PK: it runs beside another handle's
// matrix-core loop.
#pragma clang fp contract(off)
#include "resmap_kernels.h"

#include <cstdint>

#include "ddc_kernels.h"

namespace gsdr {
namespace {

constexpr int kResmapRowsInFlight = 4;
constexpr unsigned kResmapMaxLanes = 1u << 19;       // 256 compute units x 2048 lanes: what fills the device at once

struct ResmapArgs {
    ResmapFeed f;
    unsigned units, row_step;
    unsigned long long lanes;            // units x row_step
};

template <int KIND, int LANES>
__global__ __launch_bounds__(256) GSDR_NO_PK void resmap_kernel(const ResmapArgs a) {
    constexpr int W = LANES == kResmapSingle ? 1 : 2;
    const unsigned long long g = (unsigned long long)blockIdx.x * 256ULL + (unsigned long long)threadIdx.x;
    if (g >= a.lanes) return;
    const unsigned r0 = (unsigned)(g / a.units);                   // < row_step
    const unsigned k0 = (unsigned)(g - (unsigned long long)r0 * a.units) * (unsigned)W;      // first output column
    gsdr_resmap_col c[W];
    double2 o[W];
    size_t ch[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        c[w] = a.f.cols[k0 + w];
        o[w] = a.f.offs[k0 + w];
        ch[w] = a.f.channels ? (size_t)a.f.channels[k0 + w] : (size_t)(k0 + w);
    }
    const size_t n_ch = (size_t)a.f.n_ch, n_out = (size_t)a.f.n_out;
    const unsigned n_rows = (unsigned)a.f.n_rows;                  // <= 2^20; row_step <= 2^19: no unsigned sum wraps
    for (unsigned r = r0; r < n_rows; r += (unsigned)kResmapRowsInFlight * a.row_step) {
        float2 v[kResmapRowsInFlight][W];
        // (a row past the end is loaded from row r and dropped: no load sits behind a test of its own)
#pragma unroll
        for (int s = 0; s < kResmapRowsInFlight; ++s) {
            const unsigned rs = r + (unsigned)s * a.row_step;
            const float2 *x = a.f.rows + (size_t)(rs < n_rows ? rs : r) * n_ch;
            if (LANES == kResmapPair) {
                const float4 t = *reinterpret_cast<const float4 *>(x + k0);
                v[s][0].x = t.x, v[s][0].y = t.y, v[s][W - 1].x = t.z, v[s][W - 1].y = t.w;
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w) v[s][w] = x[ch[w]];
            }
        }
#pragma unroll
        for (int s = 0; s < kResmapRowsInFlight; ++s) {
            const unsigned rs = r + (unsigned)s * a.row_step;
            if (rs >= n_rows) break;
            float y[W][2];
#pragma unroll
            for (int w = 0; w < W; ++w) gsdr_resmap_sample(KIND, c[w], o[w].x, o[w].y, v[s][w].x, v[s][w].y, y[w][0], y[w][1]);
            float2 *dst = a.f.out + (size_t)rs * n_out + k0;
            if (W == 2) {
                float4 t;
                t.x = y[0][0], t.y = y[0][1], t.z = y[W - 1][0], t.w = y[W - 1][1];
                *reinterpret_cast<float4 *>(dst) = t;
            } else {
                float2 t;
                t.x = y[0][0], t.y = y[0][1];
                *dst = t;
            }
        }
    }
}

template <int KIND>
hipError_t launch_kind(const ResmapArgs &a, int lanes, unsigned blocks, hipStream_t st) {
    switch (lanes) {
        case kResmapPair: hipLaunchKernelGGL((resmap_kernel<KIND, kResmapPair>), dim3(blocks), dim3(256), 0, st, a); break;
        case kResmapPairOut: hipLaunchKernelGGL((resmap_kernel<KIND, kResmapPairOut>), dim3(blocks), dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((resmap_kernel<KIND, kResmapSingle>), dim3(blocks), dim3(256), 0, st, a); break;
    }
    return hipGetLastError();
}

}  // namespace

ResmapPlan resmap_plan_of(const ResmapFeed &f) {
    const bool in16 = (reinterpret_cast<uintptr_t>(f.rows) & 15u) == 0, out16 = (reinterpret_cast<uintptr_t>(f.out) & 15u) == 0;
    const bool pair_out = out16 && f.n_out % 2 == 0;
    const bool pair_in = pair_out && !f.channels && in16;          // identity: n_ch == n_out, even
    ResmapPlan p{};
    p.lanes = pair_in ? kResmapPair : (pair_out ? kResmapPairOut : kResmapSingle);
    p.units = (unsigned)(pair_out ? f.n_out / 2 : f.n_out);
    // a lane takes kResmapRowsInFlight rows where that still fills the device, more where it would overfill it
    const unsigned want = ((unsigned)f.n_rows + (unsigned)kResmapRowsInFlight - 1u) / (unsigned)kResmapRowsInFlight;
    const unsigned cap = kResmapMaxLanes / p.units > 1u ? kResmapMaxLanes / p.units : 1u;
    p.row_step = want < cap ? want : cap;
    p.blocks = (unsigned)(((unsigned long long)p.units * p.row_step + 255ULL) / 256ULL);
    return p;
}

hipError_t launch_resmap_feed(const ResmapFeed &f, hipStream_t st) {
    if (f.n_rows < 1 || f.n_rows > (1 << 20) || f.n_ch < 1 || f.n_ch > (1 << 20) || f.n_out < 1 || f.n_out > (1 << 20) || !f.rows || !f.out ||
        !f.cols || !f.offs || (!f.channels && f.n_out != f.n_ch) || f.kind < GSDR_RESMAP_CAL || f.kind > GSDR_RESMAP_X_QR)
        return hipErrorInvalidValue;
    const ResmapPlan p = resmap_plan_of(f);
    ResmapArgs a{};
    a.f = f, a.units = p.units, a.row_step = p.row_step;
    a.lanes = (unsigned long long)p.units * p.row_step;
    switch (f.kind) {
        case GSDR_RESMAP_CAL: return launch_kind<GSDR_RESMAP_CAL>(a, p.lanes, p.blocks, st);
        case GSDR_RESMAP_X_DQR: return launch_kind<GSDR_RESMAP_X_DQR>(a, p.lanes, p.blocks, st);
        default: return launch_kind<GSDR_RESMAP_X_QR>(a, p.lanes, p.blocks, st);
    }
}

}  // namespace gsdr
