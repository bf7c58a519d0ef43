// stats_kernels.hip -- the row statistics on demodulated rows (the contract: include/gsdr.h, "row statistics on the
// device"; the laws: stats_state.h; the design: DESIGN.md section 4.14).
//   stats_feed_kernel   one launch per feed, one pass over the rows for the chains AND the histogram.  A workgroup owns
//                       a TILE of channels and 256 / tile chains; a thread owns one (chain, channel), the channel
//                       running fastest across the lanes, so that the lanes of a wave read runs of one row.  The
//                       thread keeps its channel's axis in registers, loads its chain once, walks the feed rows
//                       j', j' + lanes, ... of its chain (kStatsDepth of them in flight) and stores the chain once: no
//                       atomics on the sums, and a chain of additions does not see where the stream was cut.  The
//                       bins are counted in an LDS table [tile][n_bins + 3] of 32-bit counters (a feed has at most
//                       2^20 rows) with ds atomics -- the lanes of a wave that share a channel are its 64 / tile
//                       chains, so two of them meet only in the same bin -- and the table is flushed at the end as
//                       wave-contiguous 64-bit global adds: the tile's counters are one contiguous run of counts[],
//                       a wave takes 64 of them per instruction and skips a stretch that is all zero (the tails of
//                       the range).  Integer adds commute: the counts do not depend on the split.  One lane per
//                       channel's histogram in global memory would be the 64-rows shape the microarchitecture guide
//                       measures 17 times below the shaped rate.
//   stats_read_kernel   one workgroup per channel: the bins' prefix sums (a chunk per thread, a scan over the 256
//                       chunk sums in LDS), the halving tree of the chains (the levels above 256 in registers, by a
//                       thread over its chains j, j + 256, ... in bit-reversed order with a stack of one partial per
//                       level -- the same pairs in the same order as the tree -- the rest in LDS), the summary and
//                       the quantiles.
// All index arithmetic that can pass 2^31 is 64-bit.  Compiler-scheduled and GSDR_NO_PK: they run beside another
// handle's matrix-core loop.
//
// Contraction is off for the whole file: hipcc contracts by default and the host twin must see the same roundings.
#pragma clang fp contract(off)
#include "stats_kernels.h"

#include "ddc_kernels.h"

namespace gsdr {
namespace {

constexpr int kStatsDepth = 8;           // rows a thread of stats_feed_kernel has in flight

struct StatsFeedArgs {
    StatsFeed f;
    int tile, tile_log2;
    unsigned phase;                      // row0 mod lanes
};

// (the HIP headers' __syncthreads, __ballot, atomicAdd, __brev, ... are not always_inline: inside a kernel with other
//  target features -- GSDR_NO_PK -- they would stay real calls; the builtins they wrap are used directly)
__device__ __forceinline__ void wg_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ unsigned f2u(float f) { return __builtin_bit_cast(unsigned, f); }
__device__ __forceinline__ float u2f(unsigned u) { return __builtin_bit_cast(float, u); }

__device__ __forceinline__ gsdr_stats_chain chain_load(const StatsChains &t, size_t at) {
    gsdr_stats_chain s;
    s.S = t.S[at], s.Q = t.Q[at];
    s.mn = u2f(t.mn[at] ^ kStatsMinEmpty), s.mx = u2f(t.mx[at] ^ kStatsMaxEmpty);
    return s;
}

__device__ __forceinline__ void chain_store(const StatsChains &t, size_t at, const gsdr_stats_chain &s) {
    t.S[at] = s.S, t.Q[at] = s.Q;
    t.mn[at] = f2u(s.mn) ^ kStatsMinEmpty, t.mx[at] = f2u(s.mx) ^ kStatsMaxEmpty;
}

__device__ __forceinline__ void stats_take(const gsdr_stats_axis &ax, int n_bins, unsigned *bins, gsdr_stats_chain &s, float2 v) {
    float q;
    const int slot = gsdr_stats_sample(ax, n_bins, v.x, v.y, q);
    (void)__hip_atomic_fetch_add(bins + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (slot != n_bins + 2) gsdr_stats_chain_add(s, ax.p, q);
}

__global__ __launch_bounds__(256) GSDR_NO_PK void stats_feed_kernel(const StatsFeedArgs a) {
    extern __shared__ unsigned table[];                            // [tile][n_bins + 3]
    const int nb3 = a.f.n_bins + 3;
    const int cl = (int)threadIdx.x & (a.tile - 1), jl = (int)threadIdx.x >> a.tile_log2;
    const int c0 = (int)blockIdx.x * a.tile, c = c0 + cl;
    const int j = (int)blockIdx.y * (256 >> a.tile_log2) + jl;
    const int cells = a.tile * nb3;                                // <= 16384
    for (int i = (int)threadIdx.x; i < cells; i += 256) table[i] = 0u;
    wg_sync();
    if (c < a.f.n_ch && j < a.f.lanes) {
        // the first feed row of chain j: the row r of the stream with r mod lanes == j
        const int first = (int)(((unsigned)j - a.phase) & (unsigned)(a.f.lanes - 1));
        const int n = a.f.n_rows, step = a.f.lanes;                // n <= 2^20, step <= 2^15: no int sum below wraps
        if (first < n) {
            const gsdr_stats_axis ax = a.f.axes[c];
            const size_t at = (size_t)j * (size_t)a.f.n_ch + (size_t)c;
            gsdr_stats_chain s = chain_load(a.f.chains, at);
            unsigned *bins = table + cl * nb3;
            const float2 *x = a.f.rows + c;
            const size_t n_ch = (size_t)a.f.n_ch;
            int i = first;
            for (; i + (kStatsDepth - 1) * step < n; i += kStatsDepth * step) {
                float2 v[kStatsDepth];
#pragma unroll
                for (int u = 0; u < kStatsDepth; ++u) v[u] = x[(size_t)(i + u * step) * n_ch];
#pragma unroll
                for (int u = 0; u < kStatsDepth; ++u) stats_take(ax, a.f.n_bins, bins, s, v[u]);
            }
            for (; i < n; i += step) stats_take(ax, a.f.n_bins, bins, s, x[(size_t)i * n_ch]);
            chain_store(a.f.chains, at, s);
        }
    }
    wg_sync();
    // the flush: the counters of the tile's channels that exist are counts[c0 (n_bins + 3), ...), in the table's order
    const int valid = a.f.n_ch - c0 < a.tile ? a.f.n_ch - c0 : a.tile;
    const int total = valid * nb3;
    unsigned long long *dst = a.f.counts + (size_t)c0 * (size_t)nb3;
    for (int base = (int)threadIdx.x & ~63; base < total; base += 256) {      // uniform in a wave
        const int i = base + ((int)threadIdx.x & 63);
        const unsigned v = i < total ? table[i] : 0u;
        if (__builtin_amdgcn_ballot_w64(v != 0u) == 0ULL) continue;
        if (v != 0u) (void)__hip_atomic_fetch_add(dst + i, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) GSDR_NO_PK void stats_read_kernel(const StatsRead a) {
    __shared__ unsigned long long scan[256];
    __shared__ gsdr_stats_chain part[256];
    const int c = (int)blockIdx.x, t = (int)threadIdx.x;
    const int n_bins = a.n_bins;
    const unsigned long long *cnt = a.counts + (size_t)c * (size_t)(n_bins + 3);
    // the bins: thread t sums bins [b0, b1), the scan gives what lies below them
    const int per = (n_bins + 255) / 256;
    const int b0 = t * per < n_bins ? t * per : n_bins, b1 = b0 + per < n_bins ? b0 + per : n_bins;
    unsigned long long mine = 0;
    for (int b = b0; b < b1; ++b) mine += cnt[1 + b];
    scan[t] = mine;
    wg_sync();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned long long v = t >= off ? scan[t - off] : 0ULL;
        wg_sync();
        scan[t] += v;
        wg_sync();
    }
    const unsigned long long bins = scan[255], below = scan[t] - mine;
    const unsigned long long under = cnt[0], over = cnt[n_bins + 1], bad = cnt[n_bins + 2];
    // the chains: P partials by the tree's levels h >= P, then the levels below in LDS
    const int P = a.lanes < 256 ? a.lanes : 256, M = a.lanes / P;                 // powers of two, M <= 128
    int logM = 0;
    while ((1 << logM) < M) ++logM;
    if (t < P) {
        // st[b]: the partial of 2^b chains that waits for its right-hand neighbour (bit b of i says whether it is there).
        // Every index is a constant after unrolling and nothing leaves the loops early: the stack stays in registers.
        gsdr_stats_chain st[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) st[b] = gsdr_stats_chain{0.0, 0.0, 0.f, 0.f};
        for (int i = 0; i < M; ++i) {
            const int m = logM ? (int)(__builtin_bitreverse32((unsigned)i) >> (32 - logM)) : 0;
            gsdr_stats_chain v = chain_load(a.chains, (size_t)(t + P * m) * (size_t)a.n_ch + (size_t)c);
            bool carried = true;                                   // v still looks for its place
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool there = ((i >> b) & 1) != 0;
                const gsdr_stats_chain joined = gsdr_stats_chain_join(st[b], v);
                if (carried && there) v = joined;
                if (carried && !there) st[b] = v;
                carried = carried && there;
            }
        }
        gsdr_stats_chain r = st[0];
#pragma unroll
        for (int b = 1; b < 8; ++b)
            if (b == logM) r = st[b];
        part[t] = r;
    }
    wg_sync();
    for (int h = P / 2; h >= 1; h >>= 1) {
        if (t < h) part[t] = gsdr_stats_chain_join(part[t], part[t + h]);
        wg_sync();
    }
    const gsdr_stats_axis ax = a.axes[c];
    if (t == 0 && a.summary) a.summary[c] = gsdr_stats_summarise(part[0], ax.p, under, bins, over, bad);
    if (!a.quant) return;
    const unsigned long long n = under + bins + over;
    for (int ip = 0; ip < a.n_p; ++ip) {
        double *o = a.quant + (size_t)c * (size_t)a.n_p + (size_t)ip;
        if (n == 0) {
            if (t == 0) *o = __builtin_nan("");
            continue;
        }
        double pr = a.pr[0];                                       // (a variable index into the arguments would copy them to scratch)
#pragma unroll
        for (int k = 1; k < GSDR_STATS_MAX_QUANTILES; ++k)
            if (k == ip) pr = a.pr[k];
        const unsigned long long rank = gsdr_stats_rank(pr, n);
        if (under >= rank) {
            if (t == 0) *o = -__builtin_inf();
            continue;
        }
        if (rank > under + bins) {
            if (t == 0) *o = __builtin_inf();
            continue;
        }
        unsigned long long C = under + below;
        if (!(C < rank && rank <= C + mine)) continue;             // exactly one thread holds the rank
        for (int b = b0; b < b1; ++b) {
            const unsigned long long h = cnt[1 + b];
            if (rank <= C + h) {
                *o = gsdr_stats_in_bin(ax, b, rank, C, h);
                break;
            }
            C += h;
        }
    }
}

}  // namespace

hipError_t launch_stats_feed(const StatsFeed &f, hipStream_t st) {
    if (!stats_shape_ok(f.n_ch, f.n_bins, f.lanes) || f.n_rows < 1 || f.n_rows > (1 << 20) || f.row0 < 0 || !f.rows || !f.axes || !f.counts ||
        !f.chains.S || !f.chains.Q || !f.chains.mn || !f.chains.mx)
        return hipErrorInvalidValue;
    const StatsPlan p = stats_plan_of(f.n_ch, f.n_bins, f.lanes);
    if (p.lds_bytes > kStatsMaxLds || p.tiles < 1 || p.splits < 1 || p.splits > kStatsMaxSplits) return hipErrorInvalidValue;
    StatsFeedArgs a{};
    a.f = f, a.tile = p.tile;
    while ((1 << a.tile_log2) < p.tile) ++a.tile_log2;
    a.phase = (unsigned)(f.row0 % f.lanes);
    hipLaunchKernelGGL(stats_feed_kernel, dim3((unsigned)p.tiles, (unsigned)p.splits), dim3(256), p.lds_bytes, st, a);
    return hipGetLastError();
}

hipError_t launch_stats_read(const StatsRead &r, hipStream_t st) {
    if (!stats_shape_ok(r.n_ch, r.n_bins, r.lanes) || !r.axes || !r.counts || !r.chains.S || !r.chains.Q || !r.chains.mn || !r.chains.mx ||
        (!r.summary && !r.quant) || r.n_p < 0 || r.n_p > GSDR_STATS_MAX_QUANTILES || (r.quant && r.n_p < 1))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(stats_read_kernel, dim3((unsigned)r.n_ch), dim3(256), 0, st, r);
    return hipGetLastError();
}

}  // namespace gsdr
