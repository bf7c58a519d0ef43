// cov_kernels.hip -- the channel covariance on demodulated rows (the contract: include/gsdr.h, "channel covariance on
// the device"; the laws: cov_state.h; the design: DESIGN.md section 4.15).
//   cov_project_kernel      rows -> D[row][n_var] doubles: a thread per (row, variable), the variable running fastest, so
//                           the stores are coalesced; the channel gather and the five float32 operations happen once per
//                           sample here and not once per tile pair in the loop below.  A double is as many bytes as the
//                           float2 it came from: the accumulate pass loses nothing by reading D.
//   cov_accumulate_kernel   a workgroup of 16 x 16 threads owns one pair (I >= J) of tiles of T = 16 R variables and one
//                           chain.  Thread (ty, tx) keeps R x R cells of the pair's square of G in registers (own():
//                           pairs of neighbouring variables, 32 apart), loads them once and stores them once.  It walks the chain's feed rows
//                           first, first + lanes, ... in order, kCovStageRows of them at a time through one of two LDS
//                           buffers (the next stage's loads are in flight while this one is computed; one barrier per
//                           stage).  Per row a thread reads R doubles of d of each tile, two at a time, and does R^2 FMAs: at
//                           R = 8, 64 FMAs (256 cycles of a SIMD's FP64 pipe) for 8 ds_read_b128 (32 cycles of the LDS,
//                           which the four SIMDs of a compute unit share).  The threads ty == 0 of a diagonal pair add the chain's S as well.  A diagonal
//                           pair computes its full square; only its lower half is read.  A chain without a row in the
//                           feed returns before it loads anything.
//   cov_read_kernel         a thread per cell (i, j <= i): the halving trees of the up to five sums the kind's law
//                           needs (each by one thread over its chains in bit-reversed order with a stack of one partial
//                           per level -- the same pairs in the same order as the tree), the law, the mirrored store.
// All index arithmetic that can pass 2^31 is 64-bit.  Compiler-scheduled and GSDR_NO_PK: they run beside another
// handle's matrix-core loop.  Register arrays are indexed by constants after unrolling; the LDS is indexed, no pointer
// into it is advanced.
//
// Contraction is off for the whole file: hipcc contracts by default and the host twin must see the same roundings.  The
// one fused operation per cell is written as such (gsdr_cov_cell).
#pragma clang fp contract(off)
#include "cov_kernels.h"

#include "ddc_kernels.h"

namespace gsdr {
namespace {

struct CovFeedArgs {
    CovFeed f;
    unsigned phase;                      // row0 mod lanes
    int pairs, project_x, project_x_log2;
};

struct CovReadArgs {
    CovRead r;
    int tile, tile_log2, pairs, lanes_log2;
};

// (the HIP headers' __syncthreads is not always_inline: inside a kernel with other target features -- GSDR_NO_PK -- it
//  would stay a real call; the builtins it wraps are used directly)
__device__ __forceinline__ void wg_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the tiles (I >= J) of pair p = I (I + 1) / 2 + J; at most 4096 / tile of them (32 with the library's 128)
__device__ __forceinline__ void tiles_of_pair(int p, int &I, int &J) {
    I = 0;
    while ((I + 1) * (I + 2) / 2 <= p) ++I;
    J = p - I * (I + 1) / 2;
}

__global__ __launch_bounds__(256) GSDR_NO_PK void cov_project_kernel(const CovFeedArgs a) {
    const int t = (int)threadIdx.x;
    const int v = (int)blockIdx.y * a.project_x + (t & (a.project_x - 1));
    const int row = (int)blockIdx.x * (256 >> a.project_x_log2) + (t >> a.project_x_log2);      // < 2^20 + 256
    if (v >= a.f.n_var || row >= a.f.n_rows) return;
    const gsdr_cov_axis ax = a.f.axes[v];
    const float2 x = a.f.rows[(size_t)row * (size_t)a.f.n_ch + (size_t)ax.channel];
    a.f.D[(size_t)row * (size_t)a.f.n_var + (size_t)v] = gsdr_cov_sample(ax, x.x, x.y);
}

// what thread t stages of stage s: element t + 256 u of [kCovStageRows][I tile | J tile][T]; 0 behind the chain's last row
// and behind the last variable (such a d only meets cells that are never read)
template <int R>
__device__ __forceinline__ void stage_load(const CovFeedArgs &a, int s, int first, int count, int I, int J, double (&pre)[R]) {
    constexpr int T = 16 * R;
    const size_t n_var = (size_t)a.f.n_var;
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int e = (int)threadIdx.x + 256 * u;
        const int k = e / (2 * T), w = e % (2 * T);
        const int var = (w < T ? I : J) * T + (w & (T - 1));
        const int step = s * kCovStageRows + k;                               // the row's number within the chain
        const size_t row = (size_t)first + (size_t)step * (size_t)a.f.lanes;
        pre[u] = step < count && var < a.f.n_var ? a.f.D[row * n_var + (size_t)var] : 0.0;
    }
}

// the variable, within its tile, of slot u < R of the thread with coordinate c < 16: pairs of neighbours from R = 2 on, so
// that a thread reads its d as 16-byte LDS reads (ds_read_b128: twice the bytes per LDS cycle of the ds_read2_b64 the
// compiler makes of single doubles) -- the 16 c of a lane group then read 16 consecutive 16-byte slots: no bank conflict
template <int R>
__device__ __forceinline__ constexpr int own(int u, int c) {
    constexpr int W = R >= 2 ? 2 : 1;
    return (u / W) * 16 * W + W * c + u % W;
}

// the R doubles of d of tile `half` (0: I, 1: J) of row k of buffer buf that the thread with coordinate c owns
template <int R, int T>
__device__ __forceinline__ void stage_read(const double (&stage)[2][kCovStageRows][2][T], int buf, int k, int half, int c, double (&d)[R]) {
    if constexpr (R >= 2) {
#pragma unroll
        for (int u = 0; u < R; u += 2) {
            const double2 v = *reinterpret_cast<const double2 *>(&stage[buf][k][half][own<R>(u, c)]);
            d[u] = v.x, d[u + 1] = v.y;
        }
    } else {
        d[0] = stage[buf][k][half][c];
    }
}

template <int R>
__global__ __launch_bounds__(256, 2) GSDR_NO_PK void cov_accumulate_kernel(const CovFeedArgs a) {
    constexpr int T = 16 * R, K = kCovStageRows;
    __shared__ __attribute__((aligned(16))) double stage[2][K][2][T];      // [buffer][row][I tile | J tile][variable]
    double *const flat = &stage[0][0][0][0];
    const int t = (int)threadIdx.x, tx = t & 15, ty = t >> 4;
    const int chain = (int)blockIdx.y;
    // the first feed row of the chain: the row r of the stream with r mod lanes == chain
    const int first = (int)(((unsigned)chain - a.phase) & (unsigned)(a.f.lanes - 1));
    if (first >= a.f.n_rows) return;                               // the whole workgroup
    const int count = (a.f.n_rows - first + a.f.lanes - 1) / a.f.lanes;      // >= 1; n_rows <= 2^20, lanes <= 2^12
    int I, J;
    tiles_of_pair((int)blockIdx.x, I, J);
    double *const G = a.f.G + ((size_t)chain * (size_t)a.pairs + (size_t)blockIdx.x) * (size_t)(T * T);
    double acc[R][R];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < R; ++j) acc[i][j] = G[own<R>(i, ty) * T + own<R>(j, tx)];
    // the sums: the threads ty == 0 of a diagonal pair, on the d of the J tile they read anyway
    const bool sums = I == J && ty == 0;
    double *const S = a.f.S + (size_t)chain * (size_t)a.f.n_var;
    double sum[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int v = J * T + own<R>(j, tx);
        sum[j] = sums && v < a.f.n_var ? S[v] : 0.0;
    }
    const int stages = (count + K - 1) / K;
    double pre[R];
    stage_load<R>(a, 0, first, count, I, J, pre);
#pragma unroll
    for (int u = 0; u < R; ++u) flat[t + 256 * u] = pre[u];
    wg_sync();
    for (int s = 0; s < stages; ++s) {
        const int buf = s & 1;
        const bool more = s + 1 < stages;
        if (more) stage_load<R>(a, s + 1, first, count, I, J, pre);
        const int rem = count - s * K < K ? count - s * K : K;     // rows of this stage that exist: >= 1
        // (not unrolled: the compiler would hoist every row's LDS reads and run out of registers at R = 8)
#pragma unroll 1
        for (int k = 0; k < rem; ++k) {
            double di[R], dj[R];
            stage_read<R, T>(stage, buf, k, 0, ty, di);
            stage_read<R, T>(stage, buf, k, 1, tx, dj);
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int j = 0; j < R; ++j) acc[i][j] = gsdr_cov_cell(di[i], dj[j], acc[i][j]);
            if (sums) {
#pragma unroll
                for (int j = 0; j < R; ++j) sum[j] = sum[j] + dj[j];
            }
        }
        // the other buffer was read one stage ago, and every thread has passed a barrier since
        if (more) {
#pragma unroll
            for (int u = 0; u < R; ++u) flat[(buf ^ 1) * (K * 2 * T) + t + 256 * u] = pre[u];
        }
        wg_sync();
    }
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < R; ++j) G[own<R>(i, ty) * T + own<R>(j, tx)] = acc[i][j];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int v = J * T + own<R>(j, tx);
        if (sums && v < a.f.n_var) S[v] = sum[j];
    }
}

constexpr int kCovTreeLevels = 13;       // GSDR_COV_MAX_LANES = 2^12 chains: partials of 1, 2, ..., 2^12 chains
static_assert((1 << (kCovTreeLevels - 1)) == GSDR_COV_MAX_LANES, "one level of the stack per power of two up to the most lanes");

// X[0] of the halving tree over x[k stride], k < lanes.  st[b]: the partial of 2^b chains that waits for its right-hand
// neighbour (bit b of i says whether it is there).  Every index is a constant after unrolling and nothing leaves the
// loops early: the stack stays in registers.  The leaves are loaded kCovTreeDepth at a time, so that their loads are in
// flight together, and pushed in their order: the additions are those of the tree, one after the other.
constexpr int kCovTreeDepth = 8;
__device__ __forceinline__ double cov_tree(const double *x, size_t stride, int lanes, int lanes_log2) {
    double st[kCovTreeLevels];
#pragma unroll
    for (int b = 0; b < kCovTreeLevels; ++b) st[b] = 0.0;
    for (int i0 = 0; i0 < lanes; i0 += kCovTreeDepth) {
        double leaf[kCovTreeDepth];
#pragma unroll
        for (int u = 0; u < kCovTreeDepth; ++u) {
            const int i = i0 + u;                                  // behind the last leaf (lanes < 8): chain 0 again, not pushed
            const int m = lanes_log2 && i < lanes ? (int)(__builtin_bitreverse32((unsigned)i) >> (32 - lanes_log2)) : 0;
            leaf[u] = x[(size_t)m * stride];
        }
#pragma unroll
        for (int u = 0; u < kCovTreeDepth; ++u) {
            const int i = i0 + u;
            double v = leaf[u];
            bool carried = i < lanes;                              // v still looks for its place
#pragma unroll
            for (int b = 0; b < kCovTreeLevels; ++b) {
                const bool there = ((i >> b) & 1) != 0;
                const double joined = st[b] + v;
                if (carried && there) v = joined;
                if (carried && !there) st[b] = v;
                carried = carried && there;
            }
        }
    }
    double r = st[0];
#pragma unroll
    for (int b = 1; b < kCovTreeLevels; ++b)
        if (b == lanes_log2) r = st[b];
    return r;
}

__global__ __launch_bounds__(256) GSDR_NO_PK void cov_read_kernel(const CovReadArgs a) {
    int I, J;
    tiles_of_pair((int)blockIdx.x, I, J);
    const int e = (int)blockIdx.y * 256 + (int)threadIdx.x;       // < tile^2
    const int il = e >> a.tile_log2, jl = e & (a.tile - 1);
    const int i = I * a.tile + il, j = J * a.tile + jl;
    if (i >= a.r.n_var || j > i) return;
    const int kind = a.r.kind;
    const size_t square = (size_t)1 << (2 * a.tile_log2), per_chain = (size_t)a.pairs * square, n_var = (size_t)a.r.n_var;
    const double Gij = cov_tree(a.r.G + (size_t)blockIdx.x * square + (size_t)e, per_chain, a.r.lanes, a.lanes_log2);
    const bool wants_mean = a.r.mean && j == 0;
    double Si = 0.0, Sj = 0.0, Gii = 0.0, Gjj = 0.0;
    if (kind != GSDR_COV_SUMS || wants_mean) Si = cov_tree(a.r.S + i, n_var, a.r.lanes, a.lanes_log2);
    if (kind != GSDR_COV_SUMS) Sj = cov_tree(a.r.S + j, n_var, a.r.lanes, a.lanes_log2);
    if (kind == GSDR_COV_CORR) {
        const size_t pi = (size_t)(I * (I + 1) / 2 + I), pj = (size_t)(J * (J + 1) / 2 + J);
        Gii = cov_tree(a.r.G + pi * square + (size_t)(il * a.tile + il), per_chain, a.r.lanes, a.lanes_log2);
        Gjj = cov_tree(a.r.G + pj * square + (size_t)(jl * a.tile + jl), per_chain, a.r.lanes, a.lanes_log2);
    }
    const double v = gsdr_cov_read_cell(kind, Si, Sj, Gij, Gii, Gjj, a.r.n, i == j);
    a.r.out[(size_t)i * n_var + (size_t)j] = v;
    a.r.out[(size_t)j * n_var + (size_t)i] = v;
    if (wants_mean) a.r.mean[i] = kind == GSDR_COV_SUMS ? Si : gsdr_cov_mean(Si, a.r.axes[i].pivot, a.r.n);
}

int log2_of(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

}  // namespace

hipError_t launch_cov_feed(const CovFeed &f, hipStream_t st) {
    if (!cov_shape_ok(f.n_ch, f.n_var, f.lanes) || f.n_rows < 1 || f.n_rows > (1 << 20) || f.row0 < 0 || !f.rows || !f.axes || !f.D || !f.S || !f.G)
        return hipErrorInvalidValue;
    const CovPlan p = cov_plan_of(f.n_var, f.lanes);
    CovFeedArgs a{};
    a.f = f, a.phase = (unsigned)(f.row0 % f.lanes), a.pairs = p.pairs, a.project_x = p.project_x, a.project_x_log2 = log2_of(p.project_x);
    const int rows_per_group = 256 / p.project_x;
    hipLaunchKernelGGL(cov_project_kernel, dim3((unsigned)((f.n_rows + rows_per_group - 1) / rows_per_group), (unsigned)((f.n_var + p.project_x - 1) / p.project_x)),
                       dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)p.pairs, (unsigned)p.lanes);
    switch (p.tile) {
    case 16: hipLaunchKernelGGL(cov_accumulate_kernel<1>, grid, dim3(256), 0, st, a); break;
    case 32: hipLaunchKernelGGL(cov_accumulate_kernel<2>, grid, dim3(256), 0, st, a); break;
    case 64: hipLaunchKernelGGL(cov_accumulate_kernel<4>, grid, dim3(256), 0, st, a); break;
    case 128: hipLaunchKernelGGL(cov_accumulate_kernel<8>, grid, dim3(256), 0, st, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_cov_read(const CovRead &r, hipStream_t st) {
    if (r.n_var < 1 || r.n_var > GSDR_COV_MAX_VARS || !cov_shape_ok(1, r.n_var, r.lanes) || !r.axes || !r.S || !r.G || !r.out || r.n < 0 ||
        (r.kind != GSDR_COV_SUMS && r.kind != GSDR_COV_COV && r.kind != GSDR_COV_CORR))
        return hipErrorInvalidValue;
    const CovPlan p = cov_plan_of(r.n_var, r.lanes);
    CovReadArgs a{};
    a.r = r, a.tile = p.tile, a.tile_log2 = log2_of(p.tile), a.pairs = p.pairs, a.lanes_log2 = log2_of(r.lanes);
    hipLaunchKernelGGL(cov_read_kernel, dim3((unsigned)p.pairs, (unsigned)(p.tile * p.tile / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace gsdr
