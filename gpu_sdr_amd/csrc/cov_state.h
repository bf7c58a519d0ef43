// cov_state.h -- the channel covariance (include/gsdr.h, "channel covariance on the device") as cov_host.cpp, cov.cpp
// and cov_kernels.hip share it: the object, THE LAWS -- the per-sample law, the cell of a row, the three read laws -- as
// inline host-and-device functions that the kernels and the host twin both include (one text of the arithmetic), the
// lanes rule, and the launch rule of a feed (cov_plan_of), which the launcher and gsdr_cov_plan both ask.
// cov_host.cpp owns creation, the refusals and the host twin; cov.cpp hangs the device part on `dev` through the hooks
// below (its release: stage_state.h).  No HIP here: cov_host.cpp is built without cov.cpp by a host compiler
// (tests/test_cov_sanitizers.py), where the hooks are absent and only host objects exist.
//
// The only fused operations are the two written as __builtin_fma (one IEEE operation on either side: v_fma_f64 on the
// device, fma() or the FMA instruction on the host).  No other product feeds an addition in one expression, and
// contraction is off wherever these functions are compiled.
#ifndef GSDR_COV_STATE_H
#define GSDR_COV_STATE_H

#include <vector>

#include "../../include/gsdr.h"
#include "stage_state.h"

#define GSDR_COV_HD GSDR_STAGE_HD

static_assert(sizeof(gsdr_cov_axis) == 32, "a variable's axis is an int, four floats, an int and a double");

constexpr long long kCovMaxCells = 1LL << 28;      // lanes x n_var (n_var + 1) / 2: 2 GiB of doubles
constexpr int kCovGroupTarget = 512;               // workgroups of 128-wide tiles the lanes rule aims at: two per compute unit

struct gsdr_cov {
    int n_ch = 0, n_var = 0, max_rows = 0, lanes = 0;
    long long total = 0;                      // rows fed since creation / reset
    int device = GSDR_COV_HOST;
    std::vector<gsdr_cov_axis> axes;          // [n_var]
    std::vector<double> S;                    // host twin: [lanes][n_var]
    std::vector<double> G;                    // host twin: [lanes][n_var (n_var + 1) / 2], the cell (i, j <= i) at i (i + 1) / 2 + j
    std::vector<double> d;                    // host twin: one row's d, [n_var]
    gsdr::StageDev *dev = nullptr;            // gsdr::CovDev (cov.cpp)
};

namespace gsdr {

// THE LAUNCH RULE of a feed (cov_kernels.hip launches what it says and decides nothing itself; gsdr_cov_plan gives the
// same answer without a GPU; tests/test_cov_host.py pins it at its edges).
//   The project pass writes D[row][n_var] doubles: a workgroup of 256 threads spans project_x variables by
//   256 / project_x rows; its grid is ceil(n_rows / (256 / project_x)) x ceil(n_var / project_x).
//   The accumulate pass: a workgroup of 16 x 16 threads owns one pair (I >= J) of tiles of `tile` variables and one
//   chain; a thread keeps (tile / 16)^2 cells of G in registers.  Its grid is pairs x lanes; a workgroup stages
//   kCovStageRows rows of both tiles at a time in one of two LDS buffers.
// GSDR_COV_MAX_TILE is for ONE use: the timing A/B of DESIGN.md section 4.15 (profiles/cov_timing_t64.log), a second
// library built with 64 and loaded beside this one.  With 64 the plan, the tile pairs and the layout of G on the device
// are others (no result is), so the figures tests/test_cov_host.py and tests/test_gpu_cov.py pin do not hold for such a
// build: it is for timing, not for the suite.
#ifndef GSDR_COV_MAX_TILE
#define GSDR_COV_MAX_TILE 128
#endif
constexpr int kCovMaxTile = GSDR_COV_MAX_TILE;      // 128: 8 x 8 cells per thread, 64 FMAs for 128 bytes of LDS reads per row
static_assert(kCovMaxTile == 64 || kCovMaxTile == 128, "the accumulate kernel has 4 x 4 and 8 x 8 cells per thread for the large tile");
constexpr int kCovMinTile = 16;          // one cell per thread
constexpr int kCovStageRows = 8;

struct CovPlan {
    int tile, tiles, pairs, lanes;
    unsigned lds_bytes;                  // 2 buffers x kCovStageRows rows x 2 tiles x tile doubles
    int project_x;
};

inline long long cov_cells(int n_var) { return (long long)n_var * (n_var + 1) / 2; }

// the tile of n_var variables: the smallest of 16, 32, 64 that holds them all (8 variables do not run a 128-wide tile
// for 36 cells), kCovMaxTile beyond
inline int cov_tile_of(int n_var) {
    int t = kCovMinTile;
    while (t < kCovMaxTile && t < n_var) t *= 2;
    return t;
}

inline int cov_pairs_of(int n_var) {
    const int t = cov_tile_of(n_var), tiles = (n_var + t - 1) / t;
    return tiles * (tiles + 1) / 2;
}

// what gsdr_cov_create accepts of the three (a lanes of 0 has become the rule's value by then)
inline bool cov_shape_ok(int n_ch, int n_var, int lanes) {
    return n_ch >= 1 && n_ch <= (1 << 20) && n_var >= 1 && n_var <= GSDR_COV_MAX_VARS && lanes >= 1 && lanes <= GSDR_COV_MAX_LANES &&
           (lanes & (lanes - 1)) == 0 && (long long)lanes * cov_cells(n_var) <= kCovMaxCells;
}

inline CovPlan cov_plan_of(int n_var, int lanes) {
    CovPlan p{};
    p.tile = cov_tile_of(n_var);
    p.tiles = (n_var + p.tile - 1) / p.tile;
    p.pairs = p.tiles * (p.tiles + 1) / 2;
    p.lanes = lanes;
    p.lds_bytes = 2u * kCovStageRows * 2u * (unsigned)p.tile * (unsigned)sizeof(double);
    p.project_x = 1;
    while (p.project_x < 256 && p.project_x < n_var) p.project_x *= 2;
    return p;
}

}  // namespace gsdr

// lanes == 0 of gsdr_cov_create: the smallest power of two that gives kCovGroupTarget x 128 / tile workgroups over tile
// pairs x chains -- two workgroups of the 128-wide tile per compute unit, which is what its registers let stay there, and
// as many more of a smaller tile as it is narrower: those are light, and what a chain's walk costs is the latency of its
// stages, so 8 variables x 2^20 rows want the most chains --, but no more chains than a feed of max_rows rows can give
// a row each, at most GSDR_COV_MAX_LANES, and no more than the bound on the cells allows
inline int gsdr_cov_lanes_rule(int n_var, int max_rows) {
    const long long pairs = gsdr::cov_pairs_of(n_var), cells = gsdr::cov_cells(n_var);
    const long long target = (long long)kCovGroupTarget * 128 / gsdr::cov_tile_of(n_var);
    int lanes = 1;
    while (lanes < GSDR_COV_MAX_LANES && pairs * lanes < target && 2 * lanes <= max_rows && 2 * lanes * cells <= kCovMaxCells) lanes *= 2;
    return lanes;
}

// The per-sample law: d of one variable from its channel's sample.
GSDR_COV_HD double gsdr_cov_sample(const gsdr_cov_axis &a, float x, float y) {
    const float v = gsdr_stage_project(a.bx, a.by, a.dx, a.dy, x, y);
    return (double)v - a.pivot;
}

// one row enters one cell
GSDR_COV_HD double gsdr_cov_cell(double di, double dj, double g) { return __builtin_fma(di, dj, g); }

// THE READ LAWS, of joined sums and n rows.  Each takes j <= i: Si, Sj the sums, Gij the cell.
// GSDR_COV_COV: the cell (i, j); `diagonal` says i == j
GSDR_COV_HD double gsdr_cov_cov(double Si, double Sj, double Gij, long long n, bool diagonal) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (n < 2) return __builtin_nan("");
    const double nn = (double)n;
    const double mj = Sj / nn;
    const double num = __builtin_fma(-Si, mj, Gij);
    const double c = num / (nn - 1.0);
    return diagonal && c < 0.0 ? 0.0 : c;                    // a NaN is not < 0: it stays
}

// the mean of variable i (GSDR_COV_COV and GSDR_COV_CORR)
GSDR_COV_HD double gsdr_cov_mean(double Si, double pivot, long long n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (n < 1) return __builtin_nan("");
    const double m = Si / (double)n;
    return pivot + m;
}

// GSDR_COV_CORR: the cell (i, j) from the three cells GSDR_COV_COV gives
GSDR_COV_HD double gsdr_cov_corr(double Cij, double Cii, double Cjj, bool diagonal) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (diagonal) return Cii > 0.0 && Cii <= 1.7976931348623157e308 ? 1.0 : __builtin_nan("");
    const double si = __builtin_sqrt(Cii), sj = __builtin_sqrt(Cjj);
    const double p = si * sj;
    return Cij / p;
}

// one cell of a read of `kind` from the five joined sums it can need
GSDR_COV_HD double gsdr_cov_read_cell(int kind, double Si, double Sj, double Gij, double Gii, double Gjj, long long n, bool diagonal) {
    if (kind == GSDR_COV_SUMS) return Gij;
    const double c = gsdr_cov_cov(Si, Sj, Gij, n, diagonal);
    if (kind == GSDR_COV_COV) return c;
    return gsdr_cov_corr(c, gsdr_cov_cov(Si, Si, Gii, n, true), gsdr_cov_cov(Sj, Sj, Gjj, n, true), diagonal);
}

extern "C" {
// cov.cpp; weak in cov_host.cpp.  _create_: allocates, zeroes and uploads c->axes, 0 or -1 with the message noted; called
// after every bound has been checked.  _reset_: waits for the device, uploads axes[n_var] (checked by the caller) where
// not null, zeroes the chains, waits; c->axes is the caller's to change, behind a 0.
int gsdr_cov_dev_create_(gsdr_cov *c);
int gsdr_cov_dev_reset_(gsdr_cov *c, const gsdr_cov_axis *axes);
}

#endif
