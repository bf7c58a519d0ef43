// cov_host.cpp -- the channel covariance's creation, refusals and host twin (the contract: include/gsdr.h, "channel
// covariance on the device"; the laws: cov_state.h).  The twin calls the functions cov_project_kernel, cov_accumulate_kernel
// and cov_read_kernel (cov_kernels.hip) call, walks every chain in stream order and joins the chains by the halving tree
// as it is written in the header: the bits are the same.  No HIP here.
#include <algorithm>
#include <cmath>
#include <vector>

#include "cov_state.h"
#include "stage_host.h"

extern "C" {
int gsdr_cov_dev_create_(gsdr_cov *c) __attribute__((weak));
int gsdr_cov_dev_reset_(gsdr_cov *c, const gsdr_cov_axis *axes) __attribute__((weak));
}

namespace {

// "" or what is wrong with the axes
std::string cov_axes_fault(const gsdr_cov_axis *axes, int n_var, int n_ch) {
    for (int i = 0; i < n_var; ++i) {
        const gsdr_cov_axis &a = axes[i];
        const std::string at = " (variable " + std::to_string(i) + ")";
        if (a.channel < 0 || a.channel >= n_ch) return "axes: channel must be in [0, n_ch)" + at;
        if (a.reserved != 0) return "axes: reserved must be 0" + at;
        if (!std::isfinite(a.bx) || !std::isfinite(a.by) || !std::isfinite(a.dx) || !std::isfinite(a.dy) || !std::isfinite(a.pivot))
            return "axes: every field must be finite" + at;
    }
    return std::string();
}

// X[0] of the halving tree over x[k * stride], k < lanes; `tree` is lanes doubles of room
double cov_join(const double *x, size_t stride, int lanes, std::vector<double> &tree) {
    for (int k = 0; k < lanes; ++k) tree[(size_t)k] = x[(size_t)k * stride];
    for (int h = lanes / 2; h >= 1; h /= 2)
        for (int k = 0; k < h; ++k) tree[(size_t)k] = tree[(size_t)k] + tree[(size_t)(k + h)];
    return tree[0];
}

bool cov_kind_ok(int kind) { return kind == GSDR_COV_SUMS || kind == GSDR_COV_COV || kind == GSDR_COV_CORR; }

}  // namespace

extern "C" {

gsdr_cov *gsdr_cov_create(int n_ch, int n_var, int max_rows, int lanes, const gsdr_cov_axis *axes, int device_index) {
    std::string bad;
    int n_lanes = lanes;
    if (n_ch < 1 || n_ch > (1 << 20)) bad = "n_ch must be in [1, 1048576]";
    else if (n_var < 1 || n_var > GSDR_COV_MAX_VARS) bad = "n_var must be in [1, 4096]";
    else if (max_rows < 1 || max_rows > (1 << 20)) bad = "max_rows must be in [1, 1048576]";
    else if (lanes < 0 || lanes > GSDR_COV_MAX_LANES || (lanes & (lanes - 1)) != 0) bad = "lanes must be 0 or a power of two in [1, 4096]";
    else {
        if (!lanes) n_lanes = gsdr_cov_lanes_rule(n_var, max_rows);
        if ((long long)n_lanes * gsdr::cov_cells(n_var) > kCovMaxCells) bad = "lanes and n_var: lanes x n_var (n_var + 1) / 2 must be at most 268435456 cells";
        else if (!axes) bad = "axes must not be NULL";
        else bad = stage_device_fault(device_index, "GSDR_COV_HOST", gsdr_cov_dev_create_ != nullptr);
    }
    if (bad.empty()) bad = cov_axes_fault(axes, n_var, n_ch);
    const size_t cells = bad.empty() ? (size_t)gsdr::cov_cells(n_var) : 0;
    return stage_create<gsdr_cov>(
        "gsdr_cov_create", bad, device_index,
        "lanes and n_var: no host memory for the chains (" + std::to_string(((size_t)n_lanes * (cells + (size_t)n_var) * 8) >> 20) + " MiB)",
        [&](gsdr_cov &c) {
            c.n_ch = n_ch, c.n_var = n_var, c.max_rows = max_rows, c.lanes = n_lanes;
            c.axes.assign(axes, axes + n_var);
            if (device_index != GSDR_COV_HOST) return;
            c.S.assign((size_t)n_lanes * (size_t)n_var, 0.0);
            c.G.assign((size_t)n_lanes * cells, 0.0);
            c.d.assign((size_t)n_var, 0.0);
        },
        gsdr_cov_dev_create_);
}

void gsdr_cov_close(gsdr_cov *c) { stage_close(c); }

long long gsdr_cov_rows(const gsdr_cov *c) { return c ? c->total : 0; }

int gsdr_cov_lanes(const gsdr_cov *c) { return c ? c->lanes : 0; }

int gsdr_cov_n_var(const gsdr_cov *c) { return c ? c->n_var : 0; }

// The launches of a feed (cov_state.h: the function launch_cov_feed itself asks).
int gsdr_cov_plan(int n_ch, int n_var, int lanes, int out[6]) {
    if (!out || !gsdr::cov_shape_ok(n_ch, n_var, lanes)) return -1;
    const gsdr::CovPlan p = gsdr::cov_plan_of(n_var, lanes);
    out[0] = p.tile, out[1] = p.tiles, out[2] = p.pairs, out[3] = p.lanes, out[4] = (int)p.lds_bytes, out[5] = p.project_x;
    return 0;
}

int gsdr_cov_reset(gsdr_cov *c, const gsdr_cov_axis *axes) {
    const char *const me = "gsdr_cov_reset";
    if (!c) return stage_refuse(me, "null object");
    if (axes) {
        const std::string bad = cov_axes_fault(axes, c->n_var, c->n_ch);
        if (!bad.empty()) return stage_refuse(me, bad);
    }
    if (c->dev) {
        // the device takes the caller's array: the object's own axes change only once that has succeeded
        if (!gsdr_cov_dev_reset_ || gsdr_cov_dev_reset_(c, axes) != 0) return -1;      // has noted why
    } else {
        std::fill(c->S.begin(), c->S.end(), 0.0);
        std::fill(c->G.begin(), c->G.end(), 0.0);
    }
    if (axes) std::copy(axes, axes + c->n_var, c->axes.begin());
    c->total = 0;
    return 0;
}

int gsdr_cov_feed_host(gsdr_cov *c, const gsdr_c64 *rows, int n_rows) {
    const char *const me = "gsdr_cov_feed_host";
    if (const char *why = stage_host_fault(c, "a device object takes gsdr_cov_feed_device")) return stage_refuse(me, why);
    if (n_rows < 0 || n_rows > c->max_rows) return stage_refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows) return stage_refuse(me, "null buffer: rows");
    const size_t n_ch = (size_t)c->n_ch, n_var = (size_t)c->n_var, cells = (size_t)gsdr::cov_cells(c->n_var);
    double *const d = c->d.data();
    for (int r = 0; r < n_rows; ++r) {
        const size_t k = (size_t)((c->total + r) % c->lanes);
        const gsdr_c64 *x = rows + (size_t)r * n_ch;
        double *S = c->S.data() + k * n_var, *G = c->G.data() + k * cells;
        for (size_t i = 0; i < n_var; ++i) {
            const gsdr_cov_axis &a = c->axes[i];
            d[i] = gsdr_cov_sample(a, x[a.channel].x, x[a.channel].y);
        }
        for (size_t i = 0; i < n_var; ++i) {
            S[i] = S[i] + d[i];
            double *g = G + i * (i + 1) / 2;
            for (size_t j = 0; j <= i; ++j) g[j] = gsdr_cov_cell(d[i], d[j], g[j]);
        }
    }
    c->total += n_rows;
    return 0;
}

int gsdr_cov_read_host(gsdr_cov *c, int kind, double *out, double *mean) {
    const char *const me = "gsdr_cov_read_host";
    if (const char *why = stage_host_fault(c, "a device object takes gsdr_cov_read or gsdr_cov_read_device")) return stage_refuse(me, why);
    if (!cov_kind_ok(kind)) return stage_refuse(me, "kind must be GSDR_COV_SUMS, GSDR_COV_COV or GSDR_COV_CORR");
    if (!out) return stage_refuse(me, "null buffer: out");
    const size_t n_var = (size_t)c->n_var, cells = (size_t)gsdr::cov_cells(c->n_var);
    std::vector<double> tree, S, G;
    try {
        tree.resize((size_t)c->lanes), S.resize(n_var), G.resize(cells);
    } catch (const std::bad_alloc &) {
        return stage_refuse(me, "out of memory");
    }
    for (size_t i = 0; i < n_var; ++i) S[i] = cov_join(c->S.data() + i, n_var, c->lanes, tree);
    for (size_t q = 0; q < cells; ++q) G[q] = cov_join(c->G.data() + q, cells, c->lanes, tree);
    for (size_t i = 0; i < n_var; ++i) {
        const double Gii = G[i * (i + 1) / 2 + i];
        for (size_t j = 0; j <= i; ++j) {
            const double v = gsdr_cov_read_cell(kind, S[i], S[j], G[i * (i + 1) / 2 + j], Gii, G[j * (j + 1) / 2 + j], c->total, i == j);
            out[i * n_var + j] = v, out[j * n_var + i] = v;
        }
        if (mean) mean[i] = kind == GSDR_COV_SUMS ? S[i] : gsdr_cov_mean(S[i], c->axes[i].pivot, c->total);
    }
    return 0;
}

}  // extern "C"
