// cov.cpp -- the device part of a cov object (the contract: include/gsdr.h, "channel covariance on the device"): what it
// owns on the GPU, the two launches of a feed, the reads and the way of the axes to the device.  Creation, the refusals of
// the arguments, the lanes rule and the host twin are in cov_host.cpp, the kernels in cov_kernels.hip, the frame of every
// stage in stage_dev.h.
//
// What the HOST has to know of the stream is only the number of rows fed: from it follow the chain of every row of a
// feed and the n of a read.  Nothing is read back by a feed.  The projected rows of a feed (max_rows x n_var doubles) and
// the staging of gsdr_cov_read (n_var^2 + n_var doubles) are allocated at creation: no entry allocates.
#include <string>

#include "cov_kernels.h"
#include "stage_dev.h"

namespace gsdr {

struct CovDev : StageDev {
    DevBuf<gsdr_cov_axis> axes;              // [n_var]
    DevBuf<double> S;                        // [lanes][n_var]
    DevBuf<double> G;                        // [lanes][pairs][tile][tile]: cov_kernels.h
    DevBuf<double> D;                        // [max_rows][n_var]: the projected rows of the feed in flight
    DevBuf<double> out, mean;                // [n_var][n_var], [n_var]: what gsdr_cov_read copies from
};

}  // namespace gsdr

using gsdr::CovDev;
using gsdr::refuse;
using gsdr::result;
using gsdr::set_device;

namespace {

// nullptr or why a device entry cannot take this object
const char *object_fault(const gsdr_cov *c) {
    return gsdr::object_fault(c, "a host object (GSDR_COV_HOST) takes gsdr_cov_feed_host and gsdr_cov_read_host");
}

size_t s_doubles(const gsdr_cov *c) { return (size_t)c->lanes * (size_t)c->n_var; }

size_t g_doubles(const gsdr_cov *c) { return gsdr::cov_g_doubles(gsdr::cov_plan_of(c->n_var, c->lanes)); }

bool kind_ok(int kind) { return kind == GSDR_COV_SUMS || kind == GSDR_COV_COV || kind == GSDR_COV_CORR; }

// the read of `kind` into out (and mean, where not null) on st
hipError_t enqueue_read(const gsdr_cov *c, int kind, double *out, double *mean, hipStream_t st) {
    CovDev *v = static_cast<CovDev *>(c->dev);
    gsdr::CovRead r{};
    r.axes = v->axes, r.S = v->S, r.G = v->G;
    r.n_var = c->n_var, r.lanes = c->lanes, r.kind = kind, r.n = c->total;
    r.out = out, r.mean = mean;
    return gsdr::launch_cov_read(r, st);
}

}  // namespace

extern "C" {

int gsdr_cov_dev_create_(gsdr_cov *c) {
    const size_t n_var = (size_t)c->n_var, s = s_doubles(c), g = g_doubles(c), d = (size_t)c->max_rows * n_var;
    const size_t bytes = (s + g + d + n_var * n_var + n_var) * sizeof(double) + n_var * sizeof(gsdr_cov_axis);
    return gsdr::create_dev<CovDev>(c, "gsdr_cov_create", "(n_var, lanes, max_rows: " + std::to_string(bytes >> 20) + " MiB)", [&](CovDev &v) {
        return v.axes.upload(c->axes) == hipSuccess && v.S.alloc_zeroed(s) == hipSuccess && v.G.alloc_zeroed(g) == hipSuccess &&
               v.D.alloc(d) == hipSuccess && v.out.alloc(n_var * n_var) == hipSuccess && v.mean.alloc(n_var) == hipSuccess;
    });
}

int gsdr_cov_dev_reset_(gsdr_cov *c, const gsdr_cov_axis *axes) {
    const char *const me = "gsdr_cov_reset";
    if (!set_device(c)) return refuse(me, "hipSetDevice failed");
    CovDev *v = static_cast<CovDev *>(c->dev);
    // behind the first wait nothing reads the axes any more: the copy (from pageable memory: it returns when it is done)
    // cannot overtake a feed, and the wait that ends the zeroing covers it too
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess && axes) e = hipMemcpy(v->axes, axes, (size_t)c->n_var * sizeof(gsdr_cov_axis), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = gsdr::zero_behind_all({{v->S, s_doubles(c) * sizeof(double)}, {v->G, g_doubles(c) * sizeof(double)}});
    return result(me, e);
}

int gsdr_cov_feed_device(gsdr_cov *c, const gsdr_c64 *rows_dev, int n_rows, void *hip_stream) {
    const char *const me = "gsdr_cov_feed_device";
    if (const char *bad = object_fault(c)) return refuse(me, bad);
    if (n_rows < 0 || n_rows > c->max_rows) return refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows_dev) return refuse(me, "null buffer: rows_dev");
    if (reinterpret_cast<uintptr_t>(rows_dev) & 7u) return refuse(me, "rows_dev must be 8-byte aligned");
    if (!set_device(c)) return refuse(me, "hipSetDevice failed");
    CovDev *v = static_cast<CovDev *>(c->dev);
    gsdr::CovFeed f{};
    f.rows = reinterpret_cast<const float2 *>(rows_dev);
    f.axes = v->axes, f.D = v->D, f.S = v->S, f.G = v->G;
    f.n_rows = n_rows, f.n_ch = c->n_ch, f.n_var = c->n_var, f.lanes = c->lanes;
    f.row0 = c->total;
    const hipError_t e = gsdr::launch_cov_feed(f, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return result(me, e);
    c->total += n_rows;
    return 0;
}

int gsdr_cov_read_device(gsdr_cov *c, int kind, double *out_dev, double *mean_dev, void *hip_stream) {
    const char *const me = "gsdr_cov_read_device";
    if (const char *bad = object_fault(c)) return refuse(me, bad);
    if (!kind_ok(kind)) return refuse(me, "kind must be GSDR_COV_SUMS, GSDR_COV_COV or GSDR_COV_CORR");
    if (!out_dev) return refuse(me, "null buffer: out_dev");
    if (reinterpret_cast<uintptr_t>(out_dev) & 7u) return refuse(me, "out_dev must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(mean_dev) & 7u) return refuse(me, "mean_dev must be 8-byte aligned");
    if (!set_device(c)) return refuse(me, "hipSetDevice failed");
    return result(me, enqueue_read(c, kind, out_dev, mean_dev, static_cast<hipStream_t>(hip_stream)));
}

int gsdr_cov_read(gsdr_cov *c, int kind, double *out_host, double *mean_host, void *hip_stream) {
    const char *const me = "gsdr_cov_read";
    if (const char *bad = object_fault(c)) return refuse(me, bad);
    if (!kind_ok(kind)) return refuse(me, "kind must be GSDR_COV_SUMS, GSDR_COV_COV or GSDR_COV_CORR");
    if (!out_host) return refuse(me, "null buffer: out_host");
    if (!set_device(c)) return refuse(me, "hipSetDevice failed");
    CovDev *v = static_cast<CovDev *>(c->dev);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const size_t n_var = (size_t)c->n_var;
    const hipError_t e = enqueue_read(c, kind, v->out, mean_host ? static_cast<double *>(v->mean) : nullptr, st);
    return result(me, gsdr::fetch(e, st, {{out_host, v->out, n_var * n_var * sizeof(double)}, {mean_host, v->mean, n_var * sizeof(double)}}));
}

}  // extern "C"
