// sweep.cpp -- the device part of a sweep object (the contract: include/gsdr.h, "VNA sweep accumulator on the device"):
// what it owns on the GPU, the one launch of a feed, the reads and the slope.  Creation, the refusals of the arguments,
// the counts and the host twin are in sweep_host.cpp, the kernels in sweep_kernels.hip, the frame of every stage in
// stage_dev.h.
//
// What the HOST has to know of the stream is only first_row and the number of rows fed: from them follow the points a
// feed touches and every n[p].  Nothing is read back by a feed.
#include <string>

#include "stage_dev.h"
#include "sweep_kernels.h"

namespace gsdr {

struct SweepDev : StageDev {
    DevBuf<double> acc;                      // [n_points][n_ch][4]
    DevBuf<double2> blocks;                  // [slope blocks][n_ch]: scratch of the slope
    DevBuf<double2> d;                       // [n_ch]: the slope
    DevBuf<float2> stage;                    // [2][n_points][n_ch]: what gsdr_sweep_read copies from; allocated by its first call
};

}  // namespace gsdr

using gsdr::refuse;
using gsdr::result;
using gsdr::set_device;
using gsdr::SweepDev;

namespace {

// nullptr or why a device entry cannot take this object
const char *object_fault(const gsdr_sweep *s) {
    return gsdr::object_fault(s, "a host object (GSDR_SWEEP_HOST) takes gsdr_sweep_feed_host and gsdr_sweep_read_host");
}

gsdr::SweepRead read_of(const gsdr_sweep *s) {
    gsdr::SweepRead r{};
    r.acc = static_cast<SweepDev *>(s->dev)->acc;
    r.n_ch = s->n_ch, r.n_points = s->n_points, r.group = s->group;
    r.a = gsdr_sweep_edge_of(s->first_row, s->n_points, s->group);
    r.b = gsdr_sweep_edge_of(s->first_row + s->total, s->n_points, s->group);
    return r;
}

}  // namespace

extern "C" {

int gsdr_sweep_dev_create_(gsdr_sweep *s) {
    const size_t cells = (size_t)s->n_points * (size_t)s->n_ch, nb = (size_t)gsdr_sweep_slope_blocks(s->n_points) * (size_t)s->n_ch;
    const size_t bytes = cells * 4 * sizeof(double) + (nb + (size_t)s->n_ch) * sizeof(double2);
    return gsdr::create_dev<SweepDev>(s, "gsdr_sweep_create", "(n_ch, n_points: " + std::to_string(bytes >> 20) + " MiB)", [&](SweepDev &v) {
        return v.acc.alloc_zeroed(cells * 4) == hipSuccess && v.blocks.alloc(nb) == hipSuccess && v.d.alloc((size_t)s->n_ch) == hipSuccess;
    });
}

int gsdr_sweep_dev_reset_(gsdr_sweep *s) {
    const char *const me = "gsdr_sweep_reset";
    if (!set_device(s)) return refuse(me, "hipSetDevice failed");
    SweepDev *v = static_cast<SweepDev *>(s->dev);
    return result(me, gsdr::zero_behind_all({{v->acc, (size_t)s->n_points * (size_t)s->n_ch * 4 * sizeof(double)}}));
}

int gsdr_sweep_dev_slope_(gsdr_sweep *s, double *d_host, void *hip_stream) {
    const char *const me = "gsdr_sweep_slope";
    if (!set_device(s)) return refuse(me, "hipSetDevice failed");
    SweepDev *v = static_cast<SweepDev *>(s->dev);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const hipError_t e = gsdr::launch_sweep_slope(read_of(s), v->blocks, v->d, st);
    return result(me, gsdr::fetch(e, st, {{d_host, v->d, (size_t)s->n_ch * sizeof(double2)}}));
}

int gsdr_sweep_feed_device(gsdr_sweep *s, const gsdr_c64 *rows_dev, int n_rows, void *hip_stream) {
    const char *const me = "gsdr_sweep_feed_device";
    if (const char *bad = object_fault(s)) return refuse(me, bad);
    if (n_rows < 0 || n_rows > GSDR_SWEEP_MAX_FEED) return refuse(me, "n_rows must be in [0, 16777216]");
    if (n_rows == 0) return 0;
    if (s->total > GSDR_SWEEP_MAX_ROWS - n_rows) return refuse(me, "n_rows: the stream would pass 2^61 rows");
    if (!rows_dev) return refuse(me, "null buffer: rows_dev");
    if (!set_device(s)) return refuse(me, "hipSetDevice failed");
    gsdr::SweepFeed f{};
    f.rows = reinterpret_cast<const float2 *>(rows_dev);
    f.acc = static_cast<SweepDev *>(s->dev)->acc;
    f.n = n_rows, f.n_ch = s->n_ch, f.n_points = s->n_points, f.group = s->group;
    f.row0 = s->first_row + s->total;
    const hipError_t e = gsdr::launch_sweep_feed(f, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return result(me, e);
    s->total += n_rows;
    return 0;
}

int gsdr_sweep_read_device(gsdr_sweep *s, gsdr_c64 *mean_dev, gsdr_c64 *var_dev, void *hip_stream) {
    const char *const me = "gsdr_sweep_read_device";
    if (const char *bad = object_fault(s)) return refuse(me, bad);
    if (!mean_dev) return refuse(me, "null buffer: mean_dev");
    if (!set_device(s)) return refuse(me, "hipSetDevice failed");
    const hipError_t e = gsdr::launch_sweep_read(read_of(s), reinterpret_cast<float2 *>(mean_dev), reinterpret_cast<float2 *>(var_dev),
                                                 static_cast<hipStream_t>(hip_stream));
    return result(me, e);
}

int gsdr_sweep_read(gsdr_sweep *s, gsdr_c64 *mean_host, gsdr_c64 *var_host, void *hip_stream) {
    const char *const me = "gsdr_sweep_read";
    if (const char *bad = object_fault(s)) return refuse(me, bad);
    if (!mean_host) return refuse(me, "null buffer: mean_host");
    if (!set_device(s)) return refuse(me, "hipSetDevice failed");
    SweepDev *v = static_cast<SweepDev *>(s->dev);
    const size_t cells = (size_t)s->n_points * (size_t)s->n_ch;
    if (!gsdr::staging_ready(v->stage, 2 * cells))
        return refuse(me, "device allocation failed (the staging of a read to the host: " + std::to_string((2 * cells * sizeof(float2)) >> 20) + " MiB)");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    float2 *mean = v->stage, *var = var_host ? mean + cells : nullptr;
    const hipError_t e = gsdr::launch_sweep_read(read_of(s), mean, var, st);
    return result(me, gsdr::fetch(e, st, {{mean_host, mean, cells * sizeof(float2)}, {var_host, var, cells * sizeof(float2)}}));
}

}  // extern "C"
