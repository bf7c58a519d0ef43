// stats.cpp -- the device part of a stats object (the contract: include/gsdr.h, "row statistics on the device"): what it
// owns on the GPU, the one launch of a feed, the reads and the way of the axes to the device.  Creation, the refusals of
// the arguments, the lanes rule, the levels and the host twin are in stats_host.cpp, the kernels in stats_kernels.hip,
// the frame of every stage in stage_dev.h.
//
// What the HOST has to know of the stream is only the number of rows fed: from it follows the chain of every row of a
// feed.  Nothing is read back by a feed.  The staging of the reads (a summary and GSDR_STATS_MAX_QUANTILES doubles per
// channel) is small and allocated at creation: no entry allocates.
#include <string>

#include "stage_dev.h"
#include "stats_kernels.h"

namespace gsdr {

struct StatsDev : StageDev {
    DevBuf<gsdr_stats_axis> axes;            // [n_ch]
    DevBuf<double> chains;                   // 24 bytes per (chain, channel): stats_chains_at
    DevBuf<unsigned long long> counts;       // [n_ch][n_bins + 3]
    DevBuf<gsdr_stats_summary> summary;      // [n_ch]: what gsdr_stats_read and the levels copy from
    DevBuf<double> quant;                    // [n_ch][GSDR_STATS_MAX_QUANTILES]: what the quantiles copy from
};

}  // namespace gsdr

using gsdr::refuse;
using gsdr::result;
using gsdr::set_device;
using gsdr::StatsDev;

namespace {

// nullptr or why a device entry cannot take this object
const char *object_fault(const gsdr_stats *s) {
    return gsdr::object_fault(s, "a host object (GSDR_STATS_HOST) takes gsdr_stats_feed_host and gsdr_stats_read_host");
}

size_t chains_of(const gsdr_stats *s) { return (size_t)s->lanes * (size_t)s->n_ch; }

size_t counters_of(const gsdr_stats *s) { return (size_t)s->n_ch * (size_t)(s->n_bins + 3); }

gsdr::StatsRead read_of(const gsdr_stats *s) {
    StatsDev *v = static_cast<StatsDev *>(s->dev);
    gsdr::StatsRead r{};
    r.axes = v->axes, r.chains = gsdr::stats_chains_at(v->chains, chains_of(s)), r.counts = v->counts;
    r.n_ch = s->n_ch, r.n_bins = s->n_bins, r.lanes = s->lanes;
    return r;
}

}  // namespace

extern "C" {

int gsdr_stats_dev_create_(gsdr_stats *s) {
    const size_t chains = chains_of(s), counters = counters_of(s), n_ch = (size_t)s->n_ch;
    const size_t bytes = chains * 24 + counters * 8 + n_ch * (sizeof(gsdr_stats_axis) + sizeof(gsdr_stats_summary) + GSDR_STATS_MAX_QUANTILES * sizeof(double));
    return gsdr::create_dev<StatsDev>(s, "gsdr_stats_create", "(n_ch, lanes, n_bins: " + std::to_string(bytes >> 20) + " MiB)", [&](StatsDev &v) {
        return v.axes.upload(s->axes) == hipSuccess && v.chains.alloc_zeroed(chains * 3) == hipSuccess && v.counts.alloc_zeroed(counters) == hipSuccess &&
               v.summary.alloc(n_ch) == hipSuccess && v.quant.alloc(n_ch * GSDR_STATS_MAX_QUANTILES) == hipSuccess;
    });
}

int gsdr_stats_dev_reset_(gsdr_stats *s, int upload) {
    const char *const me = "gsdr_stats_reset";
    if (!set_device(s)) return refuse(me, "hipSetDevice failed");
    StatsDev *v = static_cast<StatsDev *>(s->dev);
    // behind the first wait nothing reads the axes any more: the copy (from pageable memory: it returns when it is done)
    // cannot overtake a feed, and the wait that ends the zeroing covers it too
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess && upload) e = hipMemcpy(v->axes, s->axes.data(), s->axes.size() * sizeof(gsdr_stats_axis), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = gsdr::zero_behind_all({{v->chains, chains_of(s) * 24}, {v->counts, counters_of(s) * 8}});
    return result(me, e);
}

int gsdr_stats_dev_fetch_(gsdr_stats *s, const char *me, gsdr_stats_summary *summary, const double *pr, int n_p, double *quantiles,
                          unsigned long long *counts, void *hip_stream) {
    if (!set_device(s)) return refuse(me, "hipSetDevice failed");
    StatsDev *v = static_cast<StatsDev *>(s->dev);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    hipError_t e = hipSuccess;
    if (summary || quantiles) {
        gsdr::StatsRead r = read_of(s);
        r.summary = summary ? static_cast<gsdr_stats_summary *>(v->summary) : nullptr;
        r.quant = quantiles ? static_cast<double *>(v->quant) : nullptr;
        r.n_p = quantiles ? n_p : 0;
        for (int i = 0; i < r.n_p; ++i) r.pr[i] = pr[i];
        e = gsdr::launch_stats_read(r, st);
    }
    return result(me, gsdr::fetch(e, st, {{summary, v->summary, (size_t)s->n_ch * sizeof(gsdr_stats_summary)},
                                          {quantiles, v->quant, (size_t)s->n_ch * (size_t)n_p * sizeof(double)},
                                          {counts, v->counts, counters_of(s) * 8}}));
}

int gsdr_stats_feed_device(gsdr_stats *s, const gsdr_c64 *rows_dev, int n_rows, void *hip_stream) {
    const char *const me = "gsdr_stats_feed_device";
    if (const char *bad = object_fault(s)) return refuse(me, bad);
    if (n_rows < 0 || n_rows > s->max_rows) return refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows_dev) return refuse(me, "null buffer: rows_dev");
    if (reinterpret_cast<uintptr_t>(rows_dev) & 7u) return refuse(me, "rows_dev must be 8-byte aligned");
    if (!set_device(s)) return refuse(me, "hipSetDevice failed");
    StatsDev *v = static_cast<StatsDev *>(s->dev);
    gsdr::StatsFeed f{};
    f.rows = reinterpret_cast<const float2 *>(rows_dev);
    f.axes = v->axes, f.chains = gsdr::stats_chains_at(v->chains, chains_of(s)), f.counts = v->counts;
    f.n_rows = n_rows, f.n_ch = s->n_ch, f.n_bins = s->n_bins, f.lanes = s->lanes;
    f.row0 = s->total;
    const hipError_t e = gsdr::launch_stats_feed(f, static_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return result(me, e);
    s->total += n_rows;
    return 0;
}

int gsdr_stats_read_device(gsdr_stats *s, gsdr_stats_summary *summary_dev, void *hip_stream) {
    const char *const me = "gsdr_stats_read_device";
    if (const char *bad = object_fault(s)) return refuse(me, bad);
    if (!summary_dev) return refuse(me, "null buffer: summary_dev");
    if (reinterpret_cast<uintptr_t>(summary_dev) & 7u) return refuse(me, "summary_dev must be 8-byte aligned");
    if (!set_device(s)) return refuse(me, "hipSetDevice failed");
    gsdr::StatsRead r = read_of(s);
    r.summary = summary_dev;
    return result(me, gsdr::launch_stats_read(r, static_cast<hipStream_t>(hip_stream)));
}

int gsdr_stats_read(gsdr_stats *s, gsdr_stats_summary *summary_host, void *hip_stream) {
    const char *const me = "gsdr_stats_read";
    if (const char *bad = object_fault(s)) return refuse(me, bad);
    if (!summary_host) return refuse(me, "null buffer: summary_host");
    return gsdr_stats_dev_fetch_(s, me, summary_host, nullptr, 0, nullptr, nullptr, hip_stream);
}

}  // extern "C"
