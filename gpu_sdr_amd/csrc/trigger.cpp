// trigger.cpp -- the device part of a trigger object (the contract: include/gsdr.h, "trigger on the device"): what it
// owns on the GPU and the sequencing of a feed.  Creation, the refusals of the arguments and the host twin are in
// trigger_host.cpp, the kernels in trigger_kernels.hip, the frame of every stage in stage_dev.h.
//
// A feed is three launches on the caller's stream and no host synchronisation.  Everything a feed inherits lives in two
// sets used in turn -- a feed reads set `cur` and writes the other one, as d_avg_acc does for the frame average -- so no
// kernel reads what another workgroup of the same launch writes.  What the HOST has to know of the stream is only the
// number of rows fed (which carried rows and records exist) and the length of the feed before (where its window ends);
// both are known without reading anything back.
#include <algorithm>
#include <string>

#include "stage_dev.h"
#include "trigger_kernels.h"

namespace gsdr {

struct TriggerDev : StageDev {
    DevBuf<float> levels;                    // [n_ch][6]
    DevBuf<gsdr_trigger_rec> rec[2];         // windows: post - 1 + max_rows records
    DevBuf<unsigned char> flag[2];           // ... and as many flag bytes, padded by the 64 the selection reads in one step
    DevBuf<float2> carry[2];                 // [pre + post - 1][n_ch]
    DevBuf<long long> last_hit;
    int cur = 0;                             // the set the next feed reads
    int n_prev = 0;                          // rows of the feed before
    // staging of gsdr_trigger_feed, made by its first call
    DevBuf<gsdr_trigger_event> events;
    DevBuf<float2> snippets;
    DevBuf<int> counts;
};

}  // namespace gsdr

using gsdr::refuse;
using gsdr::result;
using gsdr::set_device;
using gsdr::TriggerDev;

namespace {

// the checks both device feeds share; nullptr or the refusal
const char *feed_fault(const gsdr_trigger *t, int n_rows) {
    if (const char *bad = gsdr::object_fault(t, "a host object (GSDR_TRIGGER_HOST) takes gsdr_trigger_feed_host")) return bad;
    if (n_rows < 0 || n_rows > t->max_rows) return "n_rows must be in [0, max_rows]";
    return nullptr;
}

// the launches of one feed of n_rows >= 1 rows; advances the object
hipError_t enqueue(gsdr_trigger *t, const gsdr_c64 *rows_dev, int n_rows, gsdr_trigger_event *events_dev, gsdr_c64 *snippets_dev,
                   int *counts_dev, hipStream_t st) {
    TriggerDev *d = static_cast<TriggerDev *>(t->dev);
    const long long P = t->post - 1;
    gsdr::TriggerFeed f{};
    f.rows = reinterpret_cast<const float2 *>(rows_dev);
    f.n = n_rows, f.n_ch = t->n_ch, f.pre = t->pre, f.post = t->post, f.holdoff = t->holdoff, f.max_events = t->max_events;
    f.R0 = t->total;
    f.n_prev = d->n_prev;
    f.rec_valid = (int)std::min(t->total, P);
    f.levels = d->levels;
    f.rec_in = d->rec[d->cur], f.flag_in = d->flag[d->cur], f.carry_in = d->carry[d->cur];
    f.rec_out = d->rec[d->cur ^ 1], f.flag_out = d->flag[d->cur ^ 1], f.carry_out = d->carry[d->cur ^ 1];
    f.last_hit = d->last_hit;
    f.events = events_dev;
    f.snippets = reinterpret_cast<float2 *>(snippets_dev);
    f.counts = counts_dev;
    const hipError_t e = gsdr::launch_trigger_feed(f, st);
    if (e != hipSuccess) return e;
    d->cur ^= 1;
    d->n_prev = n_rows;
    t->total += n_rows;
    return hipSuccess;
}

}  // namespace

extern "C" {

int gsdr_trigger_dev_create_(gsdr_trigger *t, const gsdr_trigger_level *levels) {
    const size_t window = (size_t)(t->post - 1) + (size_t)t->max_rows;
    const size_t carry = (size_t)(t->pre + t->post - 1) * (size_t)t->n_ch;
    const std::string asked = "(n_ch, max_rows, pre + post: " + std::to_string((2 * carry * sizeof(float2) + 2 * window * 17) >> 20) + " MiB)";
    return gsdr::create_dev<TriggerDev>(t, "gsdr_trigger_create", asked, [&](TriggerDev &d) {
        bool ok = d.levels.alloc((size_t)t->n_ch * 6) == hipSuccess && d.last_hit.alloc_zeroed(1) == hipSuccess;
        for (int s = 0; ok && s < 2; ++s)
            ok = d.rec[s].alloc_zeroed(window) == hipSuccess && d.flag[s].alloc_zeroed(window + 64) == hipSuccess &&
                 d.carry[s].alloc_zeroed(carry) == hipSuccess;
        return ok && hipMemcpy(d.levels, levels, (size_t)t->n_ch * sizeof(gsdr_trigger_level), hipMemcpyHostToDevice) == hipSuccess;
    });
}

int gsdr_trigger_dev_set_levels_(gsdr_trigger *t, const gsdr_trigger_level *levels, void *hip_stream) {
    const char *const me = "gsdr_trigger_set_levels";
    if (!t->dev) return refuse(me, "not a device object");
    if (!set_device(t)) return refuse(me, "hipSetDevice failed");
    TriggerDev *d = static_cast<TriggerDev *>(t->dev);
    // behind the feeds already on the stream; the source is the caller's pageable or pinned memory, so wait for the copy:
    // the caller may reuse `levels` at once
    hipError_t e = hipMemcpyAsync(d->levels, levels, (size_t)t->n_ch * sizeof(gsdr_trigger_level), hipMemcpyHostToDevice,
                                  static_cast<hipStream_t>(hip_stream));
    if (e == hipSuccess) e = hipStreamSynchronize(static_cast<hipStream_t>(hip_stream));
    return result(me, e);
}

int gsdr_trigger_feed_device(gsdr_trigger *t, const gsdr_c64 *rows_dev, int n_rows, gsdr_trigger_event *events_dev,
                             gsdr_c64 *snippets_dev, int *counts_dev, void *hip_stream) {
    const char *const me = "gsdr_trigger_feed_device";
    if (const char *bad = feed_fault(t, n_rows)) return refuse(me, bad);
    if (!counts_dev || (n_rows > 0 && (!rows_dev || !events_dev || !snippets_dev))) return refuse(me, "null buffer");
    if (!set_device(t)) return refuse(me, "hipSetDevice failed");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const hipError_t e = n_rows == 0 ? hipMemsetAsync(counts_dev, 0, 2 * sizeof(int), st)
                                     : enqueue(t, rows_dev, n_rows, events_dev, snippets_dev, counts_dev, st);
    return result(me, e);
}

int gsdr_trigger_feed(gsdr_trigger *t, const gsdr_c64 *rows_dev, int n_rows, gsdr_trigger_event *events_host,
                      gsdr_c64 *snippets_host, int *n_dropped, void *hip_stream) {
    const char *const me = "gsdr_trigger_feed";
    if (const char *bad = feed_fault(t, n_rows)) return refuse(me, bad);
    if (n_dropped) *n_dropped = 0;
    if (n_rows == 0) return 0;
    if (!rows_dev || !events_host || !snippets_host) return refuse(me, "null buffer");
    if (!set_device(t)) return refuse(me, "hipSetDevice failed");
    TriggerDev *d = static_cast<TriggerDev *>(t->dev);
    const size_t snip = (size_t)(t->pre + t->post) * (size_t)t->n_ch;
    if (!d->counts) {
        if (d->events.alloc((size_t)t->max_events) != hipSuccess || d->snippets.alloc((size_t)t->max_events * snip) != hipSuccess ||
            d->counts.alloc(2) != hipSuccess) {
            (void)hipGetLastError();
            d->events.reset(), d->snippets.reset(), d->counts.reset();
            return refuse(me, "device allocation of the staging failed (max_events x (pre + post) x n_ch)");
        }
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    int counts[2] = {0, 0};
    hipError_t e = enqueue(t, rows_dev, n_rows, d->events, reinterpret_cast<gsdr_c64 *>(static_cast<float2 *>(d->snippets)),
                           d->counts, st);
    e = gsdr::fetch(e, st, {{counts, d->counts, sizeof(counts)}});
    // only what was emitted crosses to the host
    if (e == hipSuccess && counts[0] > 0) {
        e = hipMemcpy(events_host, d->events, (size_t)counts[0] * sizeof(gsdr_trigger_event), hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            e = hipMemcpy(snippets_host, d->snippets, (size_t)counts[0] * snip * sizeof(gsdr_c64), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return result(me, e);
    if (n_dropped) *n_dropped = counts[1];
    return counts[0];
}

}  // extern "C"
