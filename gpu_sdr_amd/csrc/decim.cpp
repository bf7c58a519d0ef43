// decim.cpp -- the device part of a decim object (the contract: include/gsdr.h, "FIR decimation on the device"): what
// it owns on the GPU and the sequencing of a feed.  Creation, the refusals of the arguments, the default taps and the
// host twin are in decim_host.cpp, the kernels in decim_kernels.hip, the frame of every stage in stage_dev.h.
//
// A feed is two launches on the caller's stream (one when it completes no output row) and no host synchronisation.
// What the HOST has to know of the stream is only the number of rows fed: from it follow the blocks the feed touches,
// their ring slots and the output rows it completes.  Nothing is read back.
//
// The carried state is the ring of chunk sums (decim_state.h).  It needs no second copy: a (block, chunk, channel)
// entry is read and written by one thread of the first launch, and the second launch only reads the ring.
#include <algorithm>
#include <string>
#include <vector>

#include "decim_kernels.h"
#include "stage_dev.h"

namespace gsdr {

struct DecimDev : StageDev {
    DevBuf<float2> ring;                     // [ring_blocks][F][n_ch]
    DevBuf<float> taps;                      // [F q + kDecimTapsPad]: zeros, the taps, zeros (decim_kernels.h)
    DevBuf<float2> out;                      // [out_capacity][n_ch]: what gsdr_decim_feed copies from
};

}  // namespace gsdr

using gsdr::DecimDev;
using gsdr::refuse;
using gsdr::result;
using gsdr::set_device;

namespace {

// nullptr or why a device entry cannot take this object
const char *object_fault(const gsdr_decim *d) { return gsdr::object_fault(d, "a host object (GSDR_DECIM_HOST) takes gsdr_decim_feed_host"); }

// the launches of one feed on st; the rows emitted, or -1 with the reason noted.  n_rows >= 1, the arguments checked.
int enqueue_feed(gsdr_decim *d, const char *me, const gsdr_c64 *rows_dev, int n_rows, gsdr_c64 *out_dev, hipStream_t st) {
    DecimDev *v = static_cast<DecimDev *>(d->dev);
    const long long o0 = gsdr_decim_out_of(d->total, d->offset, d->q), o1 = gsdr_decim_out_of(d->total + n_rows, d->offset, d->q);
    gsdr::DecimFeed f{};
    f.rows = reinterpret_cast<const float2 *>(rows_dev);
    f.out = reinterpret_cast<float2 *>(out_dev);
    f.ring = v->ring, f.taps = v->taps;
    f.n = n_rows, f.n_ch = d->n_ch, f.q = d->q, f.T = d->n_taps, f.F = d->F;
    f.ring_blocks = (unsigned)d->ring_blocks;
    f.first_row = d->total;
    f.r0 = gsdr_decim_r0(d->offset, d->q);
    f.n_emit = (int)(o1 - o0);
    f.k_out = o0 + d->offset / d->q;
    const hipError_t e = gsdr::launch_decim_feed(f, st);
    if (e != hipSuccess) return result(me, e);
    d->total += n_rows;
    return f.n_emit;
}

}  // namespace

extern "C" {

int gsdr_decim_dev_create_(gsdr_decim *d) {
    const size_t n_ch = (size_t)d->n_ch, F = (size_t)d->F, q = (size_t)d->q, T = (size_t)d->n_taps;
    const size_t ring = (size_t)d->ring_blocks * F * n_ch, out = (size_t)gsdr_decim_out_capacity(d) * n_ch;
    const size_t bytes = (ring + out) * sizeof(float2) + (F * q + (size_t)gsdr::kDecimTapsPad) * sizeof(float);
    const std::string asked = "(n_ch, max_rows, q, n_taps: " + std::to_string(bytes >> 20) + " MiB)";
    std::vector<float> padded(F * q + (size_t)gsdr::kDecimTapsPad, 0.f);
    std::copy(d->taps.begin(), d->taps.end(), padded.begin() + (std::ptrdiff_t)(F * q - T));
    // (the ring needs no clearing: a block's sums start at +0 with its first row)
    return gsdr::create_dev<DecimDev>(d, "gsdr_decim_create", asked, [&](DecimDev &v) {
        return v.ring.alloc(ring) == hipSuccess && v.out.alloc(out) == hipSuccess && v.taps.upload(padded) == hipSuccess;
    });
}

int gsdr_decim_feed_device(gsdr_decim *d, const gsdr_c64 *rows_dev, int n_rows, gsdr_c64 *out_dev, void *hip_stream) {
    const char *const me = "gsdr_decim_feed_device";
    if (const char *bad = object_fault(d)) return refuse(me, bad);
    if (n_rows < 0 || n_rows > d->max_rows) return refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows_dev) return refuse(me, "null buffer: rows_dev");
    if (!out_dev && gsdr_decim_next_rows(d, n_rows) > 0) return refuse(me, "null buffer: out_dev");
    if (!set_device(d)) return refuse(me, "hipSetDevice failed");
    return enqueue_feed(d, me, rows_dev, n_rows, out_dev, static_cast<hipStream_t>(hip_stream));
}

int gsdr_decim_feed(gsdr_decim *d, const gsdr_c64 *rows_dev, int n_rows, gsdr_c64 *out_host, void *hip_stream) {
    const char *const me = "gsdr_decim_feed";
    if (const char *bad = object_fault(d)) return refuse(me, bad);
    if (n_rows < 0 || n_rows > d->max_rows) return refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows_dev) return refuse(me, "null buffer: rows_dev");
    if (!out_host && gsdr_decim_next_rows(d, n_rows) > 0) return refuse(me, "null buffer: out_host");
    if (!set_device(d)) return refuse(me, "hipSetDevice failed");
    DecimDev *v = static_cast<DecimDev *>(d->dev);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const int emitted = enqueue_feed(d, me, rows_dev, n_rows, reinterpret_cast<gsdr_c64 *>((float2 *)v->out), st);
    if (emitted < 0) return -1;
    return result(me, gsdr::fetch(hipSuccess, st, {{out_host, v->out, (size_t)emitted * (size_t)d->n_ch * sizeof(gsdr_c64)}}), emitted);
}

}  // extern "C"
