// resmap.cpp -- the device part of a resmap object (the contract: include/gsdr.h, "resonator map on the device"): what
// it owns on the GPU, the one launch of a feed and the offsets' way to the device.  Creation, the refusals of the
// arguments, gsdr_resmap_constants and the host twin are in resmap_host.cpp, the kernel in resmap_kernels.hip, the
// frame of every stage in stage_dev.h.
//
// The object carries no stream state: a feed needs the tables and the caller's two pointers, nothing is read back.
//
// Offsets.  set_offsets copies them into a pinned block of the object and enqueues one copy to the device table on the
// caller's stream: feeds before it on the stream read the old table, feeds behind it the new one.  The pinned block is
// reused: a later set_offsets first waits for the event behind the earlier copy (and for nothing else).
#include <cstdint>
#include <cstring>
#include <string>

#include "resmap_kernels.h"
#include "stage_dev.h"

namespace gsdr {

// page-locked host memory, released with the owner
class PinnedDoubles {
    double *p_ = nullptr;

  public:
    PinnedDoubles() = default;
    PinnedDoubles(const PinnedDoubles &) = delete;
    PinnedDoubles &operator=(const PinnedDoubles &) = delete;
    ~PinnedDoubles() {
        if (p_) (void)hipHostFree(p_);
    }
    operator double *() const { return p_; }
    hipError_t alloc(size_t count) {
        const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p_), (count ? count : 1) * sizeof(double), hipHostMallocDefault);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
};

struct ResmapDev : StageDev {
    DevBuf<gsdr_resmap_col> cols;            // [n_out]
    DevBuf<double2> offs;                    // [n_out]
    DevBuf<int> channels;                    // [n_out]; empty where the list is the identity
    DevBuf<float2> stage;                    // [max_rows][n_out]: what gsdr_resmap_feed copies from; allocated by its first call
    PinnedDoubles pinned;                    // [n_out][2]: the source of the copy set_offsets enqueues
    Event copied;                            // behind that copy
    bool in_flight = false;                  // `copied` has been recorded
};

}  // namespace gsdr

using gsdr::refuse;
using gsdr::ResmapDev;
using gsdr::result;
using gsdr::set_device;

namespace {

// nullptr or why a device entry cannot take this object
const char *object_fault(const gsdr_resmap *r) { return gsdr::object_fault(r, "a host object (GSDR_RESMAP_HOST) takes gsdr_resmap_feed_host"); }

// the launch of one feed on st; n_rows, or -1 with the reason noted.  n_rows >= 1, the arguments checked.
int enqueue_feed(gsdr_resmap *r, const char *me, const gsdr_c64 *rows_dev, int n_rows, gsdr_c64 *out_dev, hipStream_t st) {
    ResmapDev *v = static_cast<ResmapDev *>(r->dev);
    gsdr::ResmapFeed f{};
    f.rows = reinterpret_cast<const float2 *>(rows_dev);
    f.out = reinterpret_cast<float2 *>(out_dev);
    f.cols = v->cols, f.offs = v->offs;
    f.channels = r->identity ? nullptr : static_cast<const int *>(v->channels);
    f.n_rows = n_rows, f.n_ch = r->n_ch, f.n_out = r->n_out, f.kind = r->kind;
    return result(me, gsdr::launch_resmap_feed(f, st), n_rows);
}

// nullptr, or what is wrong with the two extents of a feed of n_rows >= 1 rows
const char *extents_fault(const gsdr_resmap *r, const void *rows, int n_rows, const void *out) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(rows), b = reinterpret_cast<uintptr_t>(out);
    if ((a | b) & 7u) return "rows_dev and out_dev must be 8-byte aligned";
    if (a == b && r->identity) return nullptr;
    const uintptr_t na = (uintptr_t)n_rows * (uintptr_t)r->n_ch * sizeof(gsdr_c64), nb = (uintptr_t)n_rows * (uintptr_t)r->n_out * sizeof(gsdr_c64);
    if (a < b + nb && b < a + na) return "out_dev overlaps rows_dev (out_dev == rows_dev is allowed with the identity channel list only)";
    return nullptr;
}

}  // namespace

extern "C" {

int gsdr_resmap_dev_create_(gsdr_resmap *r) {
    const size_t n_out = (size_t)r->n_out;
    const size_t bytes = n_out * (sizeof(gsdr_resmap_col) + sizeof(double2) + (r->identity ? 0 : sizeof(int)));
    return gsdr::create_dev<ResmapDev>(r, "gsdr_resmap_create", "(n_out: " + std::to_string(bytes >> 20) + " MiB of tables)", [&](ResmapDev &v) {
        return v.cols.upload(r->cols) == hipSuccess && v.offs.alloc_zeroed(n_out) == hipSuccess &&
               (r->identity || v.channels.upload(r->channels) == hipSuccess) && v.pinned.alloc(2 * n_out) == hipSuccess &&
               hipEventCreateWithFlags(v.copied.out(), hipEventDisableTiming) == hipSuccess;
    });
}

int gsdr_resmap_dev_set_offsets_(gsdr_resmap *r, void *hip_stream) {
    const char *const me = "gsdr_resmap_set_offsets";
    if (!set_device(r)) return refuse(me, "hipSetDevice failed");
    ResmapDev *v = static_cast<ResmapDev *>(r->dev);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    const size_t bytes = (size_t)r->n_out * sizeof(double2);
    hipError_t e = v->in_flight ? hipEventSynchronize(v->copied) : hipSuccess;
    if (e == hipSuccess) {
        std::memcpy(v->pinned, r->offsets.data(), bytes);
        e = hipMemcpyAsync(v->offs, v->pinned, bytes, hipMemcpyHostToDevice, st);
    }
    if (e == hipSuccess) e = hipEventRecord(v->copied, st);
    if (e == hipSuccess) v->in_flight = true;
    return result(me, e);
}

int gsdr_resmap_feed_device(gsdr_resmap *r, const gsdr_c64 *rows_dev, int n_rows, gsdr_c64 *out_dev, void *hip_stream) {
    const char *const me = "gsdr_resmap_feed_device";
    if (const char *bad = object_fault(r)) return refuse(me, bad);
    if (n_rows < 0 || n_rows > r->max_rows) return refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows_dev) return refuse(me, "null buffer: rows_dev");
    if (!out_dev) return refuse(me, "null buffer: out_dev");
    if (const char *bad = extents_fault(r, rows_dev, n_rows, out_dev)) return refuse(me, bad);
    if (!set_device(r)) return refuse(me, "hipSetDevice failed");
    return enqueue_feed(r, me, rows_dev, n_rows, out_dev, static_cast<hipStream_t>(hip_stream));
}

int gsdr_resmap_feed(gsdr_resmap *r, const gsdr_c64 *rows_dev, int n_rows, gsdr_c64 *out_host, void *hip_stream) {
    const char *const me = "gsdr_resmap_feed";
    if (const char *bad = object_fault(r)) return refuse(me, bad);
    if (n_rows < 0 || n_rows > r->max_rows) return refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows_dev) return refuse(me, "null buffer: rows_dev");
    if (!out_host) return refuse(me, "null buffer: out_host");
    if (reinterpret_cast<uintptr_t>(rows_dev) & 7u) return refuse(me, "rows_dev must be 8-byte aligned");
    if (!set_device(r)) return refuse(me, "hipSetDevice failed");
    ResmapDev *v = static_cast<ResmapDev *>(r->dev);
    const size_t cells = (size_t)r->max_rows * (size_t)r->n_out;
    if (!gsdr::staging_ready(v->stage, cells))
        return refuse(me, "device allocation failed (the staging of a feed to the host, max_rows n_out: " + std::to_string((cells * sizeof(float2)) >> 20) + " MiB)");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (enqueue_feed(r, me, rows_dev, n_rows, reinterpret_cast<gsdr_c64 *>((float2 *)v->stage), st) < 0) return -1;
    return result(me, gsdr::fetch(hipSuccess, st, {{out_host, v->stage, (size_t)n_rows * (size_t)r->n_out * sizeof(gsdr_c64)}}), n_rows);
}

}  // extern "C"
