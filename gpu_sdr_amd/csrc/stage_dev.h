// stage_dev.h -- what the device sources of the seven stages (trigger.cpp, welch.cpp, decim.cpp, sweep.cpp, resmap.cpp,
// stats.cpp, cov.cpp; stage_state.h) share: the refusal, the choice of the device, the object check of a device entry, the creation of the
// device part, the zeroing of a reset and the way of staged results to the host.  What differs from stage to stage --
// the buffers, the launches, the checks of the arguments -- stays in X.cpp.  Internal to csrc/.
#ifndef GSDR_STAGE_DEV_H
#define GSDR_STAGE_DEV_H

#include <initializer_list>
#include <string>

#include "host_util.h"
#include "stage_state.h"

namespace gsdr {

// The refusal of a device-side entry: leaves "entry: what" for gsdr_last_error(NULL), returns -1.
inline int refuse(const char *entry, const std::string &what) {
    create_error() = std::string(entry) + ": " + what;
    return -1;
}

// What an entry returns behind its HIP calls: v, or the refusal with HIP's own words.
inline int result(const char *entry, hipError_t e, int v = 0) { return e == hipSuccess ? v : refuse(entry, hipGetErrorString(e)); }

// The device of a stage object becomes the thread's current one (-1: whichever is current).
template <class Stage>
bool set_device(const Stage *s) {
    return s->device < 0 || hipSetDevice(s->device) == hipSuccess;
}

// nullptr or why a device entry cannot take this object; `hint` names the entries a host object takes
template <class Stage>
const char *object_fault(const Stage *s, const char *hint) {
    if (!s) return "null object";
    if (s->device == kStageHost || !s->dev) return hint;
    return nullptr;
}

// The creation of a stage's device part, behind the bounds X_host.cpp has checked: chooses the device, hangs a new
// Dev on s->dev and lets `allocate(Dev &)` make and fill what it owns (true: every step succeeded).  0, or -1 with
// "device allocation failed " + asked noted, nothing kept and s->dev null again.
template <class Dev, class Stage, class Allocate>
int create_dev(Stage *s, const char *me, const std::string &asked, Allocate allocate) {
    if (s->device >= 0 && hipSetDevice(s->device) != hipSuccess) return refuse(me, "device_index: hipSetDevice failed (no such GPU?)");
    Dev *d = new Dev();
    s->dev = d;
    // hipMemset returns before the fill has run, and a stage's feeds run on the caller's stream, which need not wait for
    // the null stream (torch's side streams and this library's own do not): without this wait the zeroing of a carried
    // buffer could land after the first feed had written it (demod.cpp waits behind its create for the same reason).
    if (!(allocate(*d) && hipDeviceSynchronize() == hipSuccess)) {
        (void)hipGetLastError();
        delete d;
        s->dev = nullptr;
        return refuse(me, "device allocation failed " + asked);
    }
    return 0;
}

// The zeroing of a reset.  Wait, zero, wait: the feeds and reads in flight on any stream are done with the sums before
// they are cleared, and the clearing (hipMemset returns before the fill has run) is done before a later feed adds to
// them.
struct DevSpan {
    void *p;
    size_t bytes;
};
inline hipError_t zero_behind_all(std::initializer_list<DevSpan> spans) {
    hipError_t e = hipDeviceSynchronize();
    for (const DevSpan &s : spans)
        if (e == hipSuccess) e = hipMemset(s.p, 0, s.bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e;
}

// The staging of an entry that returns to the host, allocated by its first call: false (nothing kept) where that fails.
template <class T>
bool staging_ready(DevBuf<T> &stage, size_t count) {
    if (stage) return true;
    if (stage.alloc(count) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

// The tail of an entry that returns to the host: behind what it enqueued on st (e: how that went) the copies of what
// was staged -- one with a null destination or no bytes is left out -- and the wait for the stream.
struct ToHost {
    void *dst;
    const void *src;
    size_t bytes;
};
inline hipError_t fetch(hipError_t e, hipStream_t st, std::initializer_list<ToHost> copies) {
    for (const ToHost &c : copies)
        if (e == hipSuccess && c.dst && c.bytes) e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

}  // namespace gsdr

#endif
