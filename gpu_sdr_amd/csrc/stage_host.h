// stage_host.h -- what the host sources of the seven stages (trigger_host.cpp, welch_host.cpp, decim_host.cpp,
// sweep_host.cpp, resmap_host.cpp, stats_host.cpp, cov_host.cpp; stage_state.h) share: the frame of every create, the object check of
// a host entry and the close.  The counterpart of stage_dev.h; only the X_host.cpp include it, because it declares the
// release hook weak: in a build without stage_dev.cpp the hook is absent and only host objects exist.  No HIP here.
#ifndef GSDR_STAGE_HOST_H
#define GSDR_STAGE_HOST_H

#include <new>
#include <string>

#include "stage_state.h"

extern "C" void gsdr_stage_dev_close_(int device, gsdr::StageDev *dev) __attribute__((weak));   // stage_dev.cpp

namespace {

using gsdr::stage_device_fault;
using gsdr::stage_refuse;

// The frame of every gsdr_X_create behind its argument checks.  Refuses `bad` where there is one; makes the object and
// sets its device; lets fill(*s) set the fields and fill the host vectors (a bad_alloc of its is refused as no_memory);
// lets dev_create(s) hang the device part on a device object (0, or not 0 with the reason noted).  The object, or
// nullptr with the refusal noted and nothing kept.
template <class Stage, class Fill, class DevCreate>
Stage *stage_create(const char *me, const std::string &bad, int device_index, const std::string &no_memory, Fill fill, DevCreate dev_create) {
    Stage *s = bad.empty() ? new (std::nothrow) Stage() : nullptr;
    if (!s) {
        stage_refuse(me, bad.empty() ? "out of memory" : bad);
        return nullptr;
    }
    s->device = device_index;
    try {
        fill(*s);
    } catch (const std::bad_alloc &) {
        delete s;
        stage_refuse(me, no_memory);
        return nullptr;
    }
    if (device_index != gsdr::kStageHost && dev_create(s) != 0) {
        delete s;
        return nullptr;
    }
    return s;
}

// nullptr or why a host entry cannot take this object (the host side of gsdr::object_fault, stage_dev.h); `hint` names
// the entries a device object takes
template <class Stage>
const char *stage_host_fault(const Stage *s, const char *hint) {
    if (!s) return "null object";
    return s->device != gsdr::kStageHost ? hint : nullptr;
}

// gsdr_X_close of every stage: the device part first (the hook waits for the device), then the object
template <class Stage>
void stage_close(Stage *s) {
    if (!s) return;
    if (s->dev && gsdr_stage_dev_close_) gsdr_stage_dev_close_(s->device, s->dev);
    delete s;
}

}  // namespace

#endif
