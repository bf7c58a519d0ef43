// trigger_state.h -- the trigger object (include/gsdr.h, "trigger on the device") as trigger_host.cpp and trigger.cpp
// share it.  trigger_host.cpp owns creation, the refusals, the host twin and the bookkeeping every object has;
// trigger.cpp hangs the device part on `dev` through the two hooks below (its release: stage_state.h).  No HIP here:
// trigger_host.cpp is built without trigger.cpp by a host compiler (tests/test_trigger_sanitizers.py), where the hooks are absent and
// only host objects exist.
#ifndef GSDR_TRIGGER_STATE_H
#define GSDR_TRIGGER_STATE_H

#include <vector>

#include "../../include/gsdr.h"
#include "stage_state.h"

// what a row leaves behind: the event fields without the row number, n_hit == 0 for a row that does not hit
struct gsdr_trigger_rec {
    int channel, side;
    float q;
    int n_hit;
};

struct gsdr_trigger {
    int n_ch = 0, max_rows = 0, pre = 0, post = 0, holdoff = 0, max_events = 0;
    int device = GSDR_TRIGGER_HOST;
    long long total = 0;                      // rows fed since creation / reset
    // host twin (device == GSDR_TRIGGER_HOST)
    std::vector<gsdr_trigger_level> levels;
    std::vector<gsdr_c64> carry;              // the last pre + post - 1 rows, right-aligned
    std::vector<gsdr_trigger_rec> recs;       // records of the last post - 1 rows, right-aligned
    std::vector<unsigned char> trig;          // ... and whether each was a trigger
    long long last_hit = -1;                  // the last hitting row, -1: none yet
    gsdr::StageDev *dev = nullptr;            // gsdr::TriggerDev (trigger.cpp)
};

extern "C" {
// trigger.cpp; weak in trigger_host.cpp.  _create_: allocates and uploads, 0 or -1 with the message noted; it is called
// after every bound has been checked.
int gsdr_trigger_dev_create_(gsdr_trigger *t, const gsdr_trigger_level *levels);
int gsdr_trigger_dev_set_levels_(gsdr_trigger *t, const gsdr_trigger_level *levels, void *hip_stream);
}

#endif
