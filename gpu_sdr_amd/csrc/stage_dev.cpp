// stage_dev.cpp -- the one release hook of the six stages (stage_state.h): what gsdr_X_close of X_host.cpp calls
// for an object with a device part, whichever stage it belongs to.
#include "stage_dev.h"

extern "C" void gsdr_stage_dev_close_(int device, gsdr::StageDev *dev) {
    if (device >= 0) (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();                    // the owners order nothing (dev_owner.h)
    delete dev;
}
