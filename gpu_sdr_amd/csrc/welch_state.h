// welch_state.h -- the Welch accumulator (include/gsdr.h, "Welch spectra on the device") as welch_host.cpp and welch.cpp
// share it.  welch_host.cpp owns creation, the refusals, the host twin and the bookkeeping every object has; welch.cpp
// hangs the device part on `dev` through the hooks below (its release: stage_state.h).  No HIP here: welch_host.cpp is built without welch.cpp by a host
// compiler (tests/test_welch_sanitizers.py), where the hooks are absent and only host objects exist.
#ifndef GSDR_WELCH_STATE_H
#define GSDR_WELCH_STATE_H

#include <vector>

#include "../../include/gsdr.h"
#include "stage_state.h"

struct gsdr_welch {
    int n_ch = 0, max_rows = 0, nperseg = 0, step = 0, detrend = 0;
    int device = GSDR_WELCH_HOST;
    long long total = 0;                      // rows fed since creation / reset
    std::vector<float> window;                // nperseg taps, as given or the periodic Hann window
    double sum_w2 = 0.0;                      // sum of window[n]^2, in double from the float values
    // host twin (device == GSDR_WELCH_HOST)
    std::vector<double> pending;              // rows [pending_base, total) as re, im pairs, [row][channel]
    long long pending_base = 0;
    std::vector<double> acc;                  // [n_ch][3][nperseg / 2 + 1]: |X|^2, |Y|^2, Re X conj Y
    std::vector<double> msum;                 // [n_ch][2]: sum of the rows [0, n_seg * step)
    std::vector<double> tw;                   // (cos, -sin)(2 pi k / nperseg), k < nperseg / 2
    gsdr::StageDev *dev = nullptr;            // gsdr::WelchDev (welch.cpp)
};

// segments complete after `total` rows
inline long long gsdr_welch_segments_of(long long total, int nperseg, int step) {
    return total < nperseg ? 0 : (total - nperseg) / step + 1;
}

extern "C" {
// welch.cpp; weak in welch_host.cpp.  _create_: allocates and uploads, 0 or -1 with the message noted; it is called
// after every bound has been checked.  _reset_: zeroes the device accumulators (waits for the device).
int gsdr_welch_dev_create_(gsdr_welch *w);
int gsdr_welch_dev_reset_(gsdr_welch *w);
}

#endif
