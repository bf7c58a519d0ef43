// host_util.h -- what the host sources of libgsdr.so share: demod.cpp (the RX handle) and txgen.cpp (the synthetic
// sources and the TX generator).  Internal to csrc/; nothing here is part of the C ABI.
#ifndef GSDR_HOST_UTIL_H
#define GSDR_HOST_UTIL_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/gsdr.h"
#include "ddc_kernels.h"
#include "dev_owner.h"

namespace gsdr {

// The message gsdr_last_error(NULL) returns: what the last call without a handle of its own (a creation, a TX or
// source entry, gsdr_note_error_) left on this thread.  One thread-local object, in demod.cpp.
std::string &create_error();

// compute units of the current device (256 when it cannot be asked)
inline int device_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        cus = 256;
    return cus;
}

// exp(-2*pi*i * ph/rate) for an exact integer phase, in double.
inline void phasor(unsigned long long ph, unsigned rate, double &re, double &im) {
    const double a = 2.0 * M_PI * ((double)ph / (double)rate);
    re = std::cos(a);
    im = -std::sin(a);
}

// f mod rate in [0, rate): the integer phase step of a tone, whatever the sign of f (rate > 0)
inline unsigned mod_rate(long long f, long long rate) {
    long long r = f % rate;
    if (r < 0) r += rate;
    return (unsigned)r;
}

// the chirp as the kernels take it
inline ChirpShape chirp_shape(const gsdr_chirp_param &cp) {
    ChirpShape cs{};
    cs.num_steps = cp.num_steps;
    cs.length = cp.length;
    cs.period = cp.num_steps * cp.length;
    cs.chirpness = cp.chirpness;
    cs.f0 = cp.f0;
    return cs;
}

}  // namespace gsdr

#endif
