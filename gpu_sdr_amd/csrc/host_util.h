// host_util.h -- what the host sources of libgsdr.so share: demod.cpp and its demod_*.cpp (the RX handle) and txgen.cpp (the synthetic
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

static_assert(kMultiChirpMax == GSDR_MULTI_CHIRP_MAX, "the kernels' tables hold GSDR_MULTI_CHIRP_MAX chirps");

// What a GSDR_CREATE_MULTI_CHIRP request of C > 1 chirps must satisfy, RX and TX alike (include/gsdr.h, "several chirps
// in one handle"): nullptr, or the refusal.  Looks at the parameters only.
inline const char *multi_chirp_fault(const gsdr_param_c *p, int C) {
    if (C > GSDR_MULTI_CHIRP_MAX) return "multi-chirp takes at most GSDR_MULTI_CHIRP_MAX (16) chirps";
    if (!(p->n_freq >= C && p->n_chirp_f >= C && p->freq && p->chirp_f))
        return "CHIRP needs freq[] and chirp_f[] for every wave_type entry";
    // one sweep law for all: one entry, or C equal ones
    auto shared = [C](const auto *v, int n) {
        if (!v || (n != 1 && n != C)) return false;
        for (int i = 1; i < n; ++i)
            if (!(v[i] == v[0])) return false;
        return true;
    };
    if (!shared(p->swipe_s, p->n_swipe_s) || !shared(p->chirp_t, p->n_chirp_t))
        return "multi-chirp needs one swipe_s and one chirp_t for all chirps";
    return nullptr;
}

// The chirps of a multi-chirp handle or call as the kernels take them: the common steps from cp[0], f0 and chirpness
// of each.  nullptr, or why not.
inline const char *multi_chirp_shape(const gsdr_chirp_param *cp, int C, MultiChirp &mc) {
    if (C < 1 || C > GSDR_MULTI_CHIRP_MAX) return "the number of chirps must be in [1, GSDR_MULTI_CHIRP_MAX]";
    if (cp[0].num_steps < 1 || cp[0].length < 1 || cp[0].num_steps > 0x7fffffffffffffffULL / cp[0].length)
        return "chirp period overflows";
    mc = MultiChirp{};
    mc.num_steps = cp[0].num_steps;
    mc.length = cp[0].length;
    mc.period = cp[0].num_steps * cp[0].length;
    mc.n = C;
    for (int c = 0; c < C; ++c) {
        if (cp[c].num_steps != cp[0].num_steps || cp[c].length != cp[0].length)
            return "the chirps must share num_steps and length";
        mc.f0[c] = cp[c].f0;
        mc.chirpness[c] = cp[c].chirpness;
    }
    return nullptr;
}

}  // namespace gsdr

#endif
