// chirp_plan.h -- which form of the chirp lock-in runs for a call, decided in one place: launch_chirp_lockin and
// launch_chirp_multi_lockin (chirp_kernels.hip) launch what chirp_lockin_plan says, gsdr_chirp_lockin_plan
// (host_logic.cpp) shows it to a caller without a GPU.  No HIP here: host_logic.cpp is built alone by a host compiler.
#ifndef GSDR_CHIRP_PLAN_H
#define GSDR_CHIRP_PLAN_H

namespace gsdr {

// the values of GSDR_CHIRP_FORM_* (include/gsdr.h)
enum ChirpForm { kChirpPlain = 0, kChirpSplit = 1, kChirpGeneric = 2 };

struct ChirpPlan {
    int form = -1;              // a ChirpForm; -1: nothing was launched
    long long parts = 1;        // waves per point (split: >= 2, their partial sums added by the sum kernel)
    long long per_part = 0;     // stretches of 256 samples per wave; generic: 0, that kernel walks samples
};

// the 32-bit fast kernels cover num_steps, length and period below 2^31 / 2^32
inline bool chirp_plan_fits_32(unsigned long long num_steps, unsigned long long length, unsigned long long period) {
    return period < 0xffffffffull && num_steps < 0x7fffffffull && length < 0x800000ull;
}

// The lock-in of `valid` (>= 1) points of ppt samples each, the first at chirp index index0, for `chirps` chirps at
// once; partial_cap: float2 slots for partial sums (0: none).
//   generic: the fast kernels need windows made of whole steps that start on a step boundary -- true for every
//            window the demodulator forms (ppt = length * decim, see enqueue_chirp) -- and a sweep that fits 32 bits;
//   split:   few points with many samples each: a point's total = decim * ceil(length / 256) stretches are dealt to
//            `parts` waves, ~4096 waves in the launch, at least four stretches per wave, a point's partial sums
//            (parts * chirps slots) inside the buffer (split_on false, GSDR_CHIRP_SPLIT=0: never);
//   plain:   a wave per point.
inline ChirpPlan chirp_lockin_plan(bool fits_32, unsigned long long length, long long ppt, unsigned long long index0,
                                   long long valid, int chirps, bool split_on, long long partial_cap) {
    ChirpPlan p;
    if (!(fits_32 && length >= 1 && ppt % (long long)length == 0 && index0 % length == 0)) {
        p.form = kChirpGeneric;
        return p;
    }
    const long long decim = ppt / (long long)length, nst = ((long long)length + 255) / 256, total = decim * nst;
    p.form = kChirpPlain;
    p.per_part = total;
    if (split_on && partial_cap > 0 && valid >= 1 && valid <= 512 && chirps >= 1) {
        long long want = (4096 + valid - 1) / valid;
        if (want > total / 4) want = total / 4;
        if (want > partial_cap / (valid * chirps)) want = partial_cap / (valid * chirps);
        if (want >= 2 && total >= 16 && total < 0x7fffffffLL) {
            p.form = kChirpSplit;
            p.per_part = (total + want - 1) / want;
            p.parts = (total + p.per_part - 1) / p.per_part;
        }
    }
    return p;
}

}  // namespace gsdr

#endif
