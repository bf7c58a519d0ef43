// stage_state.h -- what the seven objects behind demodulated rows (gsdr_trigger_*, gsdr_welch_*, gsdr_decim_*,
// gsdr_sweep_*, gsdr_resmap_*, gsdr_stats_*, gsdr_cov_*: the STAGES) share between their host sources (X_host.cpp) and
// their device sources: the type of `dev`, the one release hook, the host side's refusal, the device_index check of every
// create, the two macros that keep a host twin's arithmetic uncontracted and the real projection of a sample that the
// stats and the cov object share.  The X_state.h of each stage includes it.  No HIP
// here: the X_host.cpp are built without the device sources by a host compiler (tests/test_*_sanitizers.py), where the
// hooks are absent and only host objects exist.
#ifndef GSDR_STAGE_STATE_H
#define GSDR_STAGE_STATE_H

#include <string>

#include "../../include/gsdr.h"

// A function whose sums and products must stay the IEEE operations they are written as (the host twins, bit for bit
// what the kernels give) carries both: GSDR_NO_CONTRACT in front of it, for gcc, and GSDR_NO_CONTRACT_BODY as the first
// statement of its body, for clang.
#if defined(__clang__)
#define GSDR_NO_CONTRACT
#define GSDR_NO_CONTRACT_BODY _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define GSDR_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#define GSDR_NO_CONTRACT_BODY
#else
#define GSDR_NO_CONTRACT
#define GSDR_NO_CONTRACT_BODY
#endif

// An inline function of a law that a kernel and a host twin both compile, with contraction off on either side (the
// pragma inside the body for clang and hipcc, the attribute for gcc).
#if defined(__HIPCC__)
#define GSDR_STAGE_HD __host__ __device__ inline __attribute__((always_inline))
#elif defined(__GNUC__) && !defined(__clang__)
#define GSDR_STAGE_HD inline __attribute__((optimize("fp-contract=off")))
#else
#define GSDR_STAGE_HD inline
#endif

static_assert(GSDR_TRIGGER_HOST == -2 && GSDR_WELCH_HOST == -2 && GSDR_DECIM_HOST == -2 && GSDR_SWEEP_HOST == -2 && GSDR_RESMAP_HOST == -2 &&
                  GSDR_STATS_HOST == -2 && GSDR_COV_HOST == -2,
              "every stage names its host twin by the same device_index");

namespace gsdr {

constexpr int kStageHost = -2;                // GSDR_X_HOST of every stage

// What a stage owns on the GPU: X.cpp derives its XDev from this and hangs it on `dev` of the object.  The destructor is
// all that X_host.cpp and the release hook need of it.
struct StageDev {
    virtual ~StageDev() = default;
};

}  // namespace gsdr

// The real projection of one sample x + iy, the trigger's q: five float32 operations, each rounded, nothing fused.  The
// stats object (gsdr_stats_sample) and the cov object (gsdr_cov_sample) both call this text.
GSDR_STAGE_HD float gsdr_stage_project(float bx, float by, float dx, float dy, float x, float y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float t0 = x - bx;
    const float t1 = y - by;
    const float p0 = t0 * dx;
    const float p1 = t1 * dy;
    return p0 + p1;
}

extern "C" {
// demod.cpp keeps the text for gsdr_last_error(NULL); a host-only build (no demod.cpp) has nobody to tell
void gsdr_note_error_(const char *msg) __attribute__((weak));
// stage_dev.cpp; weak in stage_host.h.  Waits for the device, then releases what `dev` owns.
void gsdr_stage_dev_close_(int device, gsdr::StageDev *dev);
}

namespace gsdr {

// The refusal of a host-side entry: notes "entry: what" for gsdr_last_error(NULL), returns -1.
inline int stage_refuse(const char *entry, const std::string &what) {
    const std::string msg = std::string(entry) + ": " + what;
    if (gsdr_note_error_) gsdr_note_error_(msg.c_str());
    return -1;
}

// The two device_index checks of every create: "" or the refusal.  host_name is the stage's GSDR_X_HOST as the caller
// writes it; has_device_part is false in a build without X.cpp.
inline std::string stage_device_fault(int device_index, const char *host_name, bool has_device_part) {
    if (device_index < kStageHost) return std::string("device_index must be >= -1 or ") + host_name;
    if (device_index != kStageHost && !has_device_part) return std::string("device_index: this build has host objects only (") + host_name + ")";
    return std::string();
}

}  // namespace gsdr

#endif
