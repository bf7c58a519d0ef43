/* Host stand-in: the state type and the two device calls the reference's
 * (unpinned) noise kernels name.  They produce no randomness and are never
 * reached from the pinned paths.  TEST INFRASTRUCTURE ONLY. */
#ifndef GSDR_REF_CURAND_KERNEL_H
#define GSDR_REF_CURAND_KERNEL_H
#include <cstdlib>
#include "curand.h"
struct curandState { unsigned long long s; };
inline void curand_init(unsigned long long, unsigned long long, unsigned long long, curandState *) { std::abort(); }
inline float curand_uniform(curandState *) { std::abort(); }
#endif
