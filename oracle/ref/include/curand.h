/* Host stand-in: the pinned paths generate no random numbers; the names only
 * have to parse.  TEST INFRASTRUCTURE ONLY. */
#ifndef GSDR_REF_CURAND_H
#define GSDR_REF_CURAND_H
typedef struct ref_curand_generator *curandGenerator_t;
#endif
