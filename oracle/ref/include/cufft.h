/*
 * Host stand-in for the cuFFT calls the reference makes.  TEST INFRASTRUCTURE
 * ONLY.  C2C only, as an unnormalised DFT accumulated in double and rounded to
 * float once: X[k] = sum_j x[j] exp(sign 2 pi i j k / n), sign -1 forward,
 * +1 inverse.  Zero inputs are skipped, so a sparse input (the tone comb) costs
 * n per non-zero entry.  In place is allowed.
 */
#ifndef GSDR_REF_CUFFT_H
#define GSDR_REF_CUFFT_H

#include <complex>
#include <vector>

#include "cuda_runtime.h"

typedef float2 cufftComplex;
typedef double2 cufftDoubleComplex;
typedef int cufftHandle;
typedef enum { CUFFT_SUCCESS = 0, CUFFT_INVALID_PLAN = 1, CUFFT_INVALID_VALUE = 4 } cufftResult;
typedef enum { CUFFT_R2C = 0x2a, CUFFT_C2R = 0x2c, CUFFT_C2C = 0x29 } cufftType;
#define CUFFT_FORWARD -1
#define CUFFT_INVERSE 1

struct ref_fft_plan {
    int n, batch, istride, idist, ostride, odist;
    bool live;
};
inline std::vector<ref_fft_plan> &ref_fft_plans()
{
    static std::vector<ref_fft_plan> plans;
    return plans;
}

inline cufftResult cufftPlanMany(cufftHandle *plan, int rank, int *n, int *inembed, int istride, int idist,
                                 int *onembed, int ostride, int odist, cufftType type, int batch)
{
    if (rank != 1 || type != CUFFT_C2C || n[0] < 1 || batch < 1) return CUFFT_INVALID_VALUE;
    ref_fft_plan p;
    p.n = n[0];
    p.batch = batch;
    /* as in cuFFT: with null embeddings the basic layout holds and the strides are ignored */
    p.istride = inembed ? istride : 1;
    p.idist = inembed ? idist : n[0];
    p.ostride = onembed ? ostride : 1;
    p.odist = onembed ? odist : n[0];
    p.live = true;
    ref_fft_plans().push_back(p);
    *plan = (cufftHandle)ref_fft_plans().size() - 1;
    return CUFFT_SUCCESS;
}
inline cufftResult cufftPlan1d(cufftHandle *plan, int n, cufftType type, int batch)
{
    return cufftPlanMany(plan, 1, &n, nullptr, 1, n, nullptr, 1, n, type, batch);
}
inline cufftResult cufftSetStream(cufftHandle, cudaStream_t) { return CUFFT_SUCCESS; }
inline cufftResult cufftDestroy(cufftHandle plan)
{
    if (plan < 0 || plan >= (int)ref_fft_plans().size() || !ref_fft_plans()[plan].live) return CUFFT_INVALID_PLAN;
    ref_fft_plans()[plan].live = false;
    return CUFFT_SUCCESS;
}

inline cufftResult cufftExecC2C(cufftHandle plan, cufftComplex *in, cufftComplex *out, int direction)
{
    if (plan < 0 || plan >= (int)ref_fft_plans().size() || !ref_fft_plans()[plan].live) return CUFFT_INVALID_PLAN;
    const ref_fft_plan p = ref_fft_plans()[plan];
    const long n = p.n;
    std::vector<std::complex<double>> tw(n), x(n), acc(n);
    for (long m = 0; m < n; ++m) {
        /* exp(sign 2 pi i m / n), the angle reduced exactly through the integer m */
        const double a = 2.0 * M_PI * (double)m / (double)n;
        tw[m] = std::complex<double>(std::cos(a), direction == CUFFT_FORWARD ? -std::sin(a) : std::sin(a));
    }
    for (int b = 0; b < p.batch; ++b) {
        for (long j = 0; j < n; ++j) {
            const cufftComplex &v = in[(size_t)b * p.idist + (size_t)j * p.istride];
            x[j] = std::complex<double>(v.x, v.y);
        }
        for (long k = 0; k < n; ++k) acc[k] = 0;
        for (long j = 0; j < n; ++j) {
            if (x[j] == std::complex<double>(0)) continue;
            long m = 0;
            for (long k = 0; k < n; ++k) {
                acc[k] += x[j] * tw[m];
                m += j;
                if (m >= n) m %= n;
            }
        }
        for (long k = 0; k < n; ++k) {
            cufftComplex &o = out[(size_t)b * p.odist + (size_t)k * p.ostride];
            o.x = (float)acc[k].real();
            o.y = (float)acc[k].imag();
        }
    }
    return CUFFT_SUCCESS;
}

#endif
