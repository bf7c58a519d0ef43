/*
 * Host stand-in for the cuBLAS calls the reference makes.  TEST INFRASTRUCTURE
 * ONLY.  Column-major as in cuBLAS; every output element is accumulated in
 * double and rounded to float once.  OP_T is the plain transpose (no
 * conjugate), as in cuBLAS.
 */
#ifndef GSDR_REF_CUBLAS_V2_H
#define GSDR_REF_CUBLAS_V2_H

#include <complex>
#include <set>

#include "cuda_runtime.h"

#define CUBLAS_API_H_

typedef enum {
    CUBLAS_STATUS_SUCCESS = 0, CUBLAS_STATUS_NOT_INITIALIZED = 1, CUBLAS_STATUS_ALLOC_FAILED = 3,
    CUBLAS_STATUS_INVALID_VALUE = 7, CUBLAS_STATUS_ARCH_MISMATCH = 8, CUBLAS_STATUS_MAPPING_ERROR = 11,
    CUBLAS_STATUS_EXECUTION_FAILED = 13, CUBLAS_STATUS_INTERNAL_ERROR = 14, CUBLAS_STATUS_NOT_SUPPORTED = 15
} cublasStatus_t;
typedef enum { CUBLAS_OP_N = 0, CUBLAS_OP_T = 1, CUBLAS_OP_C = 2 } cublasOperation_t;
typedef struct ref_cublas_context { int unused; } *cublasHandle_t;

/* live handles: destroying one that was never created fails, as in cuBLAS (the reference's
 * TONES / NOISE close() destroys a handle it never created) */
inline std::set<cublasHandle_t> &ref_cublas_handles()
{
    static std::set<cublasHandle_t> live;
    return live;
}
inline cublasStatus_t cublasCreate(cublasHandle_t *h)
{
    *h = new ref_cublas_context();
    ref_cublas_handles().insert(*h);
    return CUBLAS_STATUS_SUCCESS;
}
inline cublasStatus_t cublasDestroy(cublasHandle_t h)
{
    if (!ref_cublas_handles().erase(h)) return CUBLAS_STATUS_NOT_INITIALIZED;
    delete h;
    return CUBLAS_STATUS_SUCCESS;
}
inline cublasStatus_t cublasSetStream(cublasHandle_t, cudaStream_t) { return CUBLAS_STATUS_SUCCESS; }

namespace refblas {
typedef std::complex<double> zd;
inline zd z(const float2 &a) { return zd(a.x, a.y); }
inline zd z(const double2 &a) { return zd(a.x, a.y); }
inline void put(float2 &o, zd v) { o.x = (float)v.real(); o.y = (float)v.imag(); }
inline void put(double2 &o, zd v) { o.x = v.real(); o.y = v.imag(); }
/* element (i, j) of op(A), A column-major with leading dimension lda */
template <typename T>
inline zd at(const T *A, int lda, cublasOperation_t op, int i, int j)
{
    if (op == CUBLAS_OP_N) return z(A[i + (size_t)j * lda]);
    zd v = z(A[j + (size_t)i * lda]);
    return op == CUBLAS_OP_C ? std::conj(v) : v;
}
template <typename T>
cublasStatus_t gemv(cublasOperation_t tr, int m, int n, const T *alpha, const T *A, int lda,
                    const T *x, int incx, const T *beta, T *y, int incy)
{
    /* y = alpha op(A) x + beta y, A is m x n */
    const int rows = tr == CUBLAS_OP_N ? m : n, cols = tr == CUBLAS_OP_N ? n : m;
    const zd a = z(*alpha), b = z(*beta);
    for (int i = 0; i < rows; ++i) {
        zd acc = 0;
        for (int k = 0; k < cols; ++k) {
            zd ak = tr == CUBLAS_OP_N ? z(A[i + (size_t)k * lda]) : z(A[k + (size_t)i * lda]);
            if (tr == CUBLAS_OP_C) ak = std::conj(ak);
            acc += ak * z(x[(size_t)k * incx]);
        }
        T &yi = y[(size_t)i * incy];
        put(yi, a * acc + (b == zd(0) ? zd(0) : b * z(yi)));
    }
    return CUBLAS_STATUS_SUCCESS;
}
}  // namespace refblas

/* C = alpha op(A) op(B) + beta C ; op(A) m x k, op(B) k x n */
inline cublasStatus_t cublasCgemm(cublasHandle_t, cublasOperation_t ta, cublasOperation_t tb, int m, int n, int k,
                                  const cuComplex *alpha, const cuComplex *A, int lda, const cuComplex *B, int ldb,
                                  const cuComplex *beta, cuComplex *C, int ldc)
{
    using namespace refblas;
    const zd a = z(*alpha), b = z(*beta);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < m; ++i) {
            zd acc = 0;
            for (int p = 0; p < k; ++p) acc += at(A, lda, ta, i, p) * at(B, ldb, tb, p, j);
            cuComplex &c = C[i + (size_t)j * ldc];
            put(c, a * acc + (b == zd(0) ? zd(0) : b * z(c)));
        }
    return CUBLAS_STATUS_SUCCESS;
}

/* y = alpha x + y */
inline cublasStatus_t cublasCaxpy(cublasHandle_t, int n, const cuComplex *alpha, const cuComplex *x, int incx,
                                  cuComplex *y, int incy)
{
    using namespace refblas;
    const zd a = z(*alpha);
    for (int i = 0; i < n; ++i) {
        cuComplex &yi = y[(size_t)i * incy];
        put(yi, a * z(x[(size_t)i * incx]) + z(yi));
    }
    return CUBLAS_STATUS_SUCCESS;
}

/* C = alpha op(A) + beta op(B), all m x n ; B is not read when beta == 0 */
inline cublasStatus_t cublasCgeam(cublasHandle_t, cublasOperation_t ta, cublasOperation_t tb, int m, int n,
                                  const cuComplex *alpha, const cuComplex *A, int lda, const cuComplex *beta,
                                  const cuComplex *B, int ldb, cuComplex *C, int ldc)
{
    using namespace refblas;
    const zd a = z(*alpha), b = z(*beta);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < m; ++i) {
            zd v = a * at(A, lda, ta, i, j);
            if (b != zd(0)) v += b * at(B, ldb, tb, i, j);
            put(C[i + (size_t)j * ldc], v);
        }
    return CUBLAS_STATUS_SUCCESS;
}

inline cublasStatus_t cublasCgemv(cublasHandle_t, cublasOperation_t tr, int m, int n, const cuComplex *alpha,
                                  const cuComplex *A, int lda, const cuComplex *x, int incx, const cuComplex *beta,
                                  cuComplex *y, int incy)
{
    return refblas::gemv(tr, m, n, alpha, A, lda, x, incx, beta, y, incy);
}

inline cublasStatus_t cublasZgemv(cublasHandle_t, cublasOperation_t tr, int m, int n, const cuDoubleComplex *alpha,
                                  const cuDoubleComplex *A, int lda, const cuDoubleComplex *x, int incx,
                                  const cuDoubleComplex *beta, cuDoubleComplex *y, int incy)
{
    return refblas::gemv(tr, m, n, alpha, A, lda, x, incx, beta, y, incy);
}

#endif
