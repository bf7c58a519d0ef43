/*
 * Host stand-in for the CUDA runtime, used only to compile the reference's
 * kernels as ordinary C++ (oracle/build_ref.py).  TEST INFRASTRUCTURE ONLY.
 *
 * Device memory is host memory: cudaMalloc hands out zeroed heap blocks and
 * remembers them, so that a memset aimed at something that is not such a block
 * fails the way the real runtime fails (cudaErrorInvalidValue, nothing
 * written) instead of scribbling over the host stack.  Streams and events do
 * nothing; every copy is synchronous.
 *
 * A kernel launch is rewritten by the recipe into ref_launch(kernel, grid,
 * block, args...), which calls the kernel once per (block, thread), serially,
 * with the index globals set.  That is exact only for kernels without
 * barriers, warp shuffles or cross-thread traffic: the recipe refuses sources
 * that have them.
 */
#ifndef GSDR_REF_CUDA_RUNTIME_H
#define GSDR_REF_CUDA_RUNTIME_H

#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sys/types.h>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static

struct __attribute__((aligned(8))) float2 { float x, y; };
struct __attribute__((aligned(16))) double2 { double x, y; };
typedef float2 cuFloatComplex;
typedef float2 cuComplex;
typedef double2 cuDoubleComplex;

inline cuComplex make_cuComplex(float r, float i) { cuComplex c; c.x = r; c.y = i; return c; }
inline float2 make_float2(float r, float i) { float2 c; c.x = r; c.y = i; return c; }

struct uint3 { unsigned int x, y, z; };
struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int a = 1, unsigned int b = 1, unsigned int c = 1) : x(a), y(b), z(c) {}
};

/* defined once, in oracle/ref/ref_driver.cpp */
extern thread_local uint3 threadIdx, blockIdx;
extern thread_local dim3 blockDim, gridDim;

template <typename... P, typename... A>
void ref_launch(void (*kernel)(P...), dim3 grid, dim3 block, A... args)
{
    gridDim = grid;
    blockDim = block;
    for (unsigned bz = 0; bz < grid.z; ++bz)
        for (unsigned by = 0; by < grid.y; ++by)
            for (unsigned bx = 0; bx < grid.x; ++bx)
                for (unsigned tz = 0; tz < block.z; ++tz)
                    for (unsigned ty = 0; ty < block.y; ++ty)
                        for (unsigned tx = 0; tx < block.x; ++tx) {
                            blockIdx.x = bx; blockIdx.y = by; blockIdx.z = bz;
                            threadIdx.x = tx; threadIdx.y = ty; threadIdx.z = tz;
                            kernel(args...);
                        }
}

/* CUDA's math headers give host code the float overloads (sin(float) is
 * sinf) at global scope; plain <cmath> would leave only the double ones there. */
using std::sin; using std::cos; using std::tan; using std::exp; using std::log; using std::pow;
using std::sqrt; using std::fabs; using std::floor; using std::ceil; using std::round;

/* ---- maths the device library provides, in double ---------------------- */
inline double ref_reduce_pi(double x) { return std::remainder(x, 2.0); } /* exact, in [-1, 1] */
inline void sincospi(double x, double *s, double *c)
{
    const double r = ref_reduce_pi(x);
    *s = std::sin(M_PI * r);
    *c = std::cos(M_PI * r);
}
inline void sincospif(float x, float *s, float *c)
{
    double sd, cd;
    sincospi((double)x, &sd, &cd);
    *s = (float)sd;
    *c = (float)cd;
}
inline double sinpi(double x) { return std::sin(M_PI * ref_reduce_pi(x)); }
inline double cospi(double x) { return std::cos(M_PI * ref_reduce_pi(x)); }

/* one thread at a time: the plain read-modify-write is the atomic */
inline float atomicAdd(float *a, float v) { float o = *a; *a = o + v; return o; }
inline double atomicAdd(double *a, double v) { double o = *a; *a = o + v; return o; }
inline int atomicAdd(int *a, int v) { int o = *a; *a = o + v; return o; }

/* ---- runtime ----------------------------------------------------------- */
typedef enum { cudaSuccess = 0, cudaErrorInvalidValue = 1, cudaErrorMemoryAllocation = 2 } cudaError_t;
typedef enum {
    cudaMemcpyHostToHost = 0, cudaMemcpyHostToDevice = 1, cudaMemcpyDeviceToHost = 2,
    cudaMemcpyDeviceToDevice = 3, cudaMemcpyDefault = 4
} cudaMemcpyKind;
typedef struct ref_cuda_stream *cudaStream_t;
typedef struct ref_cuda_event *cudaEvent_t;
#define cudaStreamDefault 0x0
#define cudaStreamNonBlocking 0x1

/* start -> size of every live cudaMalloc block */
inline std::map<const char *, size_t> &ref_device_blocks()
{
    static std::map<const char *, size_t> blocks;
    return blocks;
}
inline bool ref_is_device(const void *p, size_t n)
{
    const char *c = static_cast<const char *>(p);
    auto &b = ref_device_blocks();
    auto it = b.upper_bound(c);
    if (it == b.begin()) return false;
    --it;
    return c >= it->first && c + n <= it->first + it->second;
}

inline cudaError_t cudaMalloc(void **p, size_t n)
{
    char *m = static_cast<char *>(std::calloc(n ? n : 1, 1));
    *p = m;
    if (!m) return cudaErrorMemoryAllocation;
    ref_device_blocks()[m] = n;
    return cudaSuccess;
}
template <typename T>
cudaError_t cudaMalloc(T **p, size_t n) { return cudaMalloc(reinterpret_cast<void **>(p), n); }
inline cudaError_t cudaFree(void *p)
{
    if (!p) return cudaSuccess;
    auto &b = ref_device_blocks();
    auto it = b.find(static_cast<const char *>(p));
    if (it == b.end()) return cudaErrorInvalidValue;
    b.erase(it);
    std::free(p);
    return cudaSuccess;
}
inline cudaError_t cudaMemcpy(void *d, const void *s, size_t n, cudaMemcpyKind)
{
    if (n) std::memmove(d, s, n);
    return cudaSuccess;
}
inline cudaError_t cudaMemcpyAsync(void *d, const void *s, size_t n, cudaMemcpyKind k, cudaStream_t = 0)
{
    return cudaMemcpy(d, s, n, k);
}
inline cudaError_t cudaMemset(void *p, int v, size_t n)
{
    if (!ref_is_device(p, n)) return cudaErrorInvalidValue;
    std::memset(p, v, n);
    return cudaSuccess;
}
inline cudaError_t cudaMemsetAsync(void *p, int v, size_t n, cudaStream_t = 0) { return cudaMemset(p, v, n); }

inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline cudaError_t cudaDeviceGetStreamPriorityRange(int *lo, int *hi) { if (lo) *lo = 0; if (hi) *hi = -1; return cudaSuccess; }
inline cudaError_t cudaStreamCreate(cudaStream_t *s) { *s = nullptr; return cudaSuccess; }
inline cudaError_t cudaStreamCreateWithFlags(cudaStream_t *s, unsigned) { *s = nullptr; return cudaSuccess; }
inline cudaError_t cudaStreamCreateWithPriority(cudaStream_t *s, unsigned, int) { *s = nullptr; return cudaSuccess; }
inline cudaError_t cudaStreamSynchronize(cudaStream_t) { return cudaSuccess; }
inline cudaError_t cudaStreamDestroy(cudaStream_t) { return cudaSuccess; }
inline cudaError_t cudaEventCreate(cudaEvent_t *e) { *e = nullptr; return cudaSuccess; }
inline cudaError_t cudaEventRecord(cudaEvent_t, cudaStream_t = 0) { return cudaSuccess; }
inline cudaError_t cudaEventSynchronize(cudaEvent_t) { return cudaSuccess; }
inline cudaError_t cudaEventDestroy(cudaEvent_t) { return cudaSuccess; }
inline cudaError_t cudaGetLastError() { return cudaSuccess; }
inline cudaError_t cudaSetDevice(int) { return cudaSuccess; }
inline const char *cudaGetErrorString(cudaError_t) { return "host stand-in"; }

#endif
